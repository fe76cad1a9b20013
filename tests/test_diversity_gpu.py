"""GPU tests of emdenoise.diversity (csrc/diversity.hip) against the restatement of tests/diversity_ref.py.

Every entry point is called through the C ABI with its outputs and its workspace between guard bands (tests/guarded.py), and the
image stack is itself a view between two bands of NaN: a read outside an image poisons the result, a write outside an output is
caught.  Shapes, with T = TILE, KB = TILE_K, KC = CHAIN: one row pair and one column; less than a k block; one row and one column
short of / past a tile, a k block, a chain; three tiles a side with two chains and a ragged block; many tiles with few columns and
the reverse; and (T + 1) x 2048, eight chains folded into the total.

Integer images (0..15) make every product, partial sum, E^2 and tile sum exact in float32 and double (the bound is asserted), so the
results must equal int64 arithmetic bit for bit whatever the order of accumulation.  Float images: ``row_distances`` within 4 x the
float32 restatement's own relative L2 distance from the float64 restatement; the pair statistic within 4 (2 eta + eta^2) relative,
eta the float32 restatement's relative L2 error of the matrix D(a) - D(b) (ssd is that matrix's mean square, so a relative error eta
of the matrix moves it by at most 2 eta + eta^2; the scalar's own float32 error is a signed accident and no yardstick).  Both
distances are computed here at run time and every figure is printed before it is asserted."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from emdenoise import _lib, diversity
from tests import diversity_ref as R
from tests.guarded import assert_written, guarded

pytestmark = pytest.mark.gpu

T, KB, KC = diversity.TILE, diversity.TILE_K, diversity.CHAIN
SHAPES = [(2, 1), (3, KB - 1), (T - 1, KB + 1), (T, KC), (T + 1, KC - 1), (T + 1, KC + 1), (2 * T + 3, 2 * KC + KB + 5), (5, 2 * T + 3),
          (2 * T + 3, 5)]
LONG = (T + 1, 2048)                                   # B = 2, one pair
FLOAT_SHAPES = [s for s in SHAPES if s[0] >= T - 1] + [LONG]
PAIRS3 = np.array([[0, 1], [0, 2], [1, 2], [1, 1]], np.int32)


def dev():
    return torch.device("cuda", 0)


def ptr(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return _lib.stream_ptr()


def guarded_images(x, shift=0):
    """x [B,H,W] float32 -> (device view between two NaN bands, check); shift: floats by which the view is moved off its 256-byte
    alignment (the 16-byte loads need an aligned stack; the 4-byte ones must give the same bits)."""
    view, g = guarded(x.size + shift, torch.float32, dev(), name="x")
    view = view[shift:]
    view.copy_(torch.from_numpy(np.ascontiguousarray(x)).reshape(-1))
    return view, g


def guarded_i32(n, name):
    view, g = guarded(n, torch.float32, dev(), name=name)
    return view, view.view(torch.int32), g


def call_norms(x):
    B, H, W = x.shape
    xin, gx = guarded_images(x)
    norms, gn = guarded(B * H, torch.float64, dev(), name="norms")
    raw, bad, gb = guarded_i32(B, "nonfinite")
    _lib.check(_lib.load().emd_row_sq_norms_f64(ptr(xin), B, H, W, ptr(norms), ptr(raw), stream()), "emd_row_sq_norms_f64")
    torch.cuda.synchronize()
    for g in (gx, gn, gb):
        g()
    assert_written(norms, "norms")
    assert_written(raw, "nonfinite")
    return norms.cpu().numpy().reshape(B, H), bad.cpu().numpy()


def call_distances(x, shift=0):
    B, H, W = x.shape
    lib = _lib.load()
    xin, gx = guarded_images(x, shift)
    D, gd = guarded(B * H * H, torch.float32, dev(), name="D")
    need = lib.emd_row_distances_workspace_bytes(B, H, W)
    ws, gw = guarded(need // 8, torch.float64, dev(), name="workspace")
    _lib.check(lib.emd_row_distances_f32(ptr(xin), B, H, W, ptr(D), ptr(ws), need, stream()), "emd_row_distances_f32")
    torch.cuda.synchronize()
    for g in (gx, gd, gw):
        g()
    if not np.isnan(x).any():
        assert_written(D, "D")
    return D.cpu().numpy().reshape(B, H, H)


def call_pairs(x, pairs, shift=0):
    B, H, W = x.shape
    P = len(pairs)
    lib = _lib.load()
    xin, gx = guarded_images(x, shift)
    pin, gp = guarded_i32(2 * P, "pairs")[1:]
    pin.copy_(torch.from_numpy(np.ascontiguousarray(pairs, dtype=np.int32)).reshape(-1))
    ssd, gs = guarded(P, torch.float64, dev(), name="ssd")
    raw, status, gt = guarded_i32(P, "status")
    need = lib.emd_gram_ssd_workspace_bytes(B, H, W, P)
    ws, gw = guarded(need // 8, torch.float64, dev(), name="workspace")
    _lib.check(lib.emd_gram_ssd_f64(ptr(xin), B, H, W, ptr(pin), P, ptr(ssd), ptr(raw), ptr(ws), need, stream()), "emd_gram_ssd_f64")
    torch.cuda.synchronize()
    for g in (gx, gp, gs, gt, gw):
        g()
    assert_written(ssd, "ssd")
    assert_written(raw, "status")
    return ssd.cpu().numpy(), status.cpu().numpy()


def bits(a):
    return np.asarray(a, np.float64).view(np.int64)


@functools.lru_cache(maxsize=None)
def int_images(H, W):
    x = np.random.default_rng([H, W]).integers(0, 16, (3, H, W)).astype(np.float32)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("H,W", SHAPES)
def test_integer_images_are_exact(H, W):
    """Pixels 0..15: a product is at most 225, a chain's partial sum and G at most 225 W < 2^24 (exact in float32), |E| = |D(a) - D(b)|
    at most 225 W with D a squared distance, and the whole sum at most H^2 (225 W)^2 < 2^53 (exact in double): no rounding anywhere,
    so the order of accumulation cannot matter and every output equals int64 arithmetic."""
    assert 225 * W < 2 ** 24 and H * H * (225 * W) ** 2 < 2 ** 53
    x = int_images(H, W)
    norms, bad = call_norms(x)
    assert np.array_equal(norms, (x.astype(np.int64) ** 2).sum(axis=2)) and not bad.any()
    D = call_distances(x)
    for b in range(3):
        want = R.int_distances(x[b])
        wrong = np.argwhere(D[b] != want)
        assert wrong.size == 0, f"image {b}: {len(wrong)} elements of D differ, the first at {tuple(wrong[0])}"
    ssd, status = call_pairs(x, PAIRS3)
    assert not status.any()
    for (i, j), got in zip(PAIRS3, ssd):
        s, count = R.int_ssd(x[i], x[j])
        assert got == s / count, ((i, j), got, s / count)            # int / int: the correctly rounded quotient, as the device's
    assert ssd[3] == 0.0


@functools.lru_cache(maxsize=None)
def float_case(kind, H, W):
    """The images and both restatements, computed once per case."""
    B = 2 if (H, W) == LONG else 3
    x = R.images(kind, B, H, W, seed=3)
    x.setflags(write=False)
    d64 = [R.row_distances(x[b], np.float64) for b in range(B)]
    d32 = [R.row_distances(x[b], np.float32) for b in range(B)]
    return x, d64, d32


@pytest.mark.parametrize("H,W", FLOAT_SHAPES)
@pytest.mark.parametrize("kind", R.KINDS)
def test_float_images_within_four_times_float32(kind, H, W):
    x, d64, d32 = float_case(kind, H, W)
    B = x.shape[0]
    D = call_distances(x)
    for b in range(B):
        got, bar = R.rel_l2(D[b], d64[b]), 4 * R.rel_l2(d32[b], d64[b])
        print(f"{kind} {H} x {W} image {b}: D rel L2 from float64 {got:.3e}, float32 restatement {bar / 4:.3e} ({got / (bar / 4):.2f} x)")
        assert got <= bar, (kind, H, W, b, got, bar)
        assert np.array_equal(D[b], D[b].T)
    pairs = np.array([[0, 1], [0, 0]], np.int32) if B == 2 else PAIRS3
    ssd, status = call_pairs(x, pairs)
    assert not status.any()
    for (i, j), got in zip(pairs, ssd):
        if i == j:
            assert got == 0.0 and not np.signbit(got)
            continue
        want_m = d64[i] - d64[j]
        want = float((want_m * want_m).mean())
        eta = R.rel_l2(d32[i].astype(np.float32) - d32[j], want_m)
        bar = 4 * (2 * eta + eta * eta)
        rel = abs(got - want) / want
        print(f"{kind} {H} x {W} pair ({i},{j}): ssd {got:.9e}, float64 {want:.9e}, relative {rel:.3e}; eta {eta:.3e}, bar {bar:.3e} "
              f"({rel / (bar / 4):.2f} x of 2 eta + eta^2)")
        assert rel <= bar, (kind, H, W, (i, j), rel, bar)


def test_row_norms_of_float_images_in_the_stated_order():
    """The norms' order of addition is part of the contract: the restatement that follows it gives the same bits."""
    for H, W in ((T + 1, KC + 1), (5, 2 * T + 3), (3, KB - 1)):
        x = R.images("fringe", 3, H, W, seed=5)
        norms, bad = call_norms(x)
        assert np.array_equal(bits(norms), bits(R.row_sq_norms(x))) and not bad.any()


def test_bitwise_properties():
    H, W = T + 1, KC + 1
    six = R.images("uniform", 6, H, W, seed=9)
    three = six[:3]
    base, status = call_pairs(three, np.array([[0, 1], [1, 0], [2, 2], [1, 2]], np.int32))
    assert not status.any()
    assert base[2] == 0.0 and not np.signbit(base[2])                                       # the self-pair
    assert bits(base[0]) == bits(base[1]) and base[0] > 0                                   # (i, j) and (j, i)
    alone = call_pairs(three, np.array([[0, 1]], np.int32))[0]
    last = call_pairs(three, np.array([[1, 2], [2, 0], [2, 1], [0, 1]], np.int32))[0]
    in_six = call_pairs(six, np.array([[4, 5], [0, 1], [3, 1]], np.int32))[0]
    assert bits(alone[0]) == bits(base[0]) == bits(last[3]) == bits(in_six[1])              # alone, first of 4, last of 4, 3 or 6 images
    assert bits(last[0]) == bits(base[3]) == bits(last[2])
    # the two-stack form is the pair list on the concatenated stack
    a, b = torch.from_numpy(six[:3]).to(dev()), torch.from_numpy(six[3:]).to(dev())
    two = diversity.gram_ssd(a, b)
    assert two.dtype == torch.float64 and two.is_cuda and tuple(two.shape) == (3,)
    cat = call_pairs(six, np.array([[0, 3], [1, 4], [2, 5]], np.int32))[0]
    assert np.array_equal(bits(two.cpu().numpy()), bits(cat))
    both, st = diversity.gram_ssd_pairs(six, np.array([[0, 3], [1, 4], [2, 5]], np.int32))   # numpy in -> numpy out
    assert isinstance(both, np.ndarray) and st.dtype == np.int32 and np.array_equal(bits(both), bits(cat))
    # D equals its transpose as bits, also across tiles
    D = call_distances(six[:2])
    assert np.array_equal(D.view(np.int32), D.transpose(0, 2, 1).view(np.int32))
    assert np.array_equal(diversity.row_distances(a[:2]).cpu().numpy().view(np.int32), D.view(np.int32))
    # W % 4 == 0: the 16-byte loads of an aligned stack and the 4-byte loads of one moved by a float give the same bits
    x4 = R.images("uniform", 3, T, KC, seed=11)
    assert np.array_equal(bits(call_pairs(x4, PAIRS3)[0]), bits(call_pairs(x4, PAIRS3, shift=1)[0]))
    assert np.array_equal(call_distances(x4).view(np.int32), call_distances(x4, shift=1).view(np.int32))


def test_status_and_skipped_pairs():
    H, W = T + 1, KB + 1
    x = R.images("uniform", 5, H, W, seed=13).copy()
    x[1, 7, 3] = np.nan
    x[2, H - 1, W - 1] = np.inf
    x[4, 0, 0], x[4, H - 1, 0], x[4, 64, W - 1] = np.nan, -np.inf, np.nan
    norms, bad = call_norms(x)
    assert bad.tolist() == [0, 1, 1, 0, 3]
    assert np.array_equal(bits(norms[[0, 3]]), bits(R.row_sq_norms(x[[0, 3]])))
    pairs = np.array([[0, 3], [0, 1], [2, 3], [-1, 0], [0, 5], [3, 0], [1, 2], [4, 4], [3, 3], [5, -7], [2 ** 31 - 1, 0]], np.int32)
    want = [0, 1, 1, 2, 2, 0, 1, 1, 0, 2, 2]
    ssd, status = call_pairs(x, pairs)
    assert status.tolist() == want
    assert np.isnan(ssd[np.array(want) != 0]).all() and np.isfinite(ssd[np.array(want) == 0]).all()
    clean, cs = call_pairs(x, pairs[np.array(want) == 0])
    assert not cs.any() and np.array_equal(bits(clean), bits(ssd[np.array(want) == 0])) and clean[2] == 0.0
    # the same through the Python layer, and the reference's skip count
    values, skipped = diversity.dataset_diversity(x)
    sched = diversity.pair_schedule(5)
    ok = [k for k, (i, j) in enumerate(sched) if bad[i] == 0 and bad[j] == 0]
    assert skipped == len(sched) - len(ok) and len(values) == len(ok) == 1 and bits(values[0]) == bits(ssd[0])


def test_captured_graph_replays_with_new_pairs_and_images():
    H, W = T + 1, KC + 1
    x = R.images("fringe", 4, H, W, seed=17)
    stack = torch.from_numpy(x[:3]).to(dev())
    other = torch.from_numpy(x[3]).to(dev())
    first = torch.tensor([[0, 1], [1, 2]], dtype=torch.int32, device=dev())
    second = torch.tensor([[2, 0], [1, 1]], dtype=torch.int32, device=dev())
    changed = stack.clone()
    changed[0].copy_(other)
    want = {"first": diversity.gram_ssd_pairs(stack, first), "second": diversity.gram_ssd_pairs(changed, second)}
    torch.cuda.synchronize()
    assert float(want["first"][0][0]) != float(want["second"][0][0])

    static, pairs = stack.clone(), first.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        diversity.gram_ssd_pairs(static, pairs)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ssd, status = diversity.gram_ssd_pairs(static, pairs)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(ssd.view(torch.int64), want["first"][0].view(torch.int64)) and torch.equal(status, want["first"][1])
    pairs.copy_(second)
    static[0].copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(ssd.view(torch.int64), want["second"][0].view(torch.int64)) and torch.equal(status, want["second"][1])
    assert float(ssd[1]) == 0.0
