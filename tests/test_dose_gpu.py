"""GPU tests of emdenoise.dose (csrc/dose.hip) against the restatement of tests/dose_ref.py.  Every comparison is
equality of bits: the arithmetic is all-integer.

Shapes, relative to the module constants (TILE = 2048 pixels a tile, SCAN_STEP = 256 tiles a step of the scan of the tiles' sums,
COARSE = 2048 entries of the draw kernel's table): 2 x 2, 3 x 5, 31 x 33, 32 x 32 and 25 x 41 are within one tile, with odd pixel
counts (an odd count in a batch takes the tile scan's 8-byte stores); 23 x 89 is one pixel fewer than a tile, 32 x 64 one tile,
3 x 683 one pixel more; 130 x 253 is the first size of this list whose table spacing is above the least (32
pixels, the last entry short); 513 x 1025 is 257 tiles, one more than a step of the scan of the sums; 2049 x 2048 is one row more than
TILE COARSE pixels, so the table's entries are more than a tile apart (the table's spacing is n / COARSE pixels rounded up to a multiple
of 16: 16 for the small shapes, 272 for 513 x 1025, 2064 here).  Batches of 3, the last two shapes alone.  Outputs and
workspaces sit between guard bands (tests/guarded.py; int32 and int64 buffers are views of its float32 and float64 ones)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from emdenoise import _lib, dose
from tests import dose_ref as R
from tests.guarded import assert_written, guarded

pytestmark = pytest.mark.gpu

T, CO = dose.TILE, dose.COARSE
assert (T, CO, dose.SCAN_STEP) == (2048, 2048, 256)
SMALL = [(2, 2), (3, 5), (31, 33), (32, 32), (25, 41), (23, 89), (32, 64), (3, 683), (130, 253)]
assert 23 * 89 == T - 1 and 32 * 64 == T and 3 * 683 == T + 1
STEP_PLUS = (513, 1025)
assert -(-513 * 1025 // T) == dose.SCAN_STEP + 1
TABLE_PLUS = (T * CO // 2048 + 1, 2048)
assert TABLE_PLUS[0] * TABLE_PLUS[1] == T * CO + 2048 and -(-TABLE_PLUS[0] * TABLE_PLUS[1] // T) == CO + 1
SHAPES = SMALL + [STEP_PLUS, TABLE_PLUS]
KINDS = ["positive", "zero_runs", "one_pixel", "constant", "wild", "all_zero"]
SEED, FIRST_IMAGE = 0x9E3779B97F4A7C15, 5
ids = lambda s: f"{s[0]}x{s[1]}"


def dev():
    return torch.device("cuda", 0)


def batch_of(shape):
    return 1 if shape in (STEP_PLUS, TABLE_PLUS) else 3


def draws_of(shape):
    return 1000000 if shape == TABLE_PLUS else 5 * shape[0] * shape[1] + 3


@functools.lru_cache(maxsize=None)
def images(kind, B, H, W):
    rng = np.random.default_rng(1000 * H + W + 31 * KINDS.index(kind))
    n = H * W
    if kind == "positive":
        x = rng.random((B, n)) + 0.01
    elif kind == "zero_runs":                       # runs of zeros that include the first and the last pixel
        x = rng.random((B, n)) + 0.01
        for b in range(B):
            x[b, : 1 + n // 7] = 0
            x[b, n - 1 - n // 5:] = 0
            x[b, n // 2: n // 2 + n // 9 + 1] = 0
            if n == 4:
                x[b, 1 + b % 2] = 0.5
    elif kind == "one_pixel":
        x = np.zeros((B, n))
        for b in range(B):
            x[b, (n - 1) * b // max(B - 1, 1) if B > 1 else n // 3] = 2.5 + b
    elif kind == "constant":
        x = np.full((B, n), 0.37)
    elif kind == "wild":                            # 1e-30 .. 1e30 mixed with NaN, +-inf and negatives
        x = 10.0 ** rng.uniform(-30, 30, (B, n))
        what = rng.integers(0, 12, (B, n))
        x[what == 0] = np.nan
        x[what == 1] = np.inf
        x[what == 2] = -np.inf
        x[what == 3] *= -1
        x[what == 4] = -0.0
    else:
        x = np.zeros((B, n))
    x = x.astype(np.float32).reshape(B, H, W)
    x.setflags(write=False)                         # shared: nobody writes it
    return x


@functools.lru_cache(maxsize=None)
def ref_cdf(kind, B, H, W):
    pairs = [R.cdf(im) for im in images(kind, B, H, W)]
    c = np.stack([p[0] for p in pairs])
    c.setflags(write=False)
    return c, np.array([p[1] for p in pairs], np.int32)


def i64(view):
    return view.view(torch.int64)


def i32(view):
    return view.view(torch.int32)


def cdf_c(x):
    """emd_dose_cdf_i64 on guarded buffers -> (cdf [B,H,W] int64 device tensor, status numpy)."""
    B, H, W = x.shape
    lib = _lib.load()
    need = lib.emd_dose_workspace_bytes(B, H, W)
    assert need > 0 and need % 16 == 0
    xin, gx = guarded(x.size, torch.float32, dev(), fill=np.array(x), name="x")
    out, go = guarded(x.size, torch.float64, dev(), name="cdf")
    st, gs = guarded(B, torch.float32, dev(), name="status")
    ws, gw = guarded(need // 8, torch.float64, dev(), name="workspace")
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(lib.emd_dose_cdf_i64(p(xin), B, H, W, p(out), p(st), p(ws), need, _lib.stream_ptr()), "emd_dose_cdf_i64")
    torch.cuda.synchronize()
    for g in (gx, go, gs, gw):
        g()
    assert_written(out, "cdf")
    assert_written(st, "status")
    assert np.array_equal(xin.cpu().numpy().view(np.int32), np.ascontiguousarray(x).ravel().view(np.int32)), "the input was written"
    return i64(out).view(B, H, W), i32(st).cpu().numpy()


def draw_c(cdf, bounds, planes_fill=0, first_image=FIRST_IMAGE, seed=SEED):
    """emd_dose_draw_i32 on a guarded planes buffer pre-loaded with planes_fill -> planes [B,L,H,W] int32 device tensor."""
    B, H, W = cdf.shape
    L = len(bounds) - 1
    pl, gp = guarded(B * L * H * W, torch.float32, dev(), name="planes")
    planes = i32(pl)
    planes.copy_(torch.as_tensor(np.broadcast_to(np.asarray(planes_fill, np.int32), (B, L, H, W)).reshape(-1)).to(dev()))
    arr = (C.c_int64 * (L + 1))(*bounds)
    _lib.check(_lib.load().emd_dose_draw_i32(C.c_void_p(cdf.data_ptr()), B, H, W, seed, first_image, arr, L, C.c_void_p(planes.data_ptr()),
                                             _lib.stream_ptr()), "emd_dose_draw_i32")
    torch.cuda.synchronize()
    gp()
    return planes.view(B, L, H, W)


# ---- CDF and status ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_cdf_and_status_bitwise(shape, kind):
    B = batch_of(shape)
    x = images(kind, B, *shape)
    want, want_status = ref_cdf(kind, B, *shape)
    got, status = cdf_c(x)
    got = got.cpu().numpy()
    assert np.array_equal(status, want_status), (status, want_status)
    assert np.array_equal(got, want), int((got != want).sum())
    if kind == "all_zero":
        assert (status == dose.EMPTY).all() and not got.any()
    if kind == "wild" and shape[0] * shape[1] >= 1000:          # a third of the pixels is negative or not finite
        assert (status == dose.SANITIZED).all()


def test_cdf_wrapper_conventions():
    x = images("wild", 3, 25, 41)
    want, want_status = ref_cdf("wild", 3, 25, 41)
    c, s = dose.cdf(x, return_status=True)
    assert isinstance(c, np.ndarray) and c.dtype == np.int64 and np.array_equal(c, want) and np.array_equal(s, want_status)
    ct = dose.cdf(torch.from_numpy(np.array(x)).to(dev()))
    assert ct.is_cuda and ct.dtype == torch.int64 and np.array_equal(ct.cpu().numpy(), want)
    assert np.array_equal(dose.cdf(x[1]), want[1])
    # an image's CDF does not depend on the batch it is in
    assert np.array_equal(dose.cdf(np.ascontiguousarray(x[2:])), want[2:])


# ---- counts ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_counts_bitwise(shape, kind):
    """draws = 5 H W + 3 (10^6 at the largest shape) from an odd first draw, first_image = 5: the batch equals the restatement image
    by image, and image b equals the single-image call with first_image = 5 + b."""
    B = batch_of(shape)
    H, W = shape
    x = images(kind, B, H, W)
    first, D = 7, draws_of(shape)
    cdf = torch.from_numpy(np.array(ref_cdf(kind, B, H, W)[0])).to(dev())
    got = draw_c(cdf, [first, first + D])[:, 0].cpu().numpy()
    for b in range(B):
        want = R.sample_counts(x[b], D, seed=SEED, first_draw=first, image=FIRST_IMAGE + b)
        assert np.array_equal(got[b], want), (b, int((got[b] != want).sum()))
        assert int(got[b].sum()) == (0 if kind == "all_zero" else D)
    if B > 1:
        b = B - 1
        alone = draw_c(cdf[b:].contiguous(), [first, first + D], first_image=FIRST_IMAGE + b)[0, 0].cpu().numpy()
        assert np.array_equal(alone, got[b])


def test_sample_counts_wrapper_and_zero_weight_pixels():
    x = images("zero_runs", 3, 31, 33)
    D = 5 * 31 * 33 + 3
    got = dose.sample_counts(x, D, seed=SEED, first_draw=7, first_image=FIRST_IMAGE)
    assert isinstance(got, np.ndarray) and got.dtype == np.int32 and got.shape == x.shape
    for b in range(3):
        assert np.array_equal(got[b], R.sample_counts(x[b], D, seed=SEED, first_draw=7, image=FIRST_IMAGE + b))
    assert not got[x == 0].any() and (got.reshape(3, -1).sum(1) == D).all()
    one = dose.sample_counts(torch.from_numpy(np.array(x[1])).to(dev()), D, seed=SEED, first_draw=7, first_image=FIRST_IMAGE + 1)
    assert one.is_cuda and tuple(one.shape) == (31, 33) and np.array_equal(one.cpu().numpy(), got[1])


@pytest.mark.parametrize("shape", [(25, 41), STEP_PLUS], ids=ids)
def test_split_calls_add_up(shape):
    """Draws [0, D) in one call equal [0, a) then [a, D) with odd a, added into the same buffer."""
    B = batch_of(shape)
    H, W = shape
    D, a = 3 * H * W + 1, H * W + (H * W) % 2 + 1
    assert a % 2 == 1
    cdf = torch.from_numpy(np.array(ref_cdf("positive", B, H, W)[0])).to(dev())
    whole = draw_c(cdf, [0, D])
    part = draw_c(cdf, [0, a])
    both = draw_c(cdf, [a, D], planes_fill=part.cpu().numpy())
    assert torch.equal(whole, both) and int(whole[0].sum()) == D
    # the wrapper's out= adds too
    xt = torch.from_numpy(np.array(images("positive", B, H, W))).to(dev())
    out = dose.sample_counts(xt, a, seed=SEED, first_image=FIRST_IMAGE)
    assert dose.sample_counts(xt, D - a, seed=SEED, first_draw=a, first_image=FIRST_IMAGE, out=out) is out
    assert torch.equal(out, whole[:, 0])


# ---- series ------------------------------------------------------------------------------------------------------------------------
def cumulate_c(planes):
    """emd_dose_cumulate_i32 in place on a guarded copy -> (planes, minmax [B,L,2] numpy)."""
    B, L, H, W = planes.shape
    pl, gp = guarded(planes.numel(), torch.float32, dev(), name="planes")
    i32(pl).copy_(planes.reshape(-1))
    mm, gm = guarded(B * L * 2, torch.float32, dev(), name="minmax")
    _lib.check(_lib.load().emd_dose_cumulate_i32(C.c_void_p(pl.data_ptr()), B, L, H, W, C.c_void_p(mm.data_ptr()), _lib.stream_ptr()),
               "emd_dose_cumulate_i32")
    torch.cuda.synchronize()
    gp()
    gm()
    assert_written(mm, "minmax")
    return i32(pl).view(B, L, H, W), i32(mm).view(B, L, 2).cpu().numpy()


@pytest.mark.parametrize("shape", [(3, 5), (25, 41), (65, 127)], ids=ids)
def test_series_planes_are_cumulative_counts(shape):
    """The planes are the cumulative counts of their bounds and sum to them exactly; min and max are the planes' own.  65 x 127 has
    more pixels than one workgroup of the cumulate kernel takes (4096) and is not a multiple of it."""
    H, W = shape
    B, n = 3, H * W
    x = images("zero_runs", B, H, W)
    bounds = [3, 3, n // 2, 2 * n + 1, 2 * n + 1, 7 * n]        # two empty levels, an odd start
    cdf = torch.from_numpy(np.array(ref_cdf("zero_runs", B, H, W)[0])).to(dev())
    inc = draw_c(cdf, bounds)
    cum, minmax = cumulate_c(inc)
    cum = cum.cpu().numpy()
    assert np.array_equal(cum, np.cumsum(inc.cpu().numpy(), axis=1, dtype=np.int64))
    for b in range(B):
        assert np.array_equal(cum[b], R.series(x[b], bounds, SEED, FIRST_IMAGE + b))
        assert [int(p.sum()) for p in cum[b]] == [v - bounds[0] for v in bounds[1:]]
    flat = cum.reshape(B, len(bounds) - 1, -1)
    assert np.array_equal(minmax[..., 0], flat.min(2)) and np.array_equal(minmax[..., 1], flat.max(2))


def test_dose_series_equals_sample_counts_level_by_level():
    x = images("positive", 3, 25, 41)
    avg = (0.5, 2, 4.25)
    s = dose.dose_series(x, avg, seed=SEED, first_image=FIRST_IMAGE)
    assert s.dtype == np.int32 and s.shape == (3, 3, 25, 41)
    for k, a in enumerate(avg):
        D = int(round(a * 25 * 41))
        assert np.array_equal(s[:, k], dose.sample_counts(x, D, seed=SEED, first_image=FIRST_IMAGE)) and (s[:, k].reshape(3, -1).sum(1) == D).all()
    one, status = dose.dose_series(x[2], avg, seed=SEED, first_image=FIRST_IMAGE + 2, return_status=True)
    assert one.shape == (3, 25, 41) and np.array_equal(one, s[2]) and status.tolist() == [0]
    empty, status = dose.dose_series(images("all_zero", 3, 25, 41), avg, rescale="uint16", return_status=True)
    assert not empty.any() and (status == dose.EMPTY).all()


def test_lq_img_gen_equals_the_restatement():
    img = np.array(images("positive", 3, 31, 33)[1]) * 900.0
    got = dose.lq_img_gen(img, [2, 4, 9], 2, seed=11)
    want = R.lq_img_gen(img, [2, 4, 9], 2, seed=11)
    assert len(got) == 3 and all(g.dtype == np.uint16 and g.shape == (31, 33) for g in got)
    for g, w in zip(got, want):
        assert np.array_equal(g, w) and g.max() == 65535 and g.min() == 0
    levels = dose.lq_levels([2, 4, 9], 2, img.size)
    assert np.array_equal(dose.dose_series(img.astype(np.float32), [2, 4, 8], seed=11)[2].sum(), levels[2])


# ---- rescale -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["uint16", "unit"])
def test_rescale_bitwise_and_flat_planes(mode):
    B, L, H, W = 2, 3, 33, 47
    rng = np.random.default_rng(9)
    counts = rng.poisson(40.0, (B, L, H, W)).astype(np.int32)
    counts[0, 1] = 13                                              # a flat plane: zeros, where the reference divides by zero
    counts[1, 2] = 0
    counts[1, 0, 0, 0] = 100000                                    # a long range: quotients that are not short binary fractions
    planes = torch.from_numpy(counts).to(dev())
    same, minmax = cumulate_c(planes.view(B * L, 1, H, W))         # one level: the planes stay, min and max are written
    assert torch.equal(same.view(B, L, H, W), planes)
    out, go = guarded(counts.size, torch.float32, dev(), name="out")
    mm = torch.from_numpy(minmax).to(dev())
    _lib.check(_lib.load().emd_dose_rescale(C.c_void_p(planes.data_ptr()), C.c_void_p(mm.data_ptr()), B, L, H, W, dose.MODES[mode],
                                            C.c_void_p(out.data_ptr()), _lib.stream_ptr()), "emd_dose_rescale")
    torch.cuda.synchronize()
    go()
    assert_written(out, "out")
    got = (i32(out) if mode == "uint16" else out).view(B, L, H, W).cpu().numpy()
    word = np.int32 if mode == "uint16" else np.float32
    for b in range(B):
        for k in range(L):
            want = R.rescale(counts[b, k], mode)
            assert got[b, k].dtype == want.dtype == word and np.array_equal(got[b, k].view(np.int32), want.view(np.int32)), (b, k)
    assert not got[0, 1].any() and not got[1, 2].any()
    w = dose.rescale_counts(counts, mode)
    assert isinstance(w, np.ndarray) and np.array_equal(w.view(np.int32), got.view(np.int32))
    wt = dose.rescale_counts(planes[0, 0], mode)
    assert wt.is_cuda and np.array_equal(wt.cpu().numpy().view(np.int32), got[0, 0].view(np.int32))


@pytest.mark.parametrize("mode", ["uint16", "unit"])
def test_dose_series_rescaled_equals_the_restatement(mode):
    x = images("zero_runs", 3, 25, 41)
    avg = (1, 3, 6.5)
    got = dose.dose_series(x, avg, seed=SEED, first_image=FIRST_IMAGE, rescale=mode)
    bounds = [0] + [int(round(a * 25 * 41)) for a in avg]
    for b in range(3):
        s = R.series(x[b], bounds, SEED, FIRST_IMAGE + b)
        for k in range(3):
            assert np.array_equal(got[b, k].view(np.int32), R.rescale(s[k], mode).view(np.int32)), (b, k)


# ---- capture -----------------------------------------------------------------------------------------------------------------------
def test_dose_series_captured_in_a_graph_gives_the_eager_bits():
    x = torch.from_numpy(np.array(images("zero_runs", 3, 31, 33))).to(dev())
    avg = (1, 2.5, 5)
    eager = dose.dose_series(x, avg, seed=SEED, first_image=FIRST_IMAGE, rescale="uint16")
    counts = dose.dose_series(x, avg, seed=SEED, first_image=FIRST_IMAGE)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        dose.dose_series(x, avg, seed=SEED, first_image=FIRST_IMAGE, rescale="uint16")      # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        a = dose.dose_series(x, avg, seed=SEED, first_image=FIRST_IMAGE, rescale="uint16")
        b = dose.dose_series(x, avg, seed=SEED, first_image=FIRST_IMAGE)
    for _ in range(2):
        a.fill_(-1)
        b.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(a, eager) and torch.equal(b, counts)
