"""GPU tests of the candidate crops, the reconstruction of candidate stacks and the refinement of crop centres and defocuses
(csrc/register.hip, csrc/exitwave.hip, emdenoise.exitwave).

Everything is checked through bit equality with functions that have their own tests: ``crop_candidates`` against ``crop_stack``,
``reconstruct_candidate_stacks`` against ``reconstruct`` / ``reconstruction_loss``, and every loss of the refinement's history against
``reconstruction_loss(crop_stack(...))`` at parameters rebuilt from the device's own recorded choices.  The decisions are compared
with the restatement of tests/exitwave_refine_ref.py; the margins that make them the restatement's are asserted on the CPU
(tests/test_exitwave_refine.py) before the GPU is touched."""
import numpy as np
import pytest
import torch

from emdenoise import _lib, exitwave
from tests import exitwave_ref as R
from tests import exitwave_refine_ref as RR
from tests.guarded import assert_written, guarded
from tests.test_exitwave_gpu import CS, bits, ids, up
from tests.test_exitwave_refine import MARGIN, SERIES, series_ref

pytestmark = pytest.mark.gpu

LAM, PX = R.WAVELENGTH, R.PX
# (C, N, S0, side)
CROPS = [(1, 1, 8, 8), (2, 2, 16, 8), (3, 3, 33, 9), (5, 3, 37, 16)]
# (C, N, s, pad, iterations, from_intensity, cs)
STACKS = [(1, 1, 8, 0, 1, False, 0.0), (3, 2, 16, 0, 2, False, 0.0), (2, 3, 8, 1, 2, False, 0.0), (2, 3, 16, 0, 2, True, 0.0),
          (2, 3, 16, 0, 2, False, CS)]


def centres_table(C, N, S0, side, seed=1):
    """Sub-pixel centres around the middle; the last candidate's reach outside the frame on every side, one of them far outside."""
    rng = np.random.default_rng(seed)
    t = S0 / 2.0 + rng.uniform(-2.0, 2.0, size=(C, N, 2))
    t[-1, 0] = (side / 2.0 - 1.75, S0 - side / 2.0 + 2.5)
    if N > 1:
        t[-1, 1] = (S0 + 3.0 * side, S0 / 2.0)
    return t


def stacks_of(C, N, s):
    """[C,N,s,s]: candidate c's own images, the series' scaled and shifted by whole pixels; and C different defocus tables."""
    images, df = R.series(N, s)
    st = np.stack([np.roll(images, (c, 2 * c), (1, 2)) * np.float32(1.0 + 0.125 * c) for c in range(C)])
    table = np.stack([(0.7 + 0.2 * c) * df * (1.0 if c % 2 == 0 else -1.0) for c in range(C)])
    return st, table


@pytest.mark.parametrize("case", CROPS, ids=ids)
def test_crop_candidates_equal_crop_stack_bit_for_bit(case):
    C, N, S0, side = case
    stack = up(np.random.default_rng(7).random((N, S0, S0)).astype(np.float32) + 0.5)
    table = centres_table(C, N, S0, side)
    got = exitwave.crop_candidates(stack, up(table), side, pad_val=0.25)
    assert tuple(got.shape) == (C, N, side, side) and got.dtype == torch.float32
    for c in range(C):
        assert torch.equal(got[c], exitwave.crop_stack(stack, up(table[c]), side, pad_val=0.25)), c
    assert bool((got[-1, 0] == 0.25).any())                                 # taps outside the frame were met
    if N > 1:
        assert bool((got[-1, 1] == 0.25).all())
    host = exitwave.crop_candidates(stack.cpu().numpy(), table, side, pad_val=0.25)
    assert isinstance(host, np.ndarray) and np.array_equal(host, got.cpu().numpy())


@pytest.mark.parametrize("case", STACKS, ids=ids)
def test_every_candidate_stack_equals_reconstruct_bit_for_bit(case):
    C, N, s, pad, iters, fi, cs = case
    st, table = stacks_of(C, N, s)
    x, t = up(st), up(table)
    kw = dict(px=PX, cs=cs, iterations=iters, pad_periods=pad, from_intensity=fi)
    losses, E, stack = exitwave.reconstruct_candidate_stacks(x, t, LAM, per_image=True, return_waves=True, return_stack=True, **kw)
    worst = exitwave.reconstruct_candidate_stacks(x, t, LAM, **kw)
    assert tuple(losses.shape) == (C, N) and tuple(E.shape) == (C, s, s) and tuple(stack.shape) == (C, N, s, s) and tuple(worst.shape) == (C,)
    for c in range(C):
        e1, s1, l1 = exitwave.reconstruct(x[c], t[c], LAM, return_stack=True, return_losses=True, **kw)
        assert torch.equal(bits(E[c]), bits(e1)), f"E of candidate {c}"
        assert torch.equal(bits(stack[c]), bits(s1)), f"stack of candidate {c}"
        assert torch.equal(losses[c], l1), f"losses of candidate {c}"
        assert torch.equal(worst[c], exitwave.reconstruction_loss(x[c], t[c], LAM, **kw))
    if C > 1:
        assert not torch.equal(losses[0], losses[1])


@pytest.mark.parametrize("pad", [0, 1])
def test_a_candidate_stacks_bits_do_not_depend_on_the_others_or_on_the_chunking(pad):
    st, table = stacks_of(5, 3, 16)
    kw = dict(px=PX, iterations=3, pad_periods=pad, per_image=True, return_waves=True, return_stack=True)
    full = exitwave.reconstruct_candidate_stacks(up(st), up(table), LAM, **kw)
    perm = np.array([3, 0, 4, 2, 1])
    mixed = exitwave.reconstruct_candidate_stacks(up(st[perm]), up(table[perm]), LAM, **kw)
    for a, b in zip(full, mixed):
        assert torch.equal(bits(a[perm]), bits(b))
    for c in (0, 2, 4):
        alone = exitwave.reconstruct_candidate_stacks(up(st[c:c + 1]), up(table[c:c + 1]), LAM, **kw)
        assert all(torch.equal(bits(a[c:c + 1]), bits(b)) for a, b in zip(full, alone)), c
    for per in (1, 2, 5):
        chunked = exitwave.reconstruct_candidate_stacks(up(st), up(table), LAM, candidates_per_launch=per, **kw)
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(full, chunked)), per
    same = np.broadcast_to(st[1], st.shape).copy()                          # identical stacks: reconstruct_candidates' bits
    a = exitwave.reconstruct_candidate_stacks(up(same), up(table), LAM, **kw)
    b = exitwave.reconstruct_candidates(up(st[1]), up(table), LAM, **kw)
    assert all(torch.equal(bits(p), bits(q)) for p, q in zip(a, b))
    host = exitwave.reconstruct_candidate_stacks(st, table, LAM, px=PX, iterations=3, pad_periods=pad)
    assert isinstance(host, np.ndarray) and np.array_equal(host, full[0].max(1).values.cpu().numpy())


def loop_loss(x, side, kw, pad_val=0.0):
    """The loop a user runs without the batched form: one crop and one reconstruction per set of parameters."""
    return lambda c, d: float(exitwave.reconstruction_loss(exitwave.crop_stack(x, up(c), side, pad_val), up(d), LAM, **kw))


def check_history(got, x, c0, d0, steps, anchor, side, kw, pad_val=0.0):
    """Every loss of the history against the loop at parameters rebuilt from the device's own choices; the result state, the steps
    and the numbers of the result against the replay of those choices.  -> the replay."""
    hl, hc, hs = got.history_losses.cpu().numpy(), got.history_choice.cpu().numpy(), got.history_steps.cpu().numpy()
    rounds, N = len(hc), len(d0)
    replay = RR.compass_search(None, c0, d0, steps, anchor, rounds, choices=hc)
    assert np.array_equal(hs, replay["history_steps"])
    f = loop_loss(x, side, kw, pad_val)
    best = loss0 = f(np.asarray(c0, np.float64), np.asarray(d0, np.float64))
    for r in range(rounds):
        c, d = replay["states"][r]
        for q in range(6 * (N - 1)):
            assert f(*RR.candidate(c, d, hs[r], q, N, anchor)) == hl[r][q], (r, q)
        i = int(np.argmin(hl[r]))                                           # the first of the smallest
        assert hc[r] == (i if hl[r][i] < best else -1), r
        best = min(best, hl[r][i])
    assert float(got.loss0) == loss0 and float(got.loss) == best == min(hl.min(), loss0)
    assert np.array_equal(got.centres.cpu().numpy(), replay["centres"]) and np.array_equal(got.defocuses.cpu().numpy(), replay["defocus"])
    assert got.moves == replay["moves"] == int((hc >= 0).sum()) and got.status == 0
    return replay


def test_refine_params_makes_the_restatements_decisions():
    N, S0, side, it, rounds, steps, seed = SERIES
    ref = series_ref()
    gaps = RR.round_gaps(ref)
    assert min(min(g) for g in gaps) >= MARGIN                              # on the CPU, before the GPU is touched
    assert any(i >= 0 for i in ref["history_choice"]) and -1 in ref["history_choice"]   # a move and a halving
    frames, _, _, c0, d0, anchor = RR.refine_series(N, S0, side, seed)
    x, kw = up(frames), dict(px=PX, iterations=it)
    got = exitwave.refine_params(x, c0, d0, LAM, side, anchor=anchor, step_xy=steps[0], step_defocus=steps[1], rounds=rounds,
                                 return_exit_wave=True, **kw)
    print(f"device choices {got.history_choice.tolist()}, restatement {ref['history_choice']}; loss {float(got.loss)!r} "
          f"(restatement {ref['best']!r}), seed's {float(got.loss0)!r}")
    assert got.history_choice.tolist() == ref["history_choice"]
    assert tuple(got.history_losses.shape) == (rounds, 6 * (N - 1)) and tuple(got.history_steps.shape) == (rounds, 2)
    replay = check_history(got, x, c0, d0, steps, anchor, side, kw)
    assert np.array_equal(replay["centres"], ref["centres"]) and np.array_equal(replay["defocus"], ref["defocus"])
    assert np.array_equal(replay["centres"][anchor], c0[anchor]) and replay["defocus"][anchor] == d0[anchor]
    E = exitwave.reconstruct(exitwave.crop_stack(x, got.centres, side), got.defocuses, LAM, **kw)
    assert torch.equal(bits(got.wave), bits(E))


def test_the_chunking_does_not_change_a_bit():
    N, S0, side = 12, 16, 8
    frames, _, _, c0, d0, anchor = RR.refine_series(N, S0, side, 0)
    x, kw = up(frames), dict(px=PX, iterations=2)
    runs = [exitwave.refine_params(x, c0, d0, LAM, side, step_defocus=4e-9, rounds=2, candidates=cn, return_exit_wave=True, **kw)
            for cn in (64, 7, 1, None)]
    assert tuple(runs[0].history_losses.shape) == (2, 66)
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert a == b if isinstance(a, int) else torch.equal(bits(a), bits(b))
    check_history(runs[0], x, c0, d0, (1.0, 4e-9), anchor, side, kw)


def test_the_composed_path():
    N, S0, side = 3, 32, 8
    frames, _, _, c0, d0, anchor = RR.refine_series(N, S0, side, 0)
    x, kw = up(frames), dict(px=PX, iterations=2, pad_periods=1)
    got = exitwave.refine_params(x, c0, d0, LAM, side, step_defocus=4e-9, rounds=3, candidates=5, pad_val=0.5, return_exit_wave=True, **kw)
    check_history(got, x, c0, d0, (1.0, 4e-9), anchor, side, kw, pad_val=0.5)
    E = exitwave.reconstruct(exitwave.crop_stack(x, got.centres, side, 0.5), got.defocuses, LAM, **kw)
    assert torch.equal(bits(got.wave), bits(E))
    one = exitwave.refine_params(x, c0, d0, LAM, side, step_defocus=4e-9, rounds=3, candidates=1, pad_val=0.5, **kw)
    assert torch.equal(one.history_losses, got.history_losses) and one.wave is None


def test_a_nan_frame_sets_the_status_and_leaves_the_state():
    N, S0, side, it, _, steps, seed = SERIES
    frames, _, _, c0, d0, anchor = RR.refine_series(N, S0, side, seed)
    bad = frames.copy()
    bad[0, S0 // 2, S0 // 2] = np.nan
    got = exitwave.refine_params(up(bad), c0, d0, LAM, side, step_defocus=steps[1], rounds=2, px=PX, iterations=it)
    assert got.status == exitwave.SEARCH_NONFINITE and got.moves == 0 and got.history_choice.tolist() == [-2, -2]
    assert np.array_equal(got.centres.cpu().numpy(), c0) and np.array_equal(got.defocuses.cpu().numpy(), d0)
    assert bool(torch.isnan(got.history_losses).all()) and bool(torch.isnan(got.loss0)) and float(got.loss) == float("inf")
    assert np.array_equal(got.history_steps.cpu().numpy(), [steps, steps])


def test_conventions_and_the_series_in_the_constructors_order():
    N, S0, side, it, _, steps, seed = SERIES
    frames, _, _, c0, d0, anchor = RR.refine_series(N, S0, side, seed)
    kw = dict(px=PX, iterations=it)
    run = lambda im: exitwave.refine_params(im, c0, d0, LAM, side, step_defocus=steps[1], rounds=3, return_exit_wave=True, **kw)
    a, b, n = run(up(frames)), run(up(frames)), run(frames)
    for p, q, r in zip(a, b, n):
        if isinstance(p, int):
            assert p == q == r
        else:
            assert torch.equal(bits(p), bits(q)) and isinstance(r, (float, np.ndarray)) and np.array_equal(p.cpu().numpy(), r)
    assert n.history_choice.dtype == np.int32 and isinstance(n.status, int)
    # anchor and step_defocus by default: N // 2 and 0.1 max|defocuses|
    d = exitwave.refine_params(frames, c0, d0, LAM, side, rounds=1, **kw)
    assert np.array_equal(d.history_steps, [[1.0, 0.1 * np.abs(d0).max()]])
    assert np.array_equal(d.centres[N // 2], c0[N // 2]) and d.defocuses[N // 2] == d0[N // 2]
    # refine_series: align -> refine_params -> crop_stack -> reconstruct
    x, dd = up(frames), up(d0)
    rkw = dict(rounds=2, step_defocus=steps[1])
    wave, ref = exitwave.refine_series(x, dd, LAM, side, refine_kw=rkw, **kw)
    _, centres = exitwave.align(x, side)
    want = exitwave.refine_params(x, centres, dd, LAM, side, **rkw, **kw)
    assert all(p == q if isinstance(p, int) else p is None or torch.equal(bits(p), bits(q)) for p, q in zip(want, ref))
    assert torch.equal(bits(wave), bits(exitwave.reconstruct(exitwave.crop_stack(x, want.centres, side), want.defocuses, LAM, **kw)))
    hw, href = exitwave.refine_series(frames, d0, LAM, side, refine_kw=rkw, **kw)
    assert np.array_equal(hw, wave.cpu().numpy()) and np.array_equal(href.centres, ref.centres.cpu().numpy()) and isinstance(href.loss, float)


@pytest.mark.parametrize("pad", [0, 1])
def test_workspace_of_the_advertised_size_and_guarded_outputs(pad):
    lib, dev = _lib.load(), torch.device("cuda", 0)
    N, S0, side, Cn, R_ = 3, 32, 8, 5, 2
    Q = 6 * (N - 1)
    frames, _, _, c0, d0, anchor = RR.refine_series(N, S0, side, 0)
    x, c, d, st = up(frames), up(c0), up(d0), up(np.array([1.0, 4e-9]))
    nbytes = lib.emd_exitwave_refine_workspace_bytes(Cn, N, side, pad)
    assert nbytes > 0 and nbytes % 8 == 0
    ws, gws = guarded(nbytes // 8, torch.float64, dev, fill=float("nan"), name="workspace")
    outs = {k: guarded(n, torch.float64, dev, name=k) for k, n in (("centres", 2 * N), ("defocus", N), ("result", 2), ("hist_loss", R_ * Q),
                                                                   ("hist_steps", 2 * R_), ("E", 2 * side * side))}
    ints = {k: guarded(n, torch.float32, dev, name=k) for k, n in (("status", 2), ("hist_choice", R_))}
    p = lambda t: t.data_ptr()
    o = lambda k: p((outs.get(k) or ints[k])[0])
    rc = lib.emd_exitwave_refine_f64(p(x), N, S0, side, pad, 0.0, p(c), p(d), p(st), anchor, Cn, R_, LAM, PX, 0.0, 2, 0, o("centres"),
                                     o("defocus"), o("result"), o("status"), o("hist_loss"), o("hist_choice"), o("hist_steps"), o("E"),
                                     p(ws), nbytes, _lib.stream_ptr())
    _lib.check(rc, "refine")
    torch.cuda.synchronize()
    gws()
    for k, (view, g) in {**outs, **ints}.items():
        g()
        assert_written(view, k)
    for k, (view, _) in outs.items():
        assert not torch.isnan(view).any(), k                               # whatever the call reads of the workspace, it wrote
    want = exitwave.refine_params(x, c, d, LAM, side, anchor=anchor, step_xy=st, rounds=R_, candidates=Cn, px=PX, iterations=2,
                                  pad_periods=pad, return_exit_wave=True)
    assert torch.equal(outs["hist_loss"][0].view(R_, Q), want.history_losses) and torch.equal(outs["centres"][0].view(N, 2), want.centres)
    assert torch.equal(outs["defocus"][0], want.defocuses) and torch.equal(outs["result"][0], torch.stack([want.loss, want.loss0]))
    assert torch.equal(outs["E"][0], torch.view_as_real(want.wave).reshape(-1))
    assert ints["status"][0].view(torch.int32).tolist() == [want.status, want.moves]
    assert torch.equal(ints["hist_choice"][0].view(torch.int32), want.history_choice)
    # the candidates' entry points, at exactly their advertised workspace
    st4, table = stacks_of(2, N, side)
    nb = lib.emd_exitwave_candidate_stacks_workspace_bytes(2, N, side, pad)
    ws2, g2 = guarded(nb // 8, torch.float64, dev, fill=float("nan"), name="candidate stacks' workspace")
    lo, gl = guarded(2 * N, torch.float64, dev, name="losses")
    wo, gw = guarded(2, torch.float64, dev, name="worst")
    xs, t = up(st4), up(table)
    _lib.check(lib.emd_exitwave_candidate_stacks_f64(p(xs), 2, N, side, pad, p(t), LAM, PX, 0.0, 2, 0, p(lo), p(wo), None, None, p(ws2), nb,
                                                     _lib.stream_ptr()), "candidate stacks")
    crops, gc = guarded(2 * N * side * side, torch.float32, dev, name="crops")
    ct = up(centres_table(2, N, S0, side))
    _lib.check(lib.emd_crop_candidates_f32(p(x), N, S0, p(ct), 2, side, 0.0, p(crops), _lib.stream_ptr()), "crop candidates")
    torch.cuda.synchronize()
    g2(), gl(), gw(), gc()
    assert_written(lo, "losses"), assert_written(wo, "worst"), assert_written(crops, "crops")
    assert torch.equal(lo.view(2, N), exitwave.reconstruct_candidate_stacks(xs, t, LAM, px=PX, iterations=2, pad_periods=pad, per_image=True))


def test_a_captured_refinement_replays_on_new_frames_seed_and_steps():
    N, S0, side, it, _, steps, seed = SERIES
    f0, _, _, c0, d0, anchor = RR.refine_series(N, S0, side, seed)
    f1, _, _, c1, d1, _ = RR.refine_series(N, S0, side, seed + 1)
    s0, s1 = np.array(steps), np.array([0.5, 2e-9])

    def run(x, c, d, st):
        r = exitwave.refine_params(x, c, d, LAM, side, step_xy=st, rounds=3, candidates=5, return_exit_wave=True, px=PX, iterations=it)
        return [bits(v) for v in (r.centres, r.defocuses, r.loss, r.loss0, r.history_losses, r.history_choice, r.history_steps, r.wave)]

    want0, want1 = run(up(f0), up(c0), up(d0), up(s0)), run(up(f1), up(c1), up(d1), up(s1))
    sx, sc, sd, ss = up(f0), up(c0), up(d0), up(s0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = run(sx, sc, sd, ss)
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs, want0))
    sx.copy_(up(f1)), sc.copy_(up(c1)), sd.copy_(up(d1)), ss.copy_(up(s1))
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs, want1)) and not torch.equal(want0[4], want1[4])
