"""GPU tests of the candidate-batched reconstruction and the defocus search (csrc/exitwave.hip, emdenoise.exitwave).

The contract that makes the candidates checkable: for every candidate c, losses[c], E[c] and stack[c] are BIT FOR BIT what
``reconstruct`` gives for defocus_table[c] alone.  One candidate is compared with the float64 restatement within the bars of
tests/test_exitwave_gpu.py (imported, not copied); everything else is inherited through bit equality.  The searches are compared
with the restatement of tests/exitwave_search_ref.py decision by decision; the margins that make the device's decisions the
restatement's are asserted on the CPU (tests/test_exitwave_search.py's helpers) before the GPU is touched."""
import numpy as np
import pytest
import torch

from emdenoise import _lib, exitwave
from tests import exitwave_ref as R
from tests import exitwave_search_ref as SR
from tests.guarded import assert_written, guarded
from tests.test_exitwave_gpu import CS, KAPPA_MAX, RATIO_MIN, bits, check_wave, ids, loss_bar, up
from tests.test_exitwave_search import (MARGIN, SECTIONS, SWEEP, intensity_series, plateau_gap, plateau_ref, section_gap, section_ref)

pytestmark = pytest.mark.gpu

LAM, PX = R.WAVELENGTH, R.PX
# (N, s, pad, iterations, C, from_intensity, cs)
CASES = [(1, 8, 0, 1, 1, False, 0.0), (3, 16, 0, 5, 4, False, 0.0), (5, 32, 0, 5, 7, False, 0.0), (3, 64, 0, 3, 3, False, 0.0),
         (2, 256, 0, 2, 3, False, 0.0), (2, 512, 0, 2, 2, False, 0.0), (2, 8, 1, 2, 3, False, 0.0), (3, 32, 1, 3, 2, False, 0.0),
         (3, 16, 0, 3, 3, True, 0.0), (3, 32, 0, 3, 3, False, CS)]
KW = dict(px=PX, iterations=5, from_intensity=True)


def table_of(df, C):
    """C different tables around the series' defocuses: scaled, and the odd ones reversed in sign."""
    return np.stack([(0.6 + 0.3 * c) * df * (1.0 if c % 2 == 0 else -1.0) for c in range(C)])


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_every_candidate_equals_reconstruct_bit_for_bit(case):
    N, s, pad, iters, C, fi, cs = case
    images, df = R.series(N, s)
    x, table = up(images), up(table_of(df, C))
    assert len({tuple(r) for r in table.cpu().numpy()}) == C               # a kernel that reads table[0] for every candidate fails
    kw = dict(px=PX, cs=cs, iterations=iters, pad_periods=pad, from_intensity=fi)
    losses, E, stack = exitwave.reconstruct_candidates(x, table, LAM, per_image=True, return_waves=True, return_stack=True, **kw)
    worst = exitwave.reconstruct_candidates(x, table, LAM, **kw)
    assert tuple(losses.shape) == (C, N) and tuple(E.shape) == (C, s, s) and tuple(stack.shape) == (C, N, s, s) and tuple(worst.shape) == (C,)
    for c in range(C):
        e1, s1, l1 = exitwave.reconstruct(x, table[c], LAM, return_stack=True, return_losses=True, **kw)
        assert torch.equal(bits(E[c]), bits(e1)), f"E of candidate {c}"
        assert torch.equal(bits(stack[c]), bits(s1)), f"stack of candidate {c}"
        assert torch.equal(losses[c], l1), f"losses of candidate {c}"
        assert torch.equal(losses[c], exitwave.reconstruction_loss(x, table[c], LAM, per_image=True, **kw))
        assert torch.equal(worst[c], exitwave.reconstruction_loss(x, table[c], LAM, **kw))


def test_one_candidate_against_the_restatement():
    images, df = R.series(3, 32)
    table = table_of(1.5 * df, 3)
    want = R.reconstruct(images, table[2], LAM, PX, 0.0, 5)
    assert want["kappa"].max() <= KAPPA_MAX and want["ratio"] >= RATIO_MIN
    losses, E, stack = exitwave.reconstruct_candidates(images, table, LAM, px=PX, iterations=5, per_image=True, return_waves=True,
                                                       return_stack=True)
    check_wave(E[2], want["E"], "E of candidate 2 of 3")
    check_wave(stack[2], want["stack"], "stack of candidate 2 of 3")
    for k in range(3):
        e = abs(losses[2, k] - want["losses"][k]) / want["losses"][k]
        print(f"  loss[2][{k}] = {losses[2, k]!r} (numpy {want['losses'][k]!r}): relative distance {e:.3e}; bar {loss_bar(want['kappa'][k]):.3e}")
        assert e <= loss_bar(want["kappa"][k])


@pytest.mark.parametrize("pad", [0, 1])
def test_a_candidates_bits_do_not_depend_on_the_others_or_on_the_chunking(pad):
    images, df = R.series(3, 16)
    x, table = up(images), table_of(df, 7)
    kw = dict(px=PX, iterations=3, pad_periods=pad, per_image=True, return_waves=True, return_stack=True)
    full = exitwave.reconstruct_candidates(x, up(table), LAM, **kw)
    perm = np.array([4, 0, 6, 2, 5, 1, 3])
    mixed = exitwave.reconstruct_candidates(x, up(table[perm]), LAM, **kw)
    for a, b in zip(full, mixed):
        assert torch.equal(bits(a[perm]), bits(b))
    for c in (0, 3, 6):
        alone = exitwave.reconstruct_candidates(x, up(table[c:c + 1]), LAM, **kw)
        assert all(torch.equal(bits(a[c:c + 1]), bits(b)) for a, b in zip(full, alone)), c
    for per in (1, 2, 7):
        chunked = exitwave.reconstruct_candidates(x, up(table), LAM, candidates_per_launch=per, **kw)
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(full, chunked)), per


def test_worst_is_the_largest_loss_and_a_nan_image_makes_it_nan():
    images, df = R.series(3, 16)
    table = up(table_of(df, 4))
    losses = exitwave.reconstruct_candidates(up(images), table, LAM, px=PX, iterations=2, per_image=True)
    worst = exitwave.reconstruct_candidates(up(images), table, LAM, px=PX, iterations=2)
    assert torch.equal(worst, losses.max(1).values)
    bad = images.copy()
    bad[1, 3, 4] = np.nan
    w = exitwave.reconstruct_candidates(up(bad), table, LAM, px=PX, iterations=2)
    assert bool(torch.isnan(w).all())


def lossfn(x, ramp):
    return lambda inc: exitwave.reconstruction_loss(x, up(np.float64(inc) * ramp), LAM, **KW)


@pytest.mark.parametrize("i", range(len(SECTIONS)), ids=lambda i: f"C{SECTIONS[i][1]}R{SECTIONS[i][2]}")
def test_section_search_makes_the_restatements_decisions(i):
    (lo, hi), C, rounds = SECTIONS[i]
    ref = section_ref(i)
    gap = section_gap(ref)
    print(f"section {SECTIONS[i]}: restatement argmins {ref['argmins']}, best {ref['increment']!r}, smallest relative gap {gap:.3e}")
    assert gap >= MARGIN                                                    # on the CPU, before the GPU is touched
    images, ramp = intensity_series()
    x = up(images)
    got = exitwave.defocus_search(x, LAM, ramp, bracket=(lo, hi), candidates=C, rounds=rounds, return_wave=True, **KW)
    hi_, hl_ = got.history_increments.cpu().numpy(), got.history_losses.cpu().numpy()
    assert hi_.shape == (rounds, C) and got.status == 0 and got.steps == rounds
    assert [int(np.argmin(l)) for l in hl_] == ref["argmins"]
    bracket = (np.float64(lo), np.float64(hi))
    for r in range(rounds):                                                # the device's own brackets, as bits
        assert np.array_equal(hi_[r], SR.candidate_increments(*bracket, C)), r
        j = int(np.argmin(hl_[r]))
        bracket = (hi_[r][max(j - 1, 0)], hi_[r][min(j + 1, C - 1)])
    f = lossfn(x, ramp)
    for r in range(rounds):
        for c in range(C):
            assert float(f(hi_[r][c])) == hl_[r][c], (r, c)
    flat = int(np.argmin(hl_.ravel()))                                      # the first of the smallest over the whole history
    assert float(got.loss) == hl_.ravel()[flat] and float(got.increment) == hi_.ravel()[flat]
    assert abs(float(got.increment) - ref["increment"]) <= 1e-12 * ref["increment"]
    assert np.array_equal(got.defocuses.cpu().numpy(), float(got.increment) * ramp)
    E = exitwave.reconstruct(x, got.defocuses, LAM, **KW)
    assert torch.equal(bits(got.wave), bits(E))
    if i == 1:
        minima = hl_.min(1)
        assert (np.diff(minima) > 0).any() and float(got.loss) == minima.min()   # the best so far, not the last round's


def test_plateau_search_takes_the_restatements_steps():
    seed, ref = plateau_ref()
    print(f"plateau: restatement seed {seed}, candidates {ref['history_increments']}, smallest relative gap {plateau_gap(seed, ref):.3e}")
    assert plateau_gap(seed, ref) >= MARGIN and ref["steps"] == 4
    images, ramp = intensity_series()
    x = up(images)
    got = exitwave.defocus_search(x, LAM, ramp, method="plateau", sweep_increments=SWEEP, max_steps=8, **KW)
    hi_, hl_ = got.history_increments.cpu().numpy(), got.history_losses.cpu().numpy()
    assert hi_.shape == (8,) and np.array_equal(hi_, ref["history_increments"])   # midpoints of the sweep's increments: exact
    assert got.steps == 4 and got.status == 0 and float(got.increment) == ref["increment"] == hi_[3]
    f = lossfn(x, ramp)
    assert all(float(f(hi_[t])) == hl_[t] for t in range(8)) and float(got.loss) == hl_[3]
    short = exitwave.defocus_search(x, LAM, ramp, method="plateau", sweep_increments=SWEEP, max_steps=2, **KW)
    assert short.status == exitwave.SEARCH_UNFINISHED and short.steps == 2 and float(short.increment) == hi_[1]
    est = exitwave.estimate_defocuses(x, LAM, "quadratic", search_range=(0.0, 4.8e-8), sweep_num=4, max_steps=8, **KW)
    assert est.history_increments.shape == (8,) and tuple(est.defocuses.shape) == (3,)


def test_a_nan_image_sets_the_status_and_leaves_the_bracket():
    images, ramp = intensity_series()
    bad = images.copy()
    bad[0, 0, 0] = np.nan
    got = exitwave.defocus_search(up(bad), LAM, ramp, bracket=(0.3e-8, 1.9e-8), candidates=3, rounds=2, **KW)
    hi_ = got.history_increments.cpu().numpy()
    assert got.status == exitwave.SEARCH_NONFINITE and got.steps == 0 and np.array_equal(hi_[0], hi_[1])
    assert np.array_equal(hi_[0], SR.candidate_increments(0.3e-8, 1.9e-8, 3)) and bool(torch.isnan(got.history_losses).all())
    p = exitwave.defocus_search(up(bad), LAM, ramp, method="plateau", bracket=(0.6e-8, 1.2e-8, 1.0), max_steps=3, **KW)
    assert p.status == exitwave.SEARCH_NONFINITE and p.steps == 0 and float(p.increment) == 1.2e-8


def test_the_same_bits_twice_and_the_conventions():
    images, ramp = intensity_series()
    run = lambda im: exitwave.defocus_search(im, LAM, ramp, bracket=(0.3e-8, 1.9e-8), candidates=4, rounds=2, return_wave=True, **KW)
    a, b, n = run(up(images)), run(up(images)), run(images)
    for p, q, r in zip(a[:5] + a[7:], b[:5] + b[7:], n[:5] + n[7:]):
        assert torch.equal(bits(p), bits(q)) and isinstance(r, (float, np.ndarray)) and np.array_equal(p.cpu().numpy(), r)
    assert a[5:7] == b[5:7] == n[5:7] and isinstance(n.status, int)
    table = table_of(R.series(3, 32)[1], 2)
    t = exitwave.reconstruct_candidates(up(images), up(table), LAM, **KW)
    w = exitwave.reconstruct_candidates(images, table, LAM, **KW)
    assert t.is_cuda and isinstance(w, np.ndarray) and w.dtype == np.float64 and np.array_equal(t.cpu().numpy(), w)
    for seq in (True, False):                                              # the sweep on either route: the same bits
        sw = exitwave.defocus_sweep(images, LAM, SWEEP, ramp, _sequential=seq, **KW)
        assert np.array_equal(sw, exitwave.reconstruct_candidates(images, np.outer(SWEEP, ramp), LAM, **KW))


@pytest.mark.parametrize("pad", [0, 1])
def test_workspace_of_the_advertised_size_and_guarded_outputs(pad):
    lib, dev = _lib.load(), torch.device("cuda", 0)
    N, s, C, R_ = 3, 16, 3, 2
    images, ramp = intensity_series()
    x, r, seed = up(images[:, :s, :s].copy()), up(ramp), up(np.array([0.3e-8, 1.9e-8]))
    nbytes = lib.emd_exitwave_search_workspace_bytes(0, C, N, s, pad)
    assert nbytes % 8 == 0
    ws, gws = guarded(nbytes // 8, torch.float64, dev, fill=float("nan"), name="workspace")
    outs = {k: guarded(n, torch.float64, dev, name=k) for k, n in (("result", 2), ("hist_inc", R_ * C), ("hist_loss", R_ * C), ("E", 2 * s * s))}
    status, gst = guarded(2, torch.float32, dev, name="status")
    p = lambda t: t.data_ptr()
    rc = lib.emd_exitwave_search_f64(p(x), N, s, pad, p(r), p(seed), 0, C, R_, LAM, PX, 0.0, 2, 1, p(outs["result"][0]), p(outs["hist_inc"][0]),
                                     p(outs["hist_loss"][0]), p(status), p(outs["E"][0]), p(ws), nbytes, _lib.stream_ptr())
    _lib.check(rc, "search")
    torch.cuda.synchronize()
    gws(), gst()
    for k, (view, g) in outs.items():
        g()
        assert_written(view, k)
        assert not torch.isnan(view).any(), k                              # whatever the call reads of the workspace, it wrote
    want = exitwave.defocus_search(x, LAM, r, bracket=seed, candidates=C, rounds=R_, px=PX, iterations=2, pad_periods=pad,
                                   from_intensity=True, return_wave=True)
    assert torch.equal(outs["hist_loss"][0].view(R_, C), want.history_losses) and outs["result"][0][0] == want.increment
    assert torch.equal(outs["E"][0], torch.view_as_real(want.wave).reshape(-1)) and status.view(torch.int32).tolist() == [0, R_]


def test_a_captured_search_replays_on_new_images_ramp_and_bracket():
    images, ramp = intensity_series()
    x0, r0, b0 = up(images), up(ramp), up(np.array([0.3e-8, 1.9e-8]))
    x1, r1, b1 = up(images * np.float32(0.75)), up(ramp * 1.25), up(np.array([0.4e-8, 1.5e-8]))

    def run(x, r, b):
        s = exitwave.defocus_search(x, LAM, r, bracket=b, candidates=4, rounds=2, return_wave=True, **KW)
        p = exitwave.defocus_search(x, LAM, r, method="plateau", bracket=torch.cat([b, b[:1] * 0 + 1.0]), max_steps=3, **KW)
        return [bits(v) for v in (s.increment, s.loss, s.history_increments, s.history_losses, s.wave, p.increment, p.history_losses)]

    want0, want1 = run(x0, r0, b0), run(x1, r1, b1)
    sx, sr, sb = x0.clone(), r0.clone(), b0.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = run(sx, sr, sb)
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs, want0))
    sx.copy_(x1), sr.copy_(r1), sb.copy_(b1)
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs, want1)) and not torch.equal(want0[3], want1[3])
