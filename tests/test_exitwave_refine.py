"""CPU tests of the refinement of crop centres and defocuses (emdenoise.exitwave.refine_params, csrc/exitwave.hip):
the compass search of tests/exitwave_refine_ref.py on analytic losses (its rules) and on the series of the GPU tests (the margins the
device's decisions rest on), and the refusals of the C ABI and of Python.  Nothing here touches a GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

from emdenoise import _lib, exitwave
from tests import exitwave_ref as R
from tests import exitwave_refine_ref as RR

LAM, PX = R.WAVELENGTH, R.PX
# A decision of the device equals the restatement's when the losses it compares are further apart than the losses' bar (4e-13, with
# 6.4e-15 measured: DESIGN.md 3.28); MARGIN leaves six orders of magnitude above it.  A condition on the series, not a measurement.
MARGIN = 1e-6
# N, S0, side, iterations, rounds, steps, the series' seed: six rounds that hold moves and a halving
SERIES = (3, 32, 16, 3, 6, (1.0, 4e-9), 4)


@functools.lru_cache(maxsize=None)
def series_ref():
    N, S0, side, it, rounds, steps, seed = SERIES
    frames, _, _, c0, d0, anchor = RR.refine_series(N, S0, side, seed)
    return RR.compass_search(RR.recon_loss(frames, LAM, side, px=PX, iterations=it), c0, d0, steps, anchor, rounds)


def quadratic(target_c, target_d):
    return lambda c, d: float(((c - target_c) ** 2).sum() + ((d - target_d) ** 2).sum())


def test_polls_and_candidates():
    assert RR.polls(3, 1) == [(0, 0), (0, 2), (1, 0), (1, 2), (2, 0), (2, 2)] == exitwave.refine_polls(3, 1)
    assert RR.polls(4, 0)[:3] == [(0, 1), (0, 2), (0, 3)] and len(RR.polls(64, 63)) == 189
    c, d = np.arange(6, dtype=np.float64).reshape(3, 2), np.array([10.0, 20.0, 30.0])
    for q, (what, k, axis, sign) in enumerate([("c", 0, 0, 1), ("c", 0, 0, -1), ("c", 2, 0, 1), ("c", 2, 0, -1), ("c", 0, 1, 1),
                                               ("c", 0, 1, -1), ("c", 2, 1, 1), ("c", 2, 1, -1), ("d", 0, 2, 1), ("d", 0, 2, -1),
                                               ("d", 2, 2, 1), ("d", 2, 2, -1)]):
        cq, dq = RR.candidate(c, d, (0.5, 3.0), q, 3, 1)
        wc, wd = c.copy(), d.copy()
        if what == "c":
            wc[k, axis] += sign * 0.5
        else:
            wd[k] += sign * 3.0
        assert np.array_equal(cq, wc) and np.array_equal(dq, wd), q
    assert np.array_equal(c, np.arange(6).reshape(3, 2))                    # candidate() copies


def test_compass_rules_on_analytic_losses():
    c0, d0 = np.array([[5.0, 5.0], [6.0, 6.0], [7.0, 7.0]]), np.array([1.0, 2.0, 3.0])
    tc, td = c0 + [[1.0, 0.0], [9.0, 9.0], [0.0, -0.75]], d0 + [0.5, 9.0, 0.0]
    r = RR.compass_search(quadratic(tc, td), c0, d0, (1.0, 0.5), 1, 10)
    assert r["status"] == 0 and r["moves"] == sum(i >= 0 for i in r["history_choice"]) and -1 in r["history_choice"]
    assert (np.diff(r["bests"]) <= 0).all() and r["best"] == min(r["history_losses"].min(), r["loss0"])
    assert np.array_equal(r["centres"][1], c0[1]) and r["defocus"][1] == d0[1]   # the anchor keeps its bits
    assert np.array_equal(r["centres"][0], tc[0]) and r["defocus"][0] == td[0] and r["centres"][2, 1] == tc[2, 1]
    ratios = r["history_steps"][1:] / r["history_steps"][:-1]
    assert set(ratios.ravel()) <= {1.0, 0.5} and (ratios[:, 0] == ratios[:, 1]).all()   # the steps only halve, together
    for k, i in enumerate(r["history_choice"]):                             # a move is taken only if strictly better, else halved
        assert (i >= 0) == (r["history_losses"][k].min() < r["bests"][k])
    # a tie between polls: the first wins; a poll that only equals best is no move
    t = RR.compass_search(lambda c, d: float(abs(c[0, 0] - 5.0)), c0, d0, (1.0, 1.0), 1, 1)
    assert t["history_choice"] == [-1] and t["best"] == 0.0 and np.array_equal(t["history_steps"][0], [1.0, 1.0])
    t = RR.compass_search(lambda c, d: float(-abs(c[0, 0] - 5.0) - abs(d[2] - 3.0)), c0, d0, (1.0, 1.0), 1, 1)
    assert t["history_choice"] == [0]
    # NaN among finite polls is skipped; no finite poll: -2, the state stays; a non-finite seed: best = +inf and the status bit
    s = RR.compass_search(lambda c, d: float("nan") if c[0, 0] != 5.0 else float(d[0]), c0, d0, (1.0, 1.0), 1, 1)
    assert s["history_choice"] == [9] and s["status"] == 0
    n = RR.compass_search(lambda c, d: float("nan"), c0, d0, (1.0, 1.0), 1, 2)
    assert n["history_choice"] == [-2, -2] and n["status"] == RR.NONFINITE and np.isinf(n["best"]) and np.isnan(n["loss0"])
    assert np.array_equal(n["centres"], c0) and np.array_equal(n["history_steps"][1], [1.0, 1.0]) and n["moves"] == 0
    # a replay of recorded choices reaches the same state without the loss
    again = RR.compass_search(None, c0, d0, (1.0, 0.5), 1, 10, choices=r["history_choice"])
    assert np.array_equal(again["centres"], r["centres"]) and np.array_equal(again["defocus"], r["defocus"])
    assert np.array_equal(again["history_steps"], r["history_steps"])
    assert RR.NONFINITE == exitwave.SEARCH_NONFINITE


def test_the_series_of_the_gpu_tests_and_its_margins():
    N, S0, side, it, rounds, steps, seed = SERIES
    frames, centres, df, c0, d0, anchor = RR.refine_series(N, S0, side, seed)
    assert frames.shape == (N, S0, S0) and np.abs(c0 - centres).max() <= 1.0 and np.abs(d0 - df).max() <= 4e-9
    assert np.array_equal(c0[anchor], centres[anchor]) and d0[anchor] == df[anchor]
    ref = series_ref()
    gaps = RR.round_gaps(ref)
    at_truth = RR.recon_loss(frames, LAM, side, px=PX, iterations=it)(centres, df)
    print(f"series {SERIES}: choices {ref['history_choice']}, bests {ref['bests']}, gaps (two smallest, smallest and best) "
          f"{[(f'{a:.2e}', f'{b:.2e}') for a, b in gaps]}; loss at the true parameters {at_truth!r}; largest centre distance from the "
          f"truth {np.abs(ref['centres'] - centres).max():.2f} px")
    assert min(min(g) for g in gaps) >= MARGIN                              # the condition of every GPU assertion on decisions
    assert any(i >= 0 for i in ref["history_choice"]) and -1 in ref["history_choice"] and ref["status"] == 0
    assert (np.diff(ref["bests"]) <= 0).all() and ref["best"] < ref["loss0"]
    assert np.array_equal(ref["centres"][anchor], c0[anchor]) and ref["defocus"][anchor] == d0[anchor]
    ratios = ref["history_steps"][1:] / ref["history_steps"][:-1]
    assert set(ratios.ravel()) <= {1.0, 0.5}


def test_c_refusals_need_no_gpu():
    lib = _lib.load()
    ptr = [C.c_void_p(v << 20) for v in range(1, 14)]
    ws, null, big, err = C.c_void_p(1 << 30), C.c_void_p(0), 1 << 28, lib.emd_last_error
    img, c0, d0, st0, oc, od, res, stat, hl, hc, hs, E = ptr[:12]

    def refine(N=3, S0=32, side=16, pad=0, anchor=1, Cn=4, rounds=2, it=1, outs=(oc, od, res, stat, hl, hc, hs, E), wsb=big, seed=(c0, d0, st0)):
        return lib.emd_exitwave_refine_f64(img, N, S0, side, pad, 0.0, *seed, anchor, Cn, rounds, LAM, PX, 0.0, it, 0, *outs, ws, wsb, null)

    q = lib.emd_exitwave_refine_workspace_bytes
    assert q(4, 3, 16, 0) > q(1, 3, 16, 0) > lib.emd_exitwave_candidate_stacks_workspace_bytes(1, 3, 16, 0) > 0
    assert q(4, 3, 16, 0) > lib.emd_exitwave_candidate_stacks_workspace_bytes(4, 3, 16, 0)
    for Cn, N, s in ((4, 3, 16), (1, 1, 8), (64, 64, 32)):
        assert lib.emd_exitwave_candidate_stacks_workspace_bytes(Cn, N, s, 0) == lib.emd_exitwave_candidates_workspace_bytes(Cn, N, s, 0) > 0
    assert q(0, 3, 16, 0) == q(65, 3, 16, 0) == q(4, 1, 16, 0) == q(4, 65, 16, 0) == q(4, 3, 12, 0) == 0
    for kw in (dict(N=1), dict(N=65), dict(S0=0), dict(S0=4097), dict(side=33), dict(side=0), dict(anchor=-1), dict(anchor=3), dict(Cn=0),
               dict(Cn=65), dict(rounds=0), dict(rounds=1025)):
        full = {**dict(N=3, S0=32, side=16, anchor=1, Cn=4, rounds=2), **kw}
        want = (f"got {full['N']} images of side {full['S0']}, side {full['side']}, anchor {full['anchor']}, {full['Cn']} candidates, "
                f"{full['rounds']} rounds")
        assert refine(**kw) == -1 and want.encode() in err(), (kw, err())
    assert refine(side=12) == -1 and b"power of two" in err()
    assert refine(it=0) == -1 and b"iterations" in err()
    assert refine(seed=(c0, null, st0)) == -1 and b"null" in err()
    assert refine(outs=(oc, od, res, null, hl, hc, hs, E)) == -1 and b"null" in err()
    assert refine(wsb=q(4, 3, 16, 0) - 1) == -1 and b"workspace" in err()
    assert refine(outs=(oc, oc, res, stat, hl, hc, hs, E)) == -1 and b"overlap" in err()
    assert refine(seed=(c0, d0, oc)) == -1 and b"overlap" in err()
    assert refine(seed=(C.c_void_p((2 << 20) + 4), d0, st0)) == -3
    crop = lambda N, S0, Cn, side, out=ptr[12]: lib.emd_crop_candidates_f32(img, N, S0, c0, Cn, side, 0.0, out, null)
    for N, S0, Cn, side in ((0, 32, 2, 8), (3, 32, 0, 8), (3, 4097, 2, 8), (3, 32, 2, 33), (3, 32, 2, 0), (256, 32, 256, 8)):
        assert crop(N, S0, Cn, side) == -1 and f"got {Cn} candidates of {N} images of side {S0}, side {side}".encode() in err(), err()
    assert crop(3, 32, 2, 8, out=null) == -1 and b"null" in err()
    assert crop(3, 32, 2, 8, out=img) == -1 and b"overlap" in err()
    stacks = lambda Cn, N, s=16: lib.emd_exitwave_candidate_stacks_f64(img, Cn, N, s, 0, c0, LAM, PX, 0.0, 1, 0, d0, st0, oc, od, ws, big, null)
    for Cn, N in ((0, 3), (65, 3), (3, 0), (3, 65)):
        assert stacks(Cn, N) == -1 and f"got {Cn} candidates of {N} x".encode() in err(), err()
    assert stacks(2, 3, s=12) == -1 and b"power of two" in err()


def test_python_refusals_before_anything_moves():
    r = lambda *shape: np.broadcast_to(np.float32(0), shape)
    c, d = np.full((3, 2), 16.0), np.array([1e-8, 2e-8, 3e-8])
    ok = dict(stack=r(3, 32, 32), centres=c, defocuses=d, wavelength=LAM, side=16)
    for match, kw in (("images", dict(stack=r(1, 32, 32), centres=c[:1], defocuses=d[:1])), ("images", dict(stack=r(65, 32, 32))),
                      ("side", dict(side=33)), ("power of two", dict(side=12)), ("anchor", dict(anchor=3)), ("anchor", dict(anchor=-1)),
                      ("rounds", dict(rounds=0)), ("rounds", dict(rounds=1025)), ("candidates", dict(candidates=0)),
                      ("candidates", dict(candidates=65)), ("centres", dict(centres=c[:2])), ("centres", dict(centres=c * np.nan)),
                      ("defocuses", dict(defocuses=d[:2])), ("defocuses", dict(defocuses=[1e-8, np.inf, 0.0])),
                      ("step_xy", dict(step_xy=0.0)), ("step_defocus", dict(step_defocus=-1e-9)),
                      ("step_defocus", dict(defocuses=np.zeros(3))), ("pad_val", dict(pad_val=np.nan)), ("wavelength", dict(wavelength=0.0)),
                      ("iterations", dict(iterations=0))):
        with pytest.raises(ValueError, match=match):
            exitwave.refine_params(**{**ok, **kw})
    with pytest.raises(TypeError, match="unexpected keyword"):
        exitwave.refine_params(**ok, per_image=True)
    with pytest.raises(ValueError, match="images"):
        exitwave.refine_series(r(1, 32, 32), d[:1], LAM, 16)
    with pytest.raises(ValueError, match="power of two"):
        exitwave.refine_series(r(3, 32, 32), d, LAM, 12)
    with pytest.raises(TypeError, match="refine_kw"):
        exitwave.refine_series(r(3, 32, 32), d, LAM, 16, refine_kw={"steps": 1.0})
    with pytest.raises(ValueError, match="centres table"):
        exitwave.crop_candidates(r(3, 32, 32), np.zeros((2, 4, 2)), 8)
    with pytest.raises(ValueError, match="centres table"):
        exitwave.crop_candidates(r(3, 32, 32), np.zeros((0, 3, 2)), 8)
    with pytest.raises(ValueError, match="side"):
        exitwave.crop_candidates(r(3, 32, 32), np.zeros((2, 3, 2)), 33)
    with pytest.raises(ValueError, match="stacks"):
        exitwave.reconstruct_candidate_stacks(r(3, 16, 16), np.zeros((2, 3)), LAM)
    with pytest.raises(ValueError, match="table"):
        exitwave.reconstruct_candidate_stacks(r(2, 3, 16, 16), np.zeros((3, 3)), LAM)
    with pytest.raises(ValueError, match="power of two"):
        exitwave.reconstruct_candidate_stacks(r(2, 3, 12, 12), np.zeros((2, 3)), LAM)
