"""CPU tests of the defocus search (emdenoise.exitwave, csrc/exitwave.hip): the restatement of
tests/exitwave_search_ref.py on analytic losses (the tie and end rules) and on the intensity series of the GPU tests (the margins the
device's decisions rest on), and the refusals of the C ABI and of Python.  Nothing here touches a GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

from emdenoise import _lib, exitwave
from tests import exitwave_ref as R
from tests import exitwave_search_ref as SR
from tests.test_exitwave_gpu import KAPPA_MAX, loss_bar

LAM, PX = R.WAVELENGTH, R.PX
SECTIONS = [((0.3e-8, 1.9e-8), 6, 5), ((0.6e-8, 2.4e-8), 4, 6)]            # bracket, candidates, rounds
SWEEP = (0.3e-8, 0.6e-8, 1.2e-8, 2.4e-8)
# A decision of the device equals the restatement's when the two smallest losses of the round are further apart than the losses'
# bar; the bar at KAPPA_MAX is 4 x 4 x 5.9e-16 x 1e3 < 1e-11, and MARGIN leaves seven orders of magnitude above it.
MARGIN = 1e-4


@functools.lru_cache(maxsize=None)
def intensity_series():
    """(images, ramp) of test_defocus_sweep_finds_the_true_increment: R.series(3, 32) squared, the true increment 1e-8."""
    images, df = R.series(3, 32)
    return (images.astype(np.float64) ** 2).astype(np.float32), df / 1e-8


def series_loss():
    images, ramp = intensity_series()
    return SR.recon_loss(images, ramp, LAM, px=PX, iterations=5, from_intensity=True)


@functools.lru_cache(maxsize=None)
def section_ref(i):
    (lo, hi), Cn, rounds = SECTIONS[i]
    return SR.section_search(series_loss(), lo, hi, Cn, rounds)


@functools.lru_cache(maxsize=None)
def plateau_ref(max_steps=8):
    f = series_loss()
    seed = SR.plateau_seed(SWEEP, [f(v) for v in SWEEP])
    return seed, SR.plateau_search(f, *seed, max_steps)


def section_gap(ref):
    """The smallest relative distance between the two smallest losses of a round."""
    gaps = []
    for l in ref["history_losses"]:
        a, b = np.sort(l)[:2]
        gaps.append((b - a) / a)
    return min(gaps)


def plateau_gap(seed, ref):
    """The smallest relative distance between a step's loss and the loss it was compared with."""
    prev, gaps = seed[2], []
    for l in ref["history_losses"][:ref["steps"] + 1]:
        gaps.append(abs(l - prev) / prev)
        prev = min(prev, l)
    return min(gaps)


def test_candidate_increments_and_section_rules_on_analytic_losses():
    inc = SR.candidate_increments(0.1, 0.7, 4)
    assert inc[-1] == 0.7 and inc[0] == 0.1 and inc[1] == 0.1 + 1.0 * ((0.7 - 0.1) / 3.0) and len(inc) == 4
    r = SR.section_search(lambda x: (x - 0.3) ** 2, 0.0, 1.0, 5, 6)
    assert abs(r["increment"] - 0.3) < 1e-2 and r["status"] == 0 and r["steps"] == 6
    assert r["loss"] == r["history_losses"].min()                          # the best over all rounds
    for k, i in enumerate(r["argmins"]):
        assert tuple(r["brackets"][k + 1]) == (r["history_increments"][k][max(i - 1, 0)], r["history_increments"][k][min(i + 1, 4)])
    # a tie: the first of the smallest wins the round, and the first seen keeps the best
    t = SR.section_search(lambda x: abs(abs(x) - 1.0), -2.0, 2.0, 5, 1)
    assert t["argmins"] == [1] and t["increment"] == -1.0 and tuple(t["brackets"][1]) == (-2.0, 0.0)
    # the minimum at an end: the bracket is clamped
    e = SR.section_search(lambda x: x, 1.0, 2.0, 3, 2)
    assert e["argmins"] == [0, 0] and tuple(e["brackets"][1]) == (1.0, 1.5) and e["increment"] == 1.0
    # no finite candidate: the bracket stays, status bit 1; a NaN among finite ones is skipped
    n = SR.section_search(lambda x: float("nan"), 1.0, 2.0, 3, 2)
    assert n["status"] == SR.NONFINITE and tuple(n["brackets"][2]) == (1.0, 2.0) and n["steps"] == 0 and np.isnan(n["increment"])
    s = SR.section_search(lambda x: float("nan") if x == 1.0 else x, 1.0, 2.0, 3, 1)
    assert s["argmins"] == [1] and s["status"] == 0


def test_plateau_rules_on_analytic_losses():
    f = lambda x: (x - 1.0) ** 2
    assert SR.plateau_seed([0.0, 0.8, 1.6], [f(0.0), f(0.8), f(1.6)]) == (1.6, 0.8, f(0.8))
    assert SR.plateau_seed([0.0, 1.0, 2.0], [1.0, 0.0, 1.0])[0] == 0.0      # a tie of the neighbours: the left one
    assert SR.plateau_seed([0.0, 1.0], [0.0, 1.0])[:2] == (1.0, 0.0) and SR.plateau_seed([0.0, 1.0], [1.0, 0.0])[:2] == (0.0, 1.0)
    r = SR.plateau_search(f, 1.6, 0.8, f(0.8), 8)
    assert r["history_increments"][0] == 0.5 * (1.6 + 0.8) and r["status"] == 0
    assert r["steps"] < 8 and (r["history_increments"][r["steps"] + 1:] == r["increment"]).all()   # the later steps evaluate incr2
    falling = iter([-1.0, -2.0, -3.0])
    u = SR.plateau_search(lambda x: next(falling), 0.0, 1.0, 0.0, 3)        # every step improves: never done
    assert u["status"] == SR.UNFINISHED and u["steps"] == 3
    n = SR.plateau_search(lambda x: float("nan"), 0.0, 1.0, 5.0, 3)
    assert n["status"] == SR.NONFINITE and n["steps"] == 0 and n["increment"] == 1.0
    assert exitwave.plateau_seed([0.0, 0.8, 1.6], [f(0.0), f(0.8), f(1.6)]) == (1.6, 0.8, f(0.8))
    inc = exitwave.search_increments((1.0, 3.0), 4)
    assert inc.tolist() == [1.0 + 2.0 / 16, 1.0 + 2.0 / 8, 1.0 + 2.0 / 4, 2.0] and (inc > 1.0).all() and (inc < 3.0).all()


def test_the_searches_on_the_restated_intensity_series_and_their_margins():
    images, ramp = intensity_series()
    for inc in (0.3e-8, 1e-8, 2.4e-8):
        assert R.reconstruct(images, inc * ramp, LAM, PX, 0.0, 5, from_intensity=True)["kappa"].max() <= KAPPA_MAX
    assert loss_bar(KAPPA_MAX) * 1e6 < MARGIN
    for i in range(len(SECTIONS)):
        r = section_ref(i)
        print(f"section {SECTIONS[i]}: argmins {r['argmins']}, best {r['increment']!r} loss {r['loss']!r}, round minima "
              f"{r['history_losses'].min(1)}, final bracket {r['brackets'][-1]}, smallest relative gap {section_gap(r):.3e}")
        assert section_gap(r) >= MARGIN and r["status"] == 0
        assert abs(r["increment"] - 1e-8) < 0.1e-8 and r["loss"] == r["history_losses"].min()
    minima = section_ref(1)["history_losses"].min(1)
    assert (np.diff(minima) > 0).any()                                      # a round worse than the one before: best-so-far matters
    seed, p = plateau_ref()
    print(f"plateau from {seed}: candidates {p['history_increments']}, losses {p['history_losses']}, steps {p['steps']}, smallest "
          f"relative gap {plateau_gap(seed, p):.3e}")
    assert p["steps"] == 4 and p["status"] == 0 and plateau_gap(seed, p) >= MARGIN
    assert p["increment"] == p["history_increments"][3] and abs(p["increment"] - 1.0125e-8) < 1e-14
    assert SR.plateau_search(series_loss(), *seed, 2)["status"] == SR.UNFINISHED


def test_c_refusals_need_no_gpu():
    lib = _lib.load()
    a, b, c, d, e, f, g, h = (C.c_void_p(v << 20) for v in range(1, 9))
    ws, null, big, err = C.c_void_p(1 << 30), C.c_void_p(0), 1 << 28, lib.emd_last_error
    cand = lambda Cn, N, s=32, pad=0, it=1: lib.emd_exitwave_candidates_f64(a, Cn, N, s, pad, b, LAM, PX, 0.0, it, 0, c, d, e, f, ws, big, null)
    assert lib.emd_exitwave_candidates_workspace_bytes(4, 3, 32, 0) > lib.emd_exitwave_candidates_workspace_bytes(1, 3, 32, 0) > 0
    assert lib.emd_exitwave_candidates_workspace_bytes(4, 3, 16, 1) == lib.emd_exitwave_candidates_workspace_bytes(1, 3, 16, 1) > 0
    for Cn, N in ((0, 3), (65, 3), (-1, 3), (64, 64 * 16 + 1), (3, 0), (3, 65)):
        assert lib.emd_exitwave_candidates_workspace_bytes(Cn, N, 32, 0) == 0
        assert cand(Cn, N) == -1 and f"got {Cn} candidates of {N} x".encode() in err(), err()
    assert cand(2, 3, s=12) == -1 and b"power of two" in err()
    assert cand(2, 3, it=0) == -1 and b"iterations" in err()
    assert lib.emd_exitwave_candidates_f64(a, 2, 3, 32, 0, b, LAM, PX, 0.0, 1, 0, null, d, e, f, ws, big, null) == -1 and b"null" in err()
    short = lib.emd_exitwave_candidates_workspace_bytes(2, 3, 32, 0) - 1
    assert lib.emd_exitwave_candidates_f64(a, 2, 3, 32, 0, b, LAM, PX, 0.0, 1, 0, c, d, e, f, ws, short, null) == -1 and b"workspace" in err()
    assert lib.emd_exitwave_candidates_f64(a, 2, 3, 32, 0, b, LAM, PX, 0.0, 1, 0, c, c, e, f, ws, big, null) == -1 and b"overlap" in err()
    srch = lambda m, Cn, R_, N=3: lib.emd_exitwave_search_f64(a, N, 32, 0, b, c, m, Cn, R_, LAM, PX, 0.0, 1, 0, d, e, f, g, h, ws, big, null)
    for m, Cn, R_ in ((0, 2, 1), (0, 65, 1), (0, 0, 1), (1, 2, 1), (2, 3, 1), (0, 3, 0), (0, 3, 1025)):
        assert srch(m, Cn, R_) == -1 and f"got method {m}, {Cn} candidates, {R_} rounds".encode() in err(), err()
    assert lib.emd_exitwave_search_workspace_bytes(0, 2, 3, 32, 0) == 0 and lib.emd_exitwave_search_workspace_bytes(1, 2, 3, 32, 0) == 0
    assert lib.emd_exitwave_search_workspace_bytes(0, 3, 3, 32, 0) > lib.emd_exitwave_candidates_workspace_bytes(3, 3, 32, 0)
    assert lib.emd_exitwave_search_workspace_bytes(1, 1, 3, 32, 1) > 0
    assert srch(0, 3, 1, N=65) == -1 and b"bad shape" in err()
    assert lib.emd_exitwave_search_f64(a, 3, 32, 0, null, c, 0, 3, 1, LAM, PX, 0.0, 1, 0, d, e, f, g, h, ws, big, null) == -1 and b"null" in err()
    assert lib.emd_exitwave_search_f64(a, 3, 32, 0, b, c, 0, 3, 1, LAM, PX, 0.0, 1, 0, d, e, f, g, null, ws, 16, null) == -1 and b"workspace" in err()
    text = open(_lib.PKG_DIR + "/../include/emdenoise.h").read()
    for name, v in (("SECTION", exitwave.SEARCH_SECTION), ("PLATEAU", exitwave.SEARCH_PLATEAU), ("NONFINITE", exitwave.SEARCH_NONFINITE),
                    ("UNFINISHED", exitwave.SEARCH_UNFINISHED)):
        assert f"#define EMD_SEARCH_{name} {v}" in text
    assert (SR.NONFINITE, SR.UNFINISHED) == (exitwave.SEARCH_NONFINITE, exitwave.SEARCH_UNFINISHED)


def test_python_refusals_before_anything_moves():
    r = lambda *shape: np.broadcast_to(np.float32(0), shape)
    ramp = [0.0, 1.0, 2.0]
    with pytest.raises(ValueError, match="candidates"):
        exitwave.defocus_search(r(3, 16, 16), LAM, ramp, bracket=(1e-8, 2e-8), candidates=2)
    with pytest.raises(ValueError, match="candidates"):
        exitwave.defocus_search(r(3, 16, 16), LAM, ramp, bracket=(1e-8, 2e-8), candidates=65)
    with pytest.raises(ValueError, match="rounds"):
        exitwave.defocus_search(r(3, 16, 16), LAM, ramp, bracket=(1e-8, 2e-8), rounds=0)
    with pytest.raises(ValueError, match="method"):
        exitwave.defocus_search(r(3, 16, 16), LAM, ramp, bracket=(1e-8, 2e-8), method="golden")
    with pytest.raises(ValueError, match="bracket"):
        exitwave.defocus_search(r(3, 16, 16), LAM, ramp)
    for bad in ((float("nan"), 2e-8), (1e-8, float("inf")), (1e-8,)):
        with pytest.raises(ValueError, match="bracket"):
            exitwave.defocus_search(r(3, 16, 16), LAM, ramp, bracket=bad)
    with pytest.raises(ValueError, match="ramp"):
        exitwave.defocus_search(r(3, 16, 16), LAM, [0.0, 1.0], bracket=(1e-8, 2e-8))
    with pytest.raises(ValueError, match="sweep_increments"):
        exitwave.defocus_search(r(3, 16, 16), LAM, ramp, method="plateau")
    with pytest.raises(ValueError, match="power of two"):
        exitwave.defocus_search(r(3, 12, 12), LAM, ramp, bracket=(1e-8, 2e-8))
    with pytest.raises(TypeError, match="unexpected keyword"):
        exitwave.defocus_search(r(3, 16, 16), LAM, ramp, bracket=(1e-8, 2e-8), per_image=True)
    with pytest.raises(TypeError, match="unexpected keyword"):
        exitwave.estimate_defocuses(r(3, 16, 16), LAM, pixels=2)
    with pytest.raises(ValueError, match="table"):
        exitwave.reconstruct_candidates(r(3, 16, 16), np.zeros((2, 4)), LAM)
    with pytest.raises(ValueError, match="table"):
        exitwave.reconstruct_candidates(r(3, 16, 16), np.zeros((0, 3)), LAM)
    with pytest.raises(ValueError, match="images"):
        exitwave.reconstruct_candidates(r(65, 16, 16), np.zeros((2, 65)), LAM)
    with pytest.raises(ValueError, match="search_increments"):
        exitwave.search_increments((0.0, float("nan")), 4)
