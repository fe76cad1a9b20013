"""GPU tests of the psi-art fit with per-image sub-pixel shifts (csrc/psiart.hip's SHIFT instances, emdenoise.psiart with ``shifts``;
DESIGN.md 3.31) against the float64 numpy restatement of tests/psiart_shift_ref.py, whose reverse pass tests/test_psiart_shift.py
checks against torch's autograd on the CPU.

Inputs: ``psiart_ref.case(N, S)`` (see tests/test_psiart_gpu.py) with images moved by true shifts seeded in +-0.6 px, evaluated at
shifts off the truth by 0.1 .. 0.2 px to either side, so that every shift is within +-0.8 px (``psiart_shift_ref.case``).  The
conditions of tests/test_psiart_gpu.py (min|b_k| / mean|b_k| >= 0.2, max|chi| <= 400, kappa <= 1e6, every scalar gradient's sum of
|terms| > 0) are asserted on the CPU before the GPU is touched, the last one now for every shift entry too.

No bar comes from the device.  Each is FACTOR = 4 times a yardstick: the largest distance, over this file's cases, between the
restatement as written (numpy.fft, float64) and the same restatement on the radix-2 FFT of tests/fft_ref.py with chi, T, the basis
functions and the shifts' terms in numpy.longdouble; the cases are every evaluation of the tests below: the shifted points, the zero
shifts of the first test and the whole pixels of the third.  ``python -m tests.test_psiart_shift_gpu`` computes them on the CPU; they are
written below.

* Fields (p, dL/dA, dL/dP): relative L2, FIELD_YARD.  Losses: relative, 4 x (field bar) x sqrt(kappa).
* The 27 scalar gradients and the 2 N shift gradients: |error| <= FACTOR x SCALAR_YARD x (the sum of |terms| of that entry).
* Trajectories (20 steps): TRAJ_YARD, ``psiart_shift_ref.state_distance`` between the two restatements' trajectories.
* Recovery: thresholds from the restatement's own run (tests/test_psiart_shift.py), with a factor 10.

Outputs and workspaces lie between the guards of tests/guarded.py.  Every figure is printed before it is asserted."""
import functools

import numpy as np
import pytest
import torch

from emdenoise import _lib, psiart
from tests import psiart_ref as R
from tests import psiart_shift_ref as SR
from tests import test_psiart_gpu as G
from tests.guarded import Workspaces, assert_written, guarded

pytestmark = pytest.mark.gpu

FACTOR = 4.0
FIELD_YARD = 8.987e-15      # python -m tests.test_psiart_shift_gpu: dL/dA of (1, 2048) at zero shifts; 8.266e-15 (dL/dP) at its shifted point
SCALAR_YARD = 3.687e-15     # (3, 8) without normalisation; of the sum of |terms|, the 27 scalars and the 2 N shift entries
TRAJ_YARD = 1.501e-13       # the first moment of the amplitude after 20 steps at (4, 64); shifts within 1.7e-14, their moments 1.6e-15
LAM, SAMPLING, SCALE = R.LAM, R.SAMPLING, R.SCALE
ZERO_CASES = [(3, 8), (4, 64), (2, 256), (2, 512), (2, 1024), (1, 2048)]   # the last four: 1, 2, 4, 8 elements of a line per thread
SMALL_CASES = [(3, 8), (5, 16), (4, 64)]
LARGE_CASES = [(2, 256), (2, 512), (2, 1024), (1, 2048)]
LG_CASES = [(N, S, norm) for N, S in SMALL_CASES for norm in (True, False)] + [(N, S, True) for N, S in LARGE_CASES]
STEP_CASES = [(5, 16), (4, 64)]
WHOLE = np.array([[3.0, -2.0], [-1.0, 5.0], [0.0, 0.0]])
# recovery (asserted on the restatement in tests/test_psiart_shift.py): amplitude, phase, a20 and the shifts trained together
REC = dict(S=32, N=5, truth=40.0, start=38.0, rate_fields=0.01, rate_a20=0.01, rate_shifts=0.02, steps=750, beta1=0.9, epsilon=1e-8)
REC_SHIFT_REF = 2.727e-05   # px: the largest shift error the restatement ends with (measured in tests/test_psiart_shift.py)
REC_SHIFT_MAX = min(10.0 * REC_SHIFT_REF, 0.05)


def field_bar():
    return FACTOR * FIELD_YARD


ids, dev, up, host = G.ids, G.dev, G.up, G.host


@functools.lru_cache(maxsize=None)
def inputs(N, S):
    """Cached: do not write into the result."""
    return SR.case(N, S)


def shifts_of(N, S, which):
    """The shifts a test evaluates at: the case's own ("case"), all 0 ("zero": the first test), whole pixels ("whole": the third)."""
    return {"case": inputs(N, S)["shifts"], "zero": np.zeros((N, 2)), "whole": WHOLE}[which]


@functools.lru_cache(maxsize=None)
def reference(N, S, norm=True, second=False, which="case"):
    c = inputs(N, S)
    kw = dict(fft=R.Radix2FFT, ctf_dtype=np.longdouble) if second else {}
    return SR.loss_and_gradients(c["images"], c["amp"], c["phase"], c["params"], shifts_of(N, S, which), c["ramp"], c["weights"], LAM,
                                 SAMPLING, SCALE, norm, **kw)


def conditions(want, ramp, what):
    G.conditions(want, ramp, what)
    ats = want["abs_terms_shifts"]
    print(f"{what}: smallest sum of |terms| of a shift gradient {ats.min():.3e}")
    assert (ats > 0).all()


def raw_lg(c, shifts, norm=True):
    """emd_psiart_shift_loss_grad_f64 with the workspace at its advertised size, filled with NaN, and every output between guards."""
    N, S = c["images"].shape[0], c["images"].shape[-1]
    lib, d = _lib.load(), dev()
    nbytes = lib.emd_psiart_shift_workspace_bytes(N, S)
    assert nbytes == lib.emd_psiart_workspace_bytes(N, S) + -(-S * N * 2 * 8 // 256) * 256
    ws, ws_g = guarded(nbytes // 8, torch.float64, d, name="workspace")
    sizes = {"losses": N + 1, "pred": N * S * S, "g_amp": S * S, "g_phase": S * S, "g_params": 27, "g_shifts": 2 * N}
    bufs = {n: guarded(s, torch.float64, d, name=n) for n, s in sizes.items()}
    ins = [up(c[k]) for k in ("images", "amp", "phase", "params")] + [up(np.asarray(shifts, np.float64)), up(c["ramp"]), up(c["weights"])]
    p = lambda n: _lib.ptr(bufs[n][0])
    rc = lib.emd_psiart_shift_loss_grad_f64(_lib.ptr(ins[0]), N, S, *[_lib.ptr(t) for t in ins[1:]], LAM, SAMPLING, SCALE, 1 if norm else 0,
                                            p("losses"), p("pred"), p("g_amp"), p("g_phase"), p("g_params"), p("g_shifts"), _lib.ptr(ws),
                                            nbytes, _lib.stream_ptr())
    _lib.check(rc, "emd_psiart_shift_loss_grad_f64")
    torch.cuda.synchronize()
    ws_g()
    for n in sizes:
        bufs[n][1]()
        assert_written(bufs[n][0], n)
    b = {n: v[0].cpu().numpy() for n, v in bufs.items()}
    return {"predictions": b["pred"].reshape(N, S, S), "g_amplitude": b["g_amp"].reshape(S, S), "g_phase": b["g_phase"].reshape(S, S),
            "g_params": b["g_params"], "g_shifts": b["g_shifts"].reshape(N, 2), "losses": b["losses"][:N], "loss": b["losses"][N]}


def check_lg(got, want, what):
    N = want["p"].shape[0]
    for name, g, w in (("p", got["predictions"], want["p"]), ("dL/dA", got["g_amplitude"], want["g_amp"]),
                       ("dL/dP", got["g_phase"], want["g_phase"])):
        e = R.rel_l2(g, w)
        print(f"{what} {name}: rel L2 {e:.3e}; bar {field_bar():.3e}")
        assert e <= field_bar(), (what, name)
    losses = np.append(got["losses"], got["loss"])
    kap = np.append(want["kappa"], want["kappa"].max())
    el = np.abs(losses / want["losses"] - 1.0)
    bars = 4.0 * field_bar() * np.sqrt(kap)
    print(f"{what} losses: largest relative distance {el.max():.3e}; bars {bars.min():.3e} .. {bars.max():.3e}")
    assert (el <= bars).all() and losses.shape == (N + 1,)
    for name, g, w, at in (("scalar", got["g_params"], want["g_params"], want["abs_terms"]),
                           ("shift", got["g_shifts"], want["g_shifts"], want["abs_terms_shifts"])):
        es, bs = np.abs(g - w), FACTOR * SCALAR_YARD * at
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = np.nanmax(np.where(at > 0, es / at, 0.0))
        print(f"{what} {name} gradients: largest |error| / sum|terms| {worst:.3e}; bar {FACTOR * SCALAR_YARD:.3e}; gradients from "
              f"{np.abs(w).min():.2e} to {np.abs(w).max():.2e}")
        assert g.shape == w.shape and (es <= bs).all(), (what, name, np.nonzero(es > bs))


# ---- loss and gradients -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ZERO_CASES, ids=ids)
def test_zero_shifts_give_the_bits_of_the_call_without_shifts(case):
    N, S = case
    c = inputs(N, S)
    plain = host(psiart.loss_and_gradients(up(c["images"]), up(c["amp"]), up(c["phase"]), up(c["params"]), LAM, SAMPLING, ramp=up(c["ramp"]),
                                           weights=up(c["weights"]), offset_scale=SCALE, predictions=True))
    got = raw_lg(c, np.zeros((N, 2)))
    for k in plain:
        assert np.array_equal(got[k], plain[k]), k
    assert sorted(set(got) - set(plain)) == ["g_shifts"] and np.isfinite(got["g_shifts"]).all() and got["g_shifts"].any()


@pytest.mark.parametrize("case", LG_CASES, ids=ids)
def test_loss_and_gradients_with_shifts(case):
    N, S, norm = case
    c = inputs(N, S)
    want = reference(N, S, norm)
    conditions(want, c["ramp"], f"shifted loss_and_gradients {case}")
    assert np.abs(c["shifts"]).max() <= 0.8 and np.abs(c["shifts"] - c["true_shifts"]).min() >= 0.1
    got = raw_lg(c, c["shifts"], norm)
    check_lg(got, want, f"{case}")
    if N == 1:
        assert got["g_params"][R.I_A20] == 0.0                             # the ramp of one image is 0


def test_whole_pixel_shifts_roll_the_predictions():
    N, S = 3, 16
    c = inputs(N, S)
    plain, moved = raw_lg(c, np.zeros((N, 2))), raw_lg(c, WHOLE)
    want = SR.integer_roll(plain["predictions"], WHOLE)
    e = R.rel_l2(moved["predictions"], want)
    wrong = min(R.rel_l2(moved["predictions"], SR.integer_roll(plain["predictions"], alt)) for alt in (-WHOLE, WHOLE[:, ::-1], 0 * WHOLE))
    print(f"whole-pixel shifts {WHOLE.tolist()}: rel L2 from numpy.roll of the predictions without shifts {e:.3e}; bar {field_bar():.3e}; "
          f"the nearest wrong convention (sign, axes, no shift) is {wrong:.3e} away")
    assert e <= field_bar() and wrong > 1e-3


def test_numpy_and_tensor_conventions_with_shifts():
    N, S = 3, 16
    c = inputs(N, S)
    raw = raw_lg(c, c["shifts"])
    out = psiart.loss_and_gradients(c["images"], c["amp"], c["phase"], c["params"], LAM, SAMPLING, ramp=c["ramp"], weights=c["weights"],
                                    offset_scale=SCALE, predictions=True, shifts=c["shifts"])
    t = psiart.loss_and_gradients(up(c["images"]), up(c["amp"]), up(c["phase"]), up(c["params"]), LAM, SAMPLING, ramp=up(c["ramp"]),
                                  weights=up(c["weights"]), offset_scale=SCALE, predictions=True, shifts=up(c["shifts"]))
    assert all(isinstance(v, np.ndarray) for v in out.values()) and out["g_shifts"].shape == (N, 2) and all(v.is_cuda for v in t.values())
    for k in raw:
        assert np.array_equal(out[k], raw[k]) and np.array_equal(t[k].cpu().numpy(), raw[k]), k
    only = psiart.loss_and_gradients(c["images"], c["amp"], c["phase"], c["params"], LAM, SAMPLING, ramp=c["ramp"], weights=c["weights"],
                                     offset_scale=SCALE, gradients=False, shifts=c["shifts"])
    assert sorted(only) == ["loss", "losses"] and np.array_equal(only["losses"], raw["losses"])
    f = psiart.forward(c["amp"], c["phase"], c["params"], c["ramp"], LAM, SAMPLING, SCALE, images=c["images"], shifts=c["shifts"])
    assert np.array_equal(f, raw["predictions"])
    fit = psiart.PsiArtFit(c["images"], LAM, SAMPLING, shifts=True, shift_rate=0.02)
    assert isinstance(fit.shifts, np.ndarray) and fit.shifts.shape == (N, 2) and not fit.shifts.any()
    assert fit._shift_rates.cpu().numpy().tolist() == [0.02, 0.0, 0.02]      # the middle image is the gauge
    fit.step(2)
    s = fit.shifts
    assert fit.steps == 2 and (s[[0, 2]] != 0).all() and not s[1].any()
    assert psiart.PsiArtFit(c["images"], LAM, SAMPLING).shifts is None
    assert psiart.PsiArtFit(c["images"], LAM, SAMPLING, learning_rate=0.5, shifts=c["shifts"])._shift_rates.cpu().numpy().tolist() == [0.5, 0.0, 0.5]


# ---- steps --------------------------------------------------------------------------------------------------------------------------

def shift_rates(N):
    r = 0.01 * (1.0 + 0.1 * np.arange(N))
    r[N // 2] = 0.0
    return r


def make_fit(c, rates, srates, monkeypatch, shifts=None, **kw):
    """A PsiArtFit at the case's point whose workspace, shifts and their moments lie between guards -> (fit, check)."""
    work = Workspaces()
    monkeypatch.setattr(psiart, "_ws", work)
    N = c["images"].shape[0]
    fit = psiart.PsiArtFit(up(c["images"]), LAM, SAMPLING, ramp=up(c["ramp"]), rates=up(rates), offset_scale=SCALE,
                           shifts=c["shifts"] if shifts is None else shifts, **kw)
    fit._amp.copy_(up(c["amp"]))
    fit._phase.copy_(up(c["phase"]))
    fit._params.copy_(up(c["params"]))
    state = [guarded(2 * N, torch.float64, dev(), fill=f, name=n) for n, f in (("shifts", fit._shifts.cpu().numpy()), ("m_shifts", 0.0),
                                                                                 ("v_shifts", 0.0))]
    fit._shifts, fit._shift_moments = state[0][0].view(N, 2), [state[1][0].view(N, 2), state[2][0].view(N, 2)]
    fit.set_weights(up(c["weights"])).set_shift_rates(srates)

    def check():
        torch.cuda.synchronize()
        work.check()
        for _, g in state:
            g()
    return fit, check


def fit_state(fit):
    s = G.fit_state(fit)
    s.update(shifts=fit._shifts.cpu().numpy(), m_shifts=fit._shift_moments[0].cpu().numpy(), v_shifts=fit._shift_moments[1].cpu().numpy())
    return s


@functools.lru_cache(maxsize=None)
def ref_trajectory(N, S, steps, second=False):
    c = inputs(N, S)
    extra = dict(fft=R.Radix2FFT, ctf_dtype=np.longdouble) if second else {}
    f = SR.Fit(c["images"], c["amp"], c["phase"], c["params"], c["shifts"], c["ramp"], c["weights"], G.step_rates(c), shift_rates(N), LAM,
               SAMPLING, SCALE, beta1=0.9, epsilon=1e-8, **extra)
    for _ in range(steps):
        f.step()
    return f.state(), f.scale, f.scale_shifts


@pytest.mark.parametrize("case", STEP_CASES, ids=ids)
def test_twenty_steps_with_shifts(case, monkeypatch):
    N, S = case
    c = inputs(N, S)
    want, scale, scale_shifts = ref_trajectory(N, S, 20)
    sr = shift_rates(N)
    assert (np.delete(sr, N // 2) != 0).all() and sr[N // 2] == 0 and (scale_shifts > 0).all()
    fit, check = make_fit(c, G.step_rates(c), sr, monkeypatch, beta1=0.9, epsilon=1e-8)
    fit.step(20)
    check()
    got = fit_state(fit)
    d = SR.state_distance(got, want, scale, scale_shifts)
    print(f"20 steps with shifts {case}: " + ", ".join(f"{k} {v:.2e}" for k, v in d.items()) + f"; bar {FACTOR * TRAJ_YARD:.3e}")
    assert fit.steps == 20 and max(d.values()) <= FACTOR * TRAJ_YARD
    moved = np.abs(np.delete(want["shifts"] - c["shifts"], N // 2, axis=0))
    print(f"  the shifts moved by {moved.min():.3e} .. {moved.max():.3e} px over the 20 steps")
    assert moved.min() > 1e6 * FACTOR * TRAJ_YARD                         # an update that does nothing fails by far
    assert np.array_equal(got["shifts"][N // 2], c["shifts"][N // 2])


def test_a_shift_rate_of_zero_freezes_that_image(monkeypatch):
    N, S = 5, 16
    c = inputs(N, S)
    sr = shift_rates(N)
    sr[1] = 0.0
    fit, check = make_fit(c, G.step_rates(c), sr, monkeypatch, beta1=0.9, epsilon=1e-8)
    idt, word = torch.int64, 0x7FF8A5C3A5C3A5C3                             # tests/guarded.py's NaN: an entry with rate 0 is not written
    for k in (1, N // 2):
        fit._shift_moments[0][k].view(idt).fill_(word)
        fit._shift_moments[1][k].view(idt).fill_(word)
    fit.step(3)
    check()
    got = fit_state(fit)
    for k in (1, N // 2):
        assert np.array_equal(got["shifts"][k], c["shifts"][k])
        assert bool((fit._shift_moments[0][k].view(idt) == word).all()) and bool((fit._shift_moments[1][k].view(idt) == word).all())
    others = [k for k in range(N) if k not in (1, N // 2)]
    assert (got["shifts"][others] != c["shifts"][others]).all() and (got["m_shifts"][others] != 0).all() and (got["v_shifts"][others] > 0).all()


def test_frozen_zero_shifts_leave_the_trajectory_without_shifts(monkeypatch):
    N, S = 5, 16
    c = inputs(N, S)
    fit, check = make_fit(c, G.step_rates(c), np.zeros(N), monkeypatch, shifts=True, beta1=0.9, epsilon=1e-8)
    fit.step(20)
    check()
    plain = G.make_fit(c, G.step_rates(c), beta1=0.9, epsilon=1e-8).step(20)
    a, b = fit_state(fit), G.fit_state(plain)
    for k in b:
        assert np.array_equal(a[k], b[k]), k
    assert fit.steps == plain.steps == 20 and not a["shifts"].any() and not a["m_shifts"].any() and not a["v_shifts"].any()
    assert not np.array_equal(b["phase"], c["phase"])


def rec_inputs():
    S, N = REC["S"], REC["N"]
    truth = np.zeros(R.NPARAM)
    truth[R.I_A20] = REC["truth"]
    ramp = R.defocus_ramp(N)
    true_shifts = np.random.default_rng(4000).uniform(-0.8, 0.8, (N, 2))
    true_shifts[N // 2] = 0.0
    C, _ = SR.ctf(S, SAMPLING, LAM, truth, ramp, true_shifts, 1.0)
    w = R.true_wave(S)
    images = np.stack([np.abs(np.fft.ifft2(C[k] * np.fft.fft2(w))) ** 2 for k in range(N)]).astype(np.float32)
    rates = np.zeros(R.NPARAM + 2)
    rates[0] = rates[1] = REC["rate_fields"]
    rates[2 + R.I_A20] = REC["rate_a20"]
    srates = np.full(N, REC["rate_shifts"])
    srates[N // 2] = 0.0
    return images, ramp, rates, srates, true_shifts


@functools.lru_cache(maxsize=None)
def rec_reference():
    """The recovery run on the restatement -> (state, the first total loss)."""
    images, ramp, rates, srates, _ = rec_inputs()
    S, N = REC["S"], REC["N"]
    p0 = np.zeros(R.NPARAM)
    p0[R.I_A20] = REC["start"]
    f = SR.Fit(images, np.sqrt(images[N // 2].astype(np.float64)), np.zeros((S, S)), p0, np.zeros((N, 2)), ramp, np.full(N, 1.0 / N), rates,
               srates, LAM, SAMPLING, 1.0, beta1=REC["beta1"], epsilon=REC["epsilon"])
    first = None
    for _ in range(REC["steps"]):
        l = f.step()
        first = l[-1] if first is None else first
    return f.state(), first


def test_recovery_of_the_true_shifts_and_defocus(monkeypatch):
    images, ramp, rates, srates, true_shifts = rec_inputs()
    N = REC["N"]
    work = Workspaces()
    monkeypatch.setattr(psiart, "_ws", work)
    fit = psiart.PsiArtFit(up(images), LAM, SAMPLING, symbols=("a20",), estimates=(REC["start"],), rates=up(rates), beta1=REC["beta1"],
                           epsilon=REC["epsilon"], shifts=True, shift_rate=REC["rate_shifts"])
    assert np.array_equal(fit._shift_rates.cpu().numpy(), srates)           # the default: shift_rate everywhere but the middle
    fit.step(REC["steps"])
    torch.cuda.synchronize()
    work.check()
    got = fit_state(fit)
    err, a20 = np.abs(got["shifts"] - true_shifts).max(), got["params"][R.I_A20]
    print(f"recovery: true shifts up to {np.abs(true_shifts).max():.3f} px from 0, largest error {err:.3e} px after {REC['steps']} steps "
          f"(bar {REC_SHIFT_MAX:.3e}); a20 {REC['start']} -> {a20:.5f} (truth {REC['truth']}, tolerance {G.CONV_A20_TOL}); loss "
          f"{got['losses'][-1]:.3e}")
    assert err <= REC_SHIFT_MAX and abs(a20 - REC["truth"]) <= G.CONV_A20_TOL
    assert not got["shifts"][N // 2].any() and np.abs(true_shifts).max() > 0.5


# ---- house checks -------------------------------------------------------------------------------------------------------------------

def test_guarded_step_with_shifts_and_a_workspace_too_small():
    """emd_psiart_shift_step_f64 itself: the workspace at its advertised size, filled with NaN, and every output between guards."""
    N, S = 2, 512
    c = inputs(N, S)
    lib, d = _lib.load(), dev()
    nbytes = lib.emd_psiart_shift_workspace_bytes(N, S)
    g64 = lambda n, fill=None, name="": guarded(n, torch.float64, d, fill=fill, name=name)
    ws, ws_g = g64(nbytes // 8, name="workspace")
    names = ["amp", "phase", "params", "shifts", "m_amp", "v_amp", "m_phase", "v_phase", "m_params", "v_params", "m_shifts", "v_shifts",
             "losses", "pred", "g_amp", "g_phase", "g_params", "g_shifts"]
    sizes = [S * S, S * S, 27, 2 * N] + [S * S] * 4 + [27, 27, 2 * N, 2 * N, N + 1, N * S * S, S * S, S * S, 27, 2 * N]
    fills = [c["amp"], c["phase"], c["params"], c["shifts"]] + [0.0] * 8 + [None] * 6
    bufs = {n: g64(s, f, n) for n, s, f in zip(names, sizes, fills)}
    step = torch.zeros(1, dtype=torch.int32, device=d)
    x, ramp, w, rates, srates = up(c["images"]), up(c["ramp"]), up(c["weights"]), up(G.step_rates(c)), up(np.full(N, 0.01))
    p = lambda n: _lib.ptr(bufs[n][0])
    call = lambda nb: lib.emd_psiart_shift_step_f64(
        _lib.ptr(x), N, S, p("amp"), p("phase"), p("params"), p("shifts"), _lib.ptr(ramp), _lib.ptr(w), LAM, SAMPLING, SCALE, 1, p("m_amp"),
        p("v_amp"), p("m_phase"), p("v_phase"), p("m_params"), p("v_params"), p("m_shifts"), p("v_shifts"), _lib.ptr(step), _lib.ptr(rates),
        _lib.ptr(srates), 0.9, 0.999, 1e-8, p("losses"), p("pred"), p("g_amp"), p("g_phase"), p("g_params"), p("g_shifts"), _lib.ptr(ws), nb,
        _lib.stream_ptr())
    _lib.check(call(nbytes), "emd_psiart_shift_step_f64")
    torch.cuda.synchronize()
    ws_g()
    for n in names:
        bufs[n][1]()
        assert_written(bufs[n][0], n)
        assert bool(torch.isfinite(bufs[n][0]).all()), n                    # nothing read the workspace's NaN before writing it
    assert int(step) == 1
    b = {n: v[0].cpu().numpy() for n, v in bufs.items()}
    got = {"predictions": b["pred"].reshape(N, S, S), "g_amplitude": b["g_amp"].reshape(S, S), "g_phase": b["g_phase"].reshape(S, S),
           "g_params": b["g_params"], "g_shifts": b["g_shifts"].reshape(N, 2), "losses": b["losses"][:N], "loss": b["losses"][N]}
    check_lg(got, reference(N, S), f"guarded step {(N, S)}")
    assert (b["shifts"].reshape(N, 2) != c["shifts"]).all()
    assert call(nbytes - 256) == -1 and b"workspace too small" in lib.emd_last_error()
    assert call(lib.emd_psiart_workspace_bytes(N, S)) == -1 and b"workspace too small" in lib.emd_last_error()


def test_a_captured_step_with_shifts_replays_with_new_shift_rates(monkeypatch):
    N, S = 5, 16
    c = inputs(N, S)
    srates = up(shift_rates(N))
    fit, check = make_fit(c, G.step_rates(c), srates, monkeypatch, beta1=0.9, epsilon=1e-8)
    assert fit._shift_rates.data_ptr() == srates.data_ptr()                 # adopted where it is
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fit.step()                                                          # warm-up
        with torch.cuda.graph(graph, stream=side):
            fit.step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert fit.steps == 1                                                   # capturing runs nothing
    new_rates = 2.0 * shift_rates(N)[::-1].copy()
    new_rates[0] = 0.0
    fit.set_shift_rates(new_rates)                                          # copied into the tensor that the graph reads
    assert fit._shift_rates.data_ptr() == srates.data_ptr() and np.array_equal(srates.cpu().numpy(), new_rates)
    twin, check2 = make_fit(c, G.step_rates(c), new_rates, monkeypatch, beta1=0.9, epsilon=1e-8)
    for a, b in zip([twin._amp, twin._phase, twin._params, twin._step, twin._shifts] + twin._moments + twin._shift_moments,
                    [fit._amp, fit._phase, fit._params, fit._step, fit._shifts] + fit._moments + fit._shift_moments):
        a.copy_(b)
    before = fit_state(fit)
    with torch.cuda.stream(side):
        for _ in range(3):
            graph.replay()
    torch.cuda.synchronize()
    twin.step(3)
    check()
    check2()
    s1, s2 = fit_state(fit), fit_state(twin)
    assert fit.steps == twin.steps == 4
    for k in s1:
        assert np.array_equal(s1[k], s2[k]), k
    # the replays read the new rates: image 0 is now frozen, the others moved
    assert np.array_equal(s1["shifts"][0], before["shifts"][0]) and (s1["shifts"][[1, 3, 4]] != before["shifts"][[1, 3, 4]]).all()


# ---- the yardsticks (CPU) -----------------------------------------------------------------------------------------------------------

def yardsticks(large=True):
    """-> (field, scalar, trajectory).  ``large=False`` leaves LARGE_CASES out: tests/test_psiart_shift.py recomputes the rest on
    every run and holds the constants above against it."""
    field = scalar = traj = 0.0
    cases = [c + ("case",) for c in LG_CASES] + [(N, S, True, "zero") for N, S in ZERO_CASES] + [(3, 16, True, "whole")]
    for N, S, norm, which in [c for c in cases if large or c[:2] not in LARGE_CASES]:
        case = (N, S, norm, which)
        a, b = reference(N, S, norm, True, which), reference(N, S, norm, False, which)
        e = {k: R.rel_l2(a[k], b[k]) for k in ("C", "p", "g_amp", "g_phase")}
        s = 0.0
        for g, at in (("g_params", "abs_terms"), ("g_shifts", "abs_terms_shifts")):
            with np.errstate(invalid="ignore", divide="ignore"):
                s = max(s, float(np.nanmax(np.where(b[at] > 0, np.abs(a[g] - b[g]) / b[at], 0.0))))
        print(f"yardstick shifted loss_and_gradients {case}: " + ", ".join(f"{k} {v:.3e}" for k, v in e.items()) + f", scalars and shifts "
              f"{s:.3e}; ratio {b['ratio']:.3f}, max|chi| {b['chimax']:.1f}, kappa {b['kappa'].max():.3e}", flush=True)
        field, scalar = max(field, *e.values()), max(scalar, s)
    for N, S in STEP_CASES:
        (a, _, _), (b, scale, scale_shifts) = ref_trajectory(N, S, 20, second=True), ref_trajectory(N, S, 20)
        d = SR.state_distance(a, b, scale, scale_shifts)
        print(f"yardstick 20 steps with shifts {(N, S)}: " + ", ".join(f"{k} {v:.2e}" for k, v in d.items()), flush=True)
        traj = max(traj, *d.values())
    return field, scalar, traj


if __name__ == "__main__":
    print("FIELD_YARD = %.3e\nSCALAR_YARD = %.3e\nTRAJ_YARD = %.3e" % yardsticks())
    st, first = rec_reference()
    ts = rec_inputs()[4]
    print(f"recovery on the restatement: loss {first:.3e} -> {st['losses'][-1]:.3e}, a20 -> {st['params'][R.I_A20]:.5f}, "
          f"REC_SHIFT_REF = {np.abs(st['shifts'] - ts).max():.3e}")
