"""CPU tests of the psi-art fit with per-image sub-pixel shifts (emdenoise.psiart with ``shifts``): the restatement of
tests/psiart_shift_ref.py against torch's autograd in complex128 (with the bars of tests/test_psiart.py), whole-pixel shifts against
numpy.roll, zero shifts against tests/psiart_ref.py bit for bit, the refusals of the three new C entry points (argument validation
runs before any launch) and of the Python wrappers, the yardstick constants of the device tests, and the recovery property."""
import ctypes as C

import numpy as np
import pytest
import torch

from emdenoise import _lib, psiart
from tests import psiart_ref as R
from tests import psiart_shift_ref as SR
from tests import test_psiart_gpu as G
from tests import test_psiart_shift_gpu as GS


def autograd(c, normalise):
    """The model composed from torch.fft in complex128 on the CPU, the shift as a phase ramp over numpy.fft.fftfreq:
    (L, dL/dA, dL/dP, dL/dparams, dL/dshifts)."""
    S, N = c["amp"].shape[0], c["images"].shape[0]
    th, phi = [torch.from_numpy(np.array(a)) for a in R.polar_grid(S, R.SAMPLING, R.LAM)]
    f = torch.from_numpy(np.fft.fftfreq(S))
    A, P = torch.tensor(c["amp"], requires_grad=True), torch.tensor(c["phase"], requires_grad=True)
    par, d = torch.tensor(c["params"], requires_grad=True), torch.tensor(c["shifts"], requires_grad=True)
    ph = torch.fft.fft2(torch.complex(A * torch.cos(P), A * torch.sin(P)))
    off = R.SCALE * torch.tanh(par[R.I_OFFSET] / R.SCALE)
    r = torch.from_numpy(R.targets(c["images"]))
    L = 0
    for k in range(N):
        chi = 0
        for n, m, ia, ip in R.TERMS:
            a = par[ia] * c["ramp"][k] + off if ia == R.I_A20 else par[ia]
            chi = chi + a * (torch.cos(m * (phi - par[ip])) if ip is not None else 1.0) * th ** n / n
        chi = chi * 2 * np.pi / R.LAM + 2 * np.pi * (f[:, None] * d[k, 0] + f[None, :] * d[k, 1])
        T = torch.exp(-torch.sign(par[R.I_SPREAD]) * (0.5 * np.pi / R.LAM * par[R.I_SPREAD] * th ** 2) ** 2)
        m_ = torch.fft.ifft2(torch.complex(torch.cos(chi) * T, -torch.sin(chi) * T) * ph).abs()
        cc = r[k].mean() / m_.mean() if normalise else 1.0
        L = L + c["weights"][k] * ((cc * m_ - r[k]) ** 2).mean()
    L.backward()
    return float(L.detach()), A.grad.numpy(), P.grad.numpy(), par.grad.numpy(), d.grad.numpy()


def restatement(c, norm=True, shifts=None, **kw):
    return SR.loss_and_gradients(c["images"], c["amp"], c["phase"], c["params"], c["shifts"] if shifts is None else shifts, c["ramp"],
                                 c["weights"], R.LAM, R.SAMPLING, R.SCALE, norm, **kw)


@pytest.mark.parametrize("case", [(3, 8, True), (3, 8, False), (5, 16, True), (5, 16, False), (4, 32, True), (4, 32, False)], ids=G.ids)
def test_restatement_gradients_against_autograd(case):
    N, S, norm = case
    c = SR.case(N, S)
    want = restatement(c, norm)
    L, gA, gP, gp, gd = autograd(c, norm)
    assert want["ratio"] >= G.RATIO_MIN and want["chimax"] <= G.CHI_MAX and (want["abs_terms"] > 0).all() and (want["abs_terms_shifts"] > 0).all()
    eA, eP = R.rel_l2(want["g_amp"], gA), R.rel_l2(want["g_phase"], gP)
    es, ed = np.abs(want["g_params"] - gp) / want["abs_terms"], np.abs(want["g_shifts"] - gd) / want["abs_terms_shifts"]
    print(f"{case}: L {want['losses'][-1]:.6e} / {L:.6e}; dL/dA {eA:.3e}, dL/dP {eP:.3e} (bar {G.field_bar():.3e}); scalars {es.max():.3e}, "
          f"shifts {ed.max():.3e} of sum|terms| (bar {G.FACTOR * G.SCALAR_YARD:.3e}); shift gradients {np.abs(gd).min():.2e} .. "
          f"{np.abs(gd).max():.2e}")
    assert abs(want["losses"][-1] / L - 1.0) <= 4.0 * G.field_bar() * np.sqrt(want["kappa"].max())
    assert eA <= G.field_bar() and eP <= G.field_bar() and es.max() <= G.FACTOR * G.SCALAR_YARD and ed.max() <= G.FACTOR * G.SCALAR_YARD
    assert want["g_shifts"].shape == (N, 2) and np.abs(gd).min() > 1e3 * G.FACTOR * G.SCALAR_YARD * want["abs_terms_shifts"].max()


def test_whole_pixel_shifts_are_numpy_roll_of_the_predictions():
    N, S = 3, 16
    c = SR.case(N, S)
    plain, moved = restatement(c, shifts=np.zeros((N, 2))), restatement(c, shifts=GS.WHOLE)
    e = R.rel_l2(moved["p"], SR.integer_roll(plain["p"], GS.WHOLE))
    wrong = min(R.rel_l2(moved["p"], SR.integer_roll(plain["p"], alt)) for alt in (-GS.WHOLE, GS.WHOLE[:, ::-1], 0 * GS.WHOLE))
    print(f"whole-pixel shifts: rel L2 from numpy.roll {e:.3e} (bar {G.field_bar():.3e}); the nearest wrong convention {wrong:.3e}")
    assert e <= G.field_bar() and wrong > 1e-3
    assert np.array_equal(moved["losses"][2], plain["losses"][2]) and abs(moved["losses"][0] / plain["losses"][0] - 1.0) > 1e-3


@pytest.mark.parametrize("kw", [{}, dict(fft=R.Radix2FFT, ctf_dtype=np.longdouble)], ids=["as_written", "second"])
def test_zero_shifts_equal_the_restatement_without_shifts_exactly(kw):
    N, S = 4, 32
    c = R.case(N, S)
    for norm in (True, False):
        a = SR.loss_and_gradients(c["images"], c["amp"], c["phase"], c["params"], np.zeros((N, 2)), c["ramp"], c["weights"], R.LAM, R.SAMPLING,
                                  R.SCALE, norm, **kw)
        b = R.loss_and_gradients(c["images"], c["amp"], c["phase"], c["params"], c["ramp"], c["weights"], R.LAM, R.SAMPLING, R.SCALE, norm, **kw)
        for k in b:
            assert np.array_equal(a[k], b[k]), k
        assert sorted(set(a) - set(b)) == ["abs_terms_shifts", "g_shifts"]


def test_the_yardstick_constants_cover_the_restatement():
    """The bars of tests/test_psiart_shift_gpu.py are constants copied from ``python -m tests.test_psiart_shift_gpu``.  Everything but
    the S >= 256 cases is recomputed here, so that they cannot drift from the restatement: no recomputed yardstick may exceed its
    constant (the constants are printed to four digits, hence the 1e-3)."""
    field, scalar, traj = GS.yardsticks(large=False)
    print(f"recomputed without the large cases: field {field:.3e} (constant {GS.FIELD_YARD:.3e}), scalar {scalar:.3e} ({GS.SCALAR_YARD:.3e}), "
          f"trajectory {traj:.3e} ({GS.TRAJ_YARD:.3e})")
    slack = 1.0 + 1e-3
    assert 0 < field <= slack * GS.FIELD_YARD and 0 < scalar <= slack * GS.SCALAR_YARD and 0 < traj <= slack * GS.TRAJ_YARD


def test_recovery_is_a_property_of_the_formulas():
    """Amplitude, phase, a20 (38 -> 40) and the shifts (from 0; true shifts up to 0.8 px, the middle image frozen as the gauge) trained
    together for 750 steps at S = 32, N = 5: the largest shift error the restatement ends with is GS.REC_SHIFT_REF, written there from
    this run; the device's run is held to ten times that and to 0.05 px."""
    want, first = GS.rec_reference()
    ts = GS.rec_inputs()[4]
    err, a20, loss = np.abs(want["shifts"] - ts).max(), want["params"][R.I_A20], want["losses"][-1]
    print(f"recovery on the restatement: loss {first:.3e} -> {loss:.3e}, a20 {GS.REC['start']} -> {a20:.5f}, true shifts up to "
          f"{np.abs(ts).max():.3f} px, largest error {err:.3e} px (constant {GS.REC_SHIFT_REF:.3e})")
    assert err <= GS.REC_SHIFT_REF * (1.0 + 1e-3) and GS.REC_SHIFT_MAX <= 0.05 and 10.0 * abs(a20 - GS.REC["truth"]) <= G.CONV_A20_TOL
    assert np.abs(ts).max() > 0.5 and not ts[GS.REC["N"] // 2].any() and loss < 1e-3 * first


# ---- the refusals of the C entry points (no launch is made) -------------------------------------------------------------------------

BASE, GAP = 1 << 40, 1 << 33


def fake(i, off=0):
    return C.c_void_p(BASE + i * GAP + off)


def call_loss_grad(lib, N=3, S=16, lam=0.025, sampling=0.5, scale=1.0, flags=1, ws_bytes=None, **ptrs):
    names = ["images", "amp", "phase", "params", "shifts", "ramp", "weights", "losses", "pred", "g_amp", "g_phase", "g_params", "g_shifts",
             "workspace"]
    p = {n: fake(i) for i, n in enumerate(names)}
    p.update(ptrs)
    nbytes = lib.emd_psiart_shift_workspace_bytes(N, S) if ws_bytes is None else ws_bytes
    return lib.emd_psiart_shift_loss_grad_f64(p["images"], N, S, p["amp"], p["phase"], p["params"], p["shifts"], p["ramp"], p["weights"], lam,
                                              sampling, scale, flags, p["losses"], p["pred"], p["g_amp"], p["g_phase"], p["g_params"],
                                              p["g_shifts"], p["workspace"], nbytes, None)


def call_step(lib, N=3, S=16, lam=0.025, sampling=0.5, scale=1.0, flags=1, betas=(0.99, 0.999, 0.1), ws_bytes=None, **ptrs):
    names = ["images", "amp", "phase", "params", "shifts", "ramp", "weights", "m_amp", "v_amp", "m_phase", "v_phase", "m_params", "v_params",
             "m_shifts", "v_shifts", "step", "rates", "shift_rates", "losses", "pred", "g_amp", "g_phase", "g_params", "g_shifts", "workspace"]
    p = {n: fake(i) for i, n in enumerate(names)}
    p.update(ptrs)
    nbytes = lib.emd_psiart_shift_workspace_bytes(N, S) if ws_bytes is None else ws_bytes
    return lib.emd_psiart_shift_step_f64(p["images"], N, S, p["amp"], p["phase"], p["params"], p["shifts"], p["ramp"], p["weights"], lam,
                                         sampling, scale, flags, p["m_amp"], p["v_amp"], p["m_phase"], p["v_phase"], p["m_params"],
                                         p["v_params"], p["m_shifts"], p["v_shifts"], p["step"], p["rates"], p["shift_rates"], betas[0],
                                         betas[1], betas[2], p["losses"], p["pred"], p["g_amp"], p["g_phase"], p["g_params"], p["g_shifts"],
                                         p["workspace"], nbytes, None)


@pytest.mark.parametrize("call", [call_loss_grad, call_step], ids=["loss_grad", "step"])
def test_refusals_of_the_entry_points_with_shifts(call):
    lib = _lib.load()
    err = lambda: lib.emd_last_error()
    null = C.c_void_p(0)
    for kw in (dict(S=12), dict(S=4), dict(S=4096), dict(N=0), dict(N=65)):
        assert call(lib, ws_bytes=1 << 30, **kw) == -1 and b"bad shape" in err() and b"psiart_shift" in err(), kw
    assert call(lib, S=4096, ws_bytes=1 << 30) == -1 and b"4096 is refused" in err()
    for kw in (dict(lam=0.0), dict(lam=-1.0), dict(sampling=0.0), dict(scale=0.0), dict(scale=float("nan"))):
        assert call(lib, **kw) == -1 and b"must be positive" in err(), kw
    assert call(lib, flags=4) == -1 and b"unknown flag" in err()
    for name in ("images", "amp", "phase", "params", "shifts", "ramp", "weights", "losses", "workspace"):
        assert call(lib, **{name: null}) == -1 and b"null pointer" in err(), name
    assert call(lib, ws_bytes=lib.emd_psiart_shift_workspace_bytes(3, 16) - 1) == -1 and b"workspace too small" in err()
    assert call(lib, ws_bytes=lib.emd_psiart_workspace_bytes(3, 16)) == -1 and b"workspace too small" in err()   # the layout without shifts
    for name, off in (("workspace", 8), ("amp", 4), ("params", 4), ("shifts", 4), ("g_shifts", 4), ("losses", 4), ("weights", 12), ("images", 2)):
        assert call(lib, **{name: fake(30, off)}) == -3 and b"aligned" in err(), name
    assert call(lib, g_shifts=fake(1)) == -1 and b"overlap" in err()        # an output on an input
    assert call(lib, g_shifts=fake(13 if call is call_loss_grad else 24, 256)) == -1 and b"overlap" in err()   # inside the workspace
    assert call(lib, g_shifts=fake(7 if call is call_loss_grad else 18, 8)) == -1 and b"overlap" in err()      # on the losses
    if call is call_step:
        for name in ("m_shifts", "v_shifts", "shift_rates", "m_amp", "step", "rates"):
            assert call(lib, **{name: null}) == -1 and b"null pointer" in err(), name
        assert call(lib, shift_rates=fake(30, 4)) == -3 and call(lib, m_shifts=fake(30, 4)) == -3
        assert call(lib, m_shifts=fake(4)) == -1 and b"overlap" in err()    # a moment on the shifts
        for betas in ((1.0, 0.999, 0.1), (0.9, -0.1, 0.1), (0.9, 0.999, 0.0)):
            assert call(lib, betas=betas) == -1 and b"epsilon" in err(), betas


def test_the_workspace_size_with_shifts():
    lib = _lib.load()
    for bad in ((0, 16), (3, 12), (3, 4096), (65, 16)):
        assert lib.emd_psiart_shift_workspace_bytes(*bad) == 0
    for N, S in ((3, 16), (5, 8), (64, 2048)):
        assert lib.emd_psiart_shift_workspace_bytes(N, S) == lib.emd_psiart_workspace_bytes(N, S) + -(-S * N * 2 * 8 // 256) * 256


def test_python_value_errors_come_before_anything_moves():
    img = np.ones((3, 16, 16), np.float32)
    A = np.ones((16, 16))
    for bad in (np.zeros((2, 2)), np.zeros((3, 3)), np.zeros(6), np.full((3, 2), np.nan)):
        with pytest.raises(ValueError, match="shifts"):
            psiart.loss_and_gradients(img, A, A, np.zeros(27), 0.025, 0.5, shifts=bad)
        with pytest.raises(ValueError, match="shifts"):
            psiart.PsiArtFit(img, 0.025, 0.5, shifts=bad)
    with pytest.raises(ValueError, match="shifts"):
        psiart.forward(A, A, np.zeros(27), [0.0, 1.0], 0.025, 0.5, shifts=np.zeros((3, 2)))
    with pytest.raises(ValueError, match="shift_rate"):
        psiart.PsiArtFit(img, 0.025, 0.5, shift_rate=0.01)
    for rate in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="shift_rate"):
            psiart.PsiArtFit(img, 0.025, 0.5, shifts=True, shift_rate=rate)
