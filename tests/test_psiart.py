"""CPU tests of the gradient-descent exit-wave and aberration fit (emdenoise.psiart): the restatement's hand-written
reverse pass against torch's autograd in complex128, the host helpers against the reference's expressions, the refusals of the C entry
points (argument validation runs before any launch) and of the Python wrappers, and the convergence property of the formulas."""
import ctypes as C

import numpy as np
import pytest
import torch

from emdenoise import _lib, psiart
from tests import psiart_ref as R
from tests import test_psiart_gpu as G


def autograd(c, normalise, amplitudes=False):
    """The model composed from torch.fft in complex128 on the CPU: (L, dL/dA, dL/dP, dL/dparams)."""
    S, N = c["amp"].shape[0], c["images"].shape[0]
    th, phi = [torch.from_numpy(np.array(a)) for a in R.polar_grid(S, R.SAMPLING, R.LAM)]
    A, P = torch.tensor(c["amp"], requires_grad=True), torch.tensor(c["phase"], requires_grad=True)
    par = torch.tensor(c["params"], requires_grad=True)
    ph = torch.fft.fft2(torch.complex(A * torch.cos(P), A * torch.sin(P)))
    off = R.SCALE * torch.tanh(par[R.I_OFFSET] / R.SCALE)
    r = torch.from_numpy(R.targets(c["images"], amplitudes))
    L = 0
    for k in range(N):
        chi = 0
        for n, m, ia, ip in R.TERMS:                                       # get_chi, term by term
            a = par[ia] * c["ramp"][k] + off if ia == R.I_A20 else par[ia]
            chi = chi + a * (torch.cos(m * (phi - par[ip])) if ip is not None else 1.0) * th ** n / n
        chi = chi * 2 * np.pi / R.LAM
        T = torch.exp(-torch.sign(par[R.I_SPREAD]) * (0.5 * np.pi / R.LAM * par[R.I_SPREAD] * th ** 2) ** 2)
        m_ = torch.fft.ifft2(torch.complex(torch.cos(chi) * T, -torch.sin(chi) * T) * ph).abs()
        cc = r[k].mean() / m_.mean() if normalise else 1.0
        L = L + c["weights"][k] * ((cc * m_ - r[k]) ** 2).mean()
    L.backward()
    return float(L.detach()), A.grad.numpy(), P.grad.numpy(), par.grad.numpy()


@pytest.mark.parametrize("case", [(3, 8, True), (3, 8, False), (5, 16, True), (5, 16, False), (4, 32, True), (4, 32, False)], ids=G.ids)
def test_restatement_gradients_against_autograd(case):
    N, S, norm = case
    c = R.case(N, S)
    want = R.loss_and_gradients(c["images"], c["amp"], c["phase"], c["params"], c["ramp"], c["weights"], R.LAM, R.SAMPLING, R.SCALE, norm)
    L, gA, gP, gp = autograd(c, norm)
    assert want["ratio"] >= G.RATIO_MIN and want["chimax"] <= G.CHI_MAX and (want["abs_terms"] > 0).all() and (c["params"] != 0).all()
    eA, eP = R.rel_l2(want["g_amp"], gA), R.rel_l2(want["g_phase"], gP)
    es = np.abs(want["g_params"] - gp) / want["abs_terms"]
    print(f"{case}: L {want['losses'][-1]:.6e} / {L:.6e}; dL/dA {eA:.3e}, dL/dP {eP:.3e} (bar {G.field_bar():.3e}); scalars "
          f"{es.max():.3e} of sum|terms| (bar {G.FACTOR * G.SCALAR_YARD:.3e}); gradients {np.abs(gp).min():.2e} .. {np.abs(gp).max():.2e}")
    assert abs(want["losses"][-1] / L - 1.0) <= 4.0 * G.field_bar() * np.sqrt(want["kappa"].max())
    assert eA <= G.field_bar() and eP <= G.field_bar() and es.max() <= G.FACTOR * G.SCALAR_YARD


def test_amplitude_targets_against_autograd():
    c = dict(R.case(3, 16))
    c["images"] = -np.sqrt(c["images"].astype(np.float64)).astype(np.float32)
    want = R.loss_and_gradients(c["images"], c["amp"], c["phase"], c["params"], c["ramp"], c["weights"], R.LAM, R.SAMPLING, R.SCALE, True, True)
    L, gA, gP, gp = autograd(c, True, True)
    eA, eP = R.rel_l2(want["g_amp"], gA), R.rel_l2(want["g_phase"], gP)
    es = np.abs(want["g_params"] - gp) / want["abs_terms"]
    print(f"amplitude targets: L {want['losses'][-1]:.6e} / {L:.6e}; dL/dA {eA:.3e}, dL/dP {eP:.3e} (bar {G.field_bar():.3e}); scalars "
          f"{es.max():.3e} of sum|terms| (bar {G.FACTOR * G.SCALAR_YARD:.3e})")
    assert abs(want["losses"][-1] / L - 1.0) <= 4.0 * G.field_bar() * np.sqrt(want["kappa"].max())
    assert eA <= G.field_bar() and eP <= G.field_bar() and es.max() <= G.FACTOR * G.SCALAR_YARD


def test_focal_spread_zero_gives_an_envelope_of_exactly_one():
    """T = exp(-sign(D) x^2) at D = 0 is exp(-0) = 1 exactly, in both evaluations of the restatement, so C has unit modulus to rounding
    (the bar the device test uses) and dL/dD, whose every term carries |D|, is exactly 0."""
    N, S = 3, 16
    c, _ = G.inputs(N, S, "nospread")
    assert c["params"][R.I_SPREAD] == 0.0
    for dtype in (np.float64, np.longdouble):
        assert (R.ctf_parts(S, R.SAMPLING, R.LAM, c["params"], dtype)["T"] == 1.0).all()
        C, _ = R.ctf(S, R.SAMPLING, R.LAM, c["params"], c["ramp"], R.SCALE, dtype)
        assert (np.abs(np.abs(C) - 1.0) <= G.UNIT_MODULUS_BAR).all()
    want = G.reference(N, S, True, "nospread")
    assert want["g_params"][R.I_SPREAD] == 0.0 and want["abs_terms"][R.I_SPREAD] == 0.0
    spread, _ = R.ctf(S, R.SAMPLING, R.LAM, G.inputs(N, S)[0]["params"], c["ramp"], R.SCALE)
    assert np.abs(spread).min() < 0.999


def test_the_yardstick_constants_cover_the_restatement():
    """The bars of tests/test_psiart_gpu.py are constants copied from ``python -m tests.test_psiart_gpu``.  Everything but the S >= 256
    cases and the 400-step convergence run on the radix-2 transform (12 s) is recomputed here, so that they cannot drift from the
    restatement: no recomputed yardstick may exceed its constant (the constants are printed to four digits, hence the 1e-3), and the
    two that are attained on these cases (the scalars at the (3, 16) amplitude-target case, the trajectory at (4, 64)) may not have
    fallen to less than half of it either."""
    field, scalar, traj, _ = G.yardsticks(large=False, conv=False)
    print(f"recomputed without the large cases: field {field:.3e} (constant {G.FIELD_YARD:.3e}), scalar {scalar:.3e} ({G.SCALAR_YARD:.3e}), "
          f"trajectory {traj:.3e} ({G.TRAJ_YARD:.3e})")
    slack = 1.0 + 1e-3
    assert field <= slack * G.FIELD_YARD
    for got, const in ((scalar, G.SCALAR_YARD), (traj, G.TRAJ_YARD)):
        assert 0.5 * const <= got <= slack * const


def test_host_helpers_against_the_reference_expressions():
    assert abs(psiart.energy2wavelength(200) - 0.025079340) < 1e-9 and psiart.energy2wavelength(200) == R.energy2wavelength(200)
    for n, middle in [(1, 0), (5, 2), (9, 8), (17, 8), (6, 0)]:
        want = [np.abs(i) * 3 for i in range(-middle, n - middle)]        # psi-art.py:293-294
        assert np.array_equal(psiart.defocus_ramp(n, middle), np.array(want, np.float64))
    assert np.array_equal(psiart.defocus_ramp(5), [6.0, 3.0, 0.0, 3.0, 6.0])
    for n, middle in [(17, 8), (9, 4), (9, 0), (9, 8), (5, 1)]:
        for boot_size in range(0, n):                                      # psi-art.py:334-348
            lb = middle - boot_size // 2 - boot_size % 2
            ub = middle + boot_size // 2
            if lb < 0:
                ub += np.absolute(lb)
                lb = 0
            if ub >= n:
                lb -= ub - (n - 1)
                ub = n - 1
            want = np.array([1.0 / (boot_size + 1) if i in list(range(n))[lb:ub] else 0.0 for i in range(n)])
            assert np.array_equal(psiart.boot_weights(n, middle, boot_size), want), (n, middle, boot_size)
    assert np.array_equal(psiart.boot_weights(9, 4, 3), [0, 0, 0.25, 0.25, 0.25, 0, 0, 0, 0])
    assert psiart.SYMBOLS == R.SYMBOLS and len(psiart.SYMBOLS) == 25 and psiart.NPARAM == 27
    th, phi = psiart.polar_grid(16, 0.5, R.LAM)
    f = np.fft.fftfreq(16, 0.5)
    assert th[0, 0] == 0 and phi[0, 0] == 0 and th[3, 0] == R.LAM * abs(f[3]) and phi[0, 2] == np.pi / 2 and phi[9, 0] == np.pi
    assert np.array_equal(th, R.polar_grid(16, 0.5, R.LAM)[0]) and np.array_equal(phi, R.polar_grid(16, 0.5, R.LAM)[1])


# ---- the refusals of the C entry points (no launch is made) -------------------------------------------------------------------------

BASE, GAP = 1 << 40, 1 << 33


def fake(i, off=0):
    return C.c_void_p(BASE + i * GAP + off)


def call_loss_grad(lib, N=3, S=16, lam=0.025, sampling=0.5, scale=1.0, flags=1, ws_bytes=None, **ptrs):
    names = ["images", "amp", "phase", "params", "ramp", "weights", "losses", "pred", "g_amp", "g_phase", "g_params", "workspace"]
    p = {n: fake(i) for i, n in enumerate(names)}
    p.update(ptrs)
    nbytes = lib.emd_psiart_workspace_bytes(N, S) if ws_bytes is None else ws_bytes
    return lib.emd_psiart_loss_grad_f64(p["images"], N, S, p["amp"], p["phase"], p["params"], p["ramp"], p["weights"], lam, sampling, scale,
                                        flags, p["losses"], p["pred"], p["g_amp"], p["g_phase"], p["g_params"], p["workspace"], nbytes, None)


def call_step(lib, N=3, S=16, lam=0.025, sampling=0.5, scale=1.0, flags=1, betas=(0.99, 0.999, 0.1), ws_bytes=None, **ptrs):
    names = ["images", "amp", "phase", "params", "ramp", "weights", "m_amp", "v_amp", "m_phase", "v_phase", "m_params", "v_params", "step",
             "rates", "losses", "pred", "g_amp", "g_phase", "g_params", "workspace"]
    p = {n: fake(i) for i, n in enumerate(names)}
    p.update(ptrs)
    nbytes = lib.emd_psiart_workspace_bytes(N, S) if ws_bytes is None else ws_bytes
    return lib.emd_psiart_step_f64(p["images"], N, S, p["amp"], p["phase"], p["params"], p["ramp"], p["weights"], lam, sampling, scale, flags,
                                   p["m_amp"], p["v_amp"], p["m_phase"], p["v_phase"], p["m_params"], p["v_params"], p["step"], p["rates"],
                                   betas[0], betas[1], betas[2], p["losses"], p["pred"], p["g_amp"], p["g_phase"], p["g_params"],
                                   p["workspace"], nbytes, None)


@pytest.mark.parametrize("call", [call_loss_grad, call_step], ids=["loss_grad", "step"])
def test_refusals_of_the_entry_points(call):
    lib = _lib.load()
    err = lambda: lib.emd_last_error()
    null = C.c_void_p(0)
    for kw in (dict(S=12), dict(S=4), dict(S=4096), dict(N=0), dict(N=65)):
        assert call(lib, ws_bytes=1 << 30, **kw) == -1 and b"bad shape" in err(), kw
    assert call(lib, S=4096, ws_bytes=1 << 30) == -1 and b"4096 is refused" in err()
    for kw in (dict(lam=0.0), dict(lam=-1.0), dict(sampling=0.0), dict(scale=0.0), dict(scale=float("nan"))):
        assert call(lib, **kw) == -1 and b"must be positive" in err(), kw
    assert call(lib, flags=4) == -1 and b"unknown flag" in err()
    for name in ("images", "amp", "phase", "params", "ramp", "weights", "losses", "workspace"):
        assert call(lib, **{name: null}) == -1 and b"null pointer" in err(), name
    assert call(lib, ws_bytes=lib.emd_psiart_workspace_bytes(3, 16) - 1) == -1 and b"workspace too small" in err()
    for name, off in (("workspace", 8), ("amp", 4), ("params", 4), ("losses", 4), ("g_amp", 4), ("weights", 12), ("images", 2)):
        assert call(lib, **{name: fake(30, off)}) == -3 and b"aligned" in err(), name
    assert call(lib, g_amp=fake(1)) == -1 and b"overlap" in err()           # an output on an input
    assert call(lib, pred=fake(11 if call is call_loss_grad else 19, 256)) == -1 and b"overlap" in err()   # an output inside the workspace
    assert call(lib, losses=fake(8, 8)) == -1 and b"overlap" in err()       # two outputs
    if call is call_step:
        for name in ("m_amp", "v_phase", "m_params", "step", "rates"):
            assert call(lib, **{name: null}) == -1 and b"null pointer" in err(), name
        assert call(lib, step=fake(30, 2)) == -3 and call(lib, rates=fake(30, 4)) == -3
        assert call(lib, m_amp=fake(1)) == -1 and b"overlap" in err()
        for betas in ((1.0, 0.999, 0.1), (0.9, -0.1, 0.1), (0.9, 0.999, 0.0)):
            assert call(lib, betas=betas) == -1 and b"epsilon" in err(), betas


def test_refusals_of_ctf_and_the_workspace_size():
    lib = _lib.load()
    assert lib.emd_psiart_workspace_bytes(0, 16) == 0 and lib.emd_psiart_workspace_bytes(3, 12) == 0
    assert lib.emd_psiart_workspace_bytes(3, 4096) == 0 and lib.emd_psiart_workspace_bytes(65, 16) == 0
    assert lib.emd_psiart_workspace_bytes(64, 2048) > 2 * 64 * 2048 * 2048 * 16 and lib.emd_psiart_workspace_bytes(3, 16) % 256 == 0
    f = lambda S=16, n=2, par=fake(0), ramp=fake(1), lam=0.025, sampling=0.5, scale=1.0, out=fake(2): \
        lib.emd_psiart_ctf_f64(S, n, par, ramp, lam, sampling, scale, out, None)
    assert f(S=24) == -1 and b"bad shape" in lib.emd_last_error()
    assert f(n=-1) == -1 and f(n=70000) == -1 and b"65535" in lib.emd_last_error()
    assert f(n=0) == 0
    assert f(lam=0.0) == -1 and f(sampling=-2.0) == -1 and f(scale=0.0) == -1 and b"must be positive" in lib.emd_last_error()
    assert f(par=C.c_void_p(0)) == -1 and b"null pointer" in lib.emd_last_error()
    assert f(out=fake(2, 8)) == -3 and f(ramp=fake(1, 4)) == -3 and b"aligned" in lib.emd_last_error()
    assert f(out=fake(0)) == -1 and b"overlap" in lib.emd_last_error()


def test_python_value_errors_come_before_anything_moves():
    img = np.ones((3, 16, 16), np.float32)
    A = np.ones((16, 16))
    with pytest.raises(ValueError, match="power of two"):
        psiart.PsiArtFit(np.ones((3, 12, 12), np.float32), 0.025, 0.5)
    with pytest.raises(ValueError, match="power of two"):
        psiart.PsiArtFit(np.ones((1, 4096, 4096), np.float32), 0.025, 0.5)
    with pytest.raises(ValueError, match=r"\[N,S,S\]"):
        psiart.PsiArtFit(np.ones((16, 16), np.float32), 0.025, 0.5)
    with pytest.raises(ValueError, match="1..64 images"):
        psiart.PsiArtFit(np.ones((65, 8, 8), np.float32), 0.025, 0.5)
    with pytest.raises(ValueError, match="real"):
        psiart.PsiArtFit(img.astype(np.complex64), 0.025, 0.5)
    for kw in (dict(wavelength=0.0), dict(sampling=-1.0)):
        with pytest.raises(ValueError, match="positive"):
            psiart.PsiArtFit(img, **{"wavelength": 0.025, "sampling": 0.5, **kw})
    for kw in (dict(offset_scale=0.0), dict(epsilon=0.0), dict(beta1=1.0), dict(learning_rate=-1.0), dict(symbols=("a20", "b7"), estimates=(1, 2)),
               dict(symbols=("a20",), estimates=(1.0, 2.0)), dict(middle=3), dict(rates={"a21": 1.0}), dict(rates=np.ones(28)),
               dict(rates=-np.ones(29)), dict(ramp=[0.0, 1.0])):
        with pytest.raises(ValueError):
            psiart.PsiArtFit(img, 0.025, 0.5, **kw)
    with pytest.raises(ValueError, match=r"amplitude is \[S,S\]"):
        psiart.loss_and_gradients(img, np.ones((8, 8)), A, np.zeros(27), 0.025, 0.5)
    with pytest.raises(ValueError, match="27"):
        psiart.params_vector(np.zeros(25))
    with pytest.raises(ValueError, match="unknown parameter"):
        psiart.params_vector({"a21": 1.0})
    with pytest.raises(ValueError):
        psiart.ctf(12, 0.025, 0.5, np.zeros(27))
    with pytest.raises(ValueError):
        psiart.ctf(16, 0.025, 0.0, np.zeros(27))
    with pytest.raises(ValueError):
        psiart.forward(np.ones((16, 8)), A, np.zeros(27), [0.0], 0.025, 0.5)
    for bad in (dict(n=0), dict(n=5, middle=5)):
        with pytest.raises(ValueError):
            psiart.defocus_ramp(**bad)
    with pytest.raises(ValueError):
        psiart.boot_weights(5, 2, 5)
    with pytest.raises(ValueError):
        psiart.polar_grid(10, 0.5, 0.025)
    assert psiart.params_vector({"a40": 2.0, "focal_spread": 3.0})[[11, 25]].tolist() == [2.0, 3.0]


def test_convergence_is_a_property_of_the_formulas():
    """From a20 = 38 towards the truth 40 with the amplitude and phase free (S = 32, N = 5, 400 steps): measured on this restatement the
    loss falls from 1.96e-4 to 1.05e-8, a20 ends at 39.998 and the wave within 1.34e-3 of the truth after the best complex scale; the
    thresholds (also asserted on the device's run) leave a factor 10."""
    want, _, first = G.conv_reference()
    w = G.conv_inputs()[3]
    a20, loss, wd = want["params"][R.I_A20], want["losses"][-1], G.wave_distance(want["amp"], want["phase"], w)
    print(f"convergence on the restatement: loss {first:.3e} -> {loss:.3e}, a20 {G.CONV['start']} -> {a20:.5f}, wave within {wd:.3e}")
    assert first > 1e-4 and 10.0 * loss <= G.CONV_LOSS_MAX and 10.0 * abs(a20 - G.CONV["truth"]) <= G.CONV_A20_TOL
    assert 10.0 * wd <= G.CONV_WAVE_MAX
