"""GPU tests of the gradient-descent exit-wave and aberration fit (csrc/psiart.hip, emdenoise.psiart) against the
float64 numpy restatement of tests/psiart_ref.py, whose reverse pass tests/test_psiart.py checks against torch's autograd on the CPU.

Inputs: the wave of ``exitwave_ref.true_wave(S)``, lambda = energy2wavelength(200), sampling 0.5 A, ramp 3 |k - N // 2|, scale 5, and
the all-coefficient point of ``psiart_ref.all_coefficient_point``: every amplitude contributes 1.5 .. 4.5 rad at the grid's largest
theta, every azimuth is non-zero, focal spread 15 .. 20 A, u 0.2 .. 0.3.  The images are float32(|b_k|^2) of the restatement at that
point; the model is evaluated OFF it (parameters 10 % away, amplitude and phase perturbed), so that the residual is not rounding noise.
Conditions, asserted on the CPU before the GPU is touched: min|b_k| / mean|b_k| >= 0.2, max|chi| <= 400, kappa <= 1e6, and every
scalar gradient's sum of |terms| > 0 (a20's is 0 where the ramp is: N = 1; the device must then give exactly 0).

No bar comes from the device.  Each is FACTOR = 4 times a yardstick: the largest distance, over this file's cases, between the
restatement as written (numpy.fft, float64) and the same restatement on the radix-2 FFT of tests/fft_ref.py with chi, T and the basis
functions evaluated in numpy.longdouble and rounded.  ``python -m tests.test_psiart_gpu`` computes them on the CPU; they are written
below.

* Fields (C, p, dL/dA, dL/dP): relative L2, FIELD_YARD.
* Losses: relative, 4 x (field bar) x sqrt(kappa), kappa = sum r^2 / sum d^2 (as the exit-wave reconstruction's losses).
* Each scalar gradient: |error| <= FACTOR x SCALAR_YARD x (the sum over frequencies and images of |term|, from the restatement).
* Trajectories (20 steps; the convergence run): TRAJ_YARD / CONV_YARD, the same distance between the two restatements' trajectories
  (psiart_ref.state_distance).

Every figure is printed before it is asserted."""
import functools

import numpy as np
import pytest
import torch

from emdenoise import _lib, exitwave, psiart
from tests import psiart_ref as R
from tests.guarded import assert_written, guarded

pytestmark = pytest.mark.gpu

FACTOR = 4.0
FIELD_YARD = 1.002e-14      # python -m tests.test_psiart_gpu: dL/dP of (1, 2048); C alone is within 1.2e-15, p within 1.4e-15
SCALAR_YARD = 4.798e-15     # of the sum of |terms|: the (3, 16) amplitude-target case
TRAJ_YARD = 1.830e-13       # the first moment of the amplitude after 20 steps at (4, 64); parameters stay within 1.1e-14
CONV_YARD = 1.281e-06       # a20 and the fields after the 400 steps of the convergence run
UNIT_MODULUS_BAR = 2.0 ** -51  # focal spread 0: | |C| - 1 |, 2 ulp of 1.0 (derived in test_loss_and_gradients_variants)
RATIO_MIN, CHI_MAX, KAPPA_MAX = 0.2, 400.0, 1e6
LAM, SAMPLING, SCALE = R.LAM, R.SAMPLING, R.SCALE
SMALL_CASES = [(3, 8), (5, 16), (4, 64)]
LARGE_CASES = [(2, 256), (2, 512), (2, 1024), (1, 2048)]        # 1, 2, 4 and 8 elements of a line per thread in the column kernels
LG_CASES = [(N, S, norm) for N, S in SMALL_CASES for norm in (True, False)] + [(N, S, True) for N, S in LARGE_CASES]
VARIANTS = [(1, 16, "all"), (3, 16, "amplitudes"), (3, 16, "nospread")]
STEP_CASES = [(5, 16), (4, 64)]
CTF_SIZES = [8, 64, 256]
# the convergence property (asserted on the restatement in tests/test_psiart.py, thresholds with a factor 10 of slack over its run)
CONV = dict(S=32, N=5, truth=40.0, start=38.0, rate_a20=0.02, rate_fields=0.01, steps=400, beta1=0.9, epsilon=1e-8)
CONV_LOSS_MAX, CONV_A20_TOL, CONV_WAVE_MAX = 1.1e-7, 2e-2, 1.4e-2


def field_bar():
    return FACTOR * FIELD_YARD


def ids(c):
    return "x".join(str(v) for v in c)


def dev():
    return torch.device("cuda", 0)


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def host(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def inputs(N, S, variant="all"):
    """-> (case dict, amplitudes flag).  Cached: do not write into the result."""
    c = dict(R.case(N, S, spread=variant != "nospread"))
    if variant == "amplitudes":
        c["images"] = np.sqrt(c["images"].astype(np.float64)).astype(np.float32) * np.float32(-1.0)   # |image| is the target
    if variant == "nospread":
        c["params"] = c["params"].copy()
        c["params"][R.I_SPREAD] = 0.0
    return c, variant == "amplitudes"


@functools.lru_cache(maxsize=None)
def reference(N, S, norm=True, variant="all", second=False):
    c, amps = inputs(N, S, variant)
    kw = dict(fft=R.Radix2FFT, ctf_dtype=np.longdouble) if second else {}
    return R.loss_and_gradients(c["images"], c["amp"], c["phase"], c["params"], c["ramp"], c["weights"], LAM, SAMPLING, SCALE, norm, amps, **kw)


def conditions(want, ramp, what, spread=True):
    at = want["abs_terms"]
    print(f"{what}: min|b| / mean|b| {want['ratio']:.3f}, max|chi| {want['chimax']:.1f}, kappa {want['kappa'].max():.3e}, smallest sum of "
          f"|terms| {at.min():.3e}")
    assert want["ratio"] >= RATIO_MIN and want["chimax"] <= CHI_MAX and want["kappa"].max() <= KAPPA_MAX
    free = np.ones(R.NPARAM, bool)
    free[R.I_A20] = bool(np.any(np.asarray(ramp) != 0))                    # a20's terms carry the ramp
    free[R.I_SPREAD] = spread                                              # focal spread 0: its terms are 0
    assert (at[free] > 0).all()


def device_lg(N, S, norm=True, variant="all", **kw):
    c, amps = inputs(N, S, variant)
    return psiart.loss_and_gradients(up(c["images"]), up(c["amp"]), up(c["phase"]), up(c["params"]), LAM, SAMPLING, ramp=up(c["ramp"]),
                                     weights=up(c["weights"]), offset_scale=SCALE, normalise=norm, from_intensity=not amps,
                                     predictions=True, **kw)


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
    es = np.abs(got["g_params"] - want["g_params"])
    bs = FACTOR * SCALAR_YARD * want["abs_terms"]
    with np.errstate(invalid="ignore", divide="ignore"):
        worst = np.nanmax(np.where(want["abs_terms"] > 0, es / want["abs_terms"], 0.0))
    print(f"{what} scalar gradients: largest |error| / sum|terms| {worst:.3e}; bar {FACTOR * SCALAR_YARD:.3e}; gradients from "
          f"{np.abs(want['g_params']).min():.2e} to {np.abs(want['g_params']).max():.2e}")
    assert (es <= bs).all(), (what, np.nonzero(es > bs)[0])


# ---- the contrast transfer function -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", CTF_SIZES)
def test_ctf(S):
    p = R.all_coefficient_point(S)
    ramp = R.defocus_ramp(3)
    want, chimax = R.ctf(S, SAMPLING, LAM, p, ramp, SCALE)
    assert chimax <= CHI_MAX
    got = psiart.ctf(S, LAM, SAMPLING, p, ramp, SCALE)
    assert isinstance(got, np.ndarray) and got.dtype == np.complex128 and got.shape == (3, S, S)
    e = R.rel_l2(got, want)
    print(f"ctf S = {S}: rel L2 {e:.3e}; bar {field_bar():.3e}; max|chi| {chimax:.1f}")
    assert e <= field_bar()
    assert (got[:, 0, 0] == 1.0).all()                                      # theta = 0: exactly 1
    a20, a40 = 300.0, 4e5                                                   # only defocus and Cs: conj of the Fresnel transfer function
    two = psiart.ctf(S, LAM, SAMPLING, {"a20": a20, "a40": a40}, [1.0])
    H = exitwave.transfer_function(S, LAM, a20, px=SAMPLING, cs=a40)
    e2 = R.rel_l2(two[0], np.conj(H))
    print(f"ctf S = {S}, a20 and a40 only, against conj transfer_function: rel L2 {e2:.3e}; bar {field_bar():.3e}")
    assert e2 <= field_bar() and R.rel_l2(two[0], H) > 0.1
    t = psiart.ctf(S, LAM, SAMPLING, up(p), up(ramp), SCALE)
    assert t.is_cuda and np.array_equal(t.cpu().numpy(), got)


def test_forward_with_defocus_only_is_fresnel_propagation():
    N, S, a20 = 3, 64, 60.0
    c, _ = inputs(N, S)
    ramp = R.defocus_ramp(N)
    psi = up(c["amp"] * np.exp(1j * c["phase"]))
    want = exitwave.propagate(psi.expand(N, S, S).contiguous(), up(-a20 * ramp), LAM, px=SAMPLING).abs()
    got = psiart.forward(up(c["amp"]), up(c["phase"]), {"a20": a20}, ramp, LAM, SAMPLING)
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (N, S, S)
    e = float(torch.linalg.norm((got - want).reshape(-1)) / torch.linalg.norm(want.reshape(-1)))
    print(f"forward, a20 only, against |propagate(psi, -a20_k)|: rel L2 {e:.3e}; bar {field_bar():.3e}")
    assert e <= field_bar()
    assert float((want[0] - want[1]).abs().max()) > 1e-3                    # the foci differ


# ---- loss and gradients -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", LG_CASES, ids=ids)
def test_loss_and_gradients(case):
    N, S, norm = case
    want = reference(N, S, norm)
    conditions(want, inputs(N, S)[0]["ramp"], f"loss_and_gradients {case}")
    got = device_lg(N, S, norm)
    assert got["g_amplitude"].is_cuda and got["losses"].dtype == torch.float64 and tuple(got["predictions"].shape) == (N, S, S)
    check_lg(host(got), want, f"{case}")
    if N == 1:
        assert float(got["g_params"][R.I_A20]) == 0.0                      # the ramp of one image is 0


@pytest.mark.parametrize("case", VARIANTS, ids=ids)
def test_loss_and_gradients_variants(case):
    """One image; |image| as the target (EMD_PSIART_AMPLITUDES, the images negated so that the root would be 0); focal spread 0."""
    N, S, variant = case
    want = reference(N, S, True, variant)
    conditions(want, inputs(N, S, variant)[0]["ramp"], f"{case}", variant != "nospread")
    got = host(device_lg(N, S, True, variant))
    check_lg(got, want, f"{case}")
    if variant == "nospread":
        # T is exactly 1, so |C| = |cospi(t) - i sinpi(t)| leaves 1 only by rounding: sinpi and cospi within 1 ulp of values below 1
        # (2^-53) move the modulus by at most (|c| + |s|) 2^-53 <= sqrt(2) 2^-53, numpy's hypot rounds it by at most 2^-52 more; the sum,
        # 1.71 x 2^-52, is under UNIT_MODULUS_BAR = 2 ulp of 1.0, on both sides
        par = inputs(N, S, variant)[0]["params"]
        assert par[R.I_SPREAD] == 0.0 and (R.ctf_parts(S, SAMPLING, LAM, par)["T"] == 1.0).all()
        C = psiart.ctf(S, LAM, SAMPLING, par, inputs(N, S, variant)[0]["ramp"], SCALE)
        off = np.abs(np.abs(C) - 1.0)
        print(f"{case} focal spread 0: | |C| - 1 | <= {off.max():.3e} over {C.shape}; bar {UNIT_MODULUS_BAR:.3e}; dL/dspread "
              f"{got['g_params'][R.I_SPREAD]!r}")
        assert C.shape == (N, S, S) and (off <= UNIT_MODULUS_BAR).all() and got["g_params"][R.I_SPREAD] == 0.0
        with_spread = psiart.ctf(S, LAM, SAMPLING, inputs(N, S)[0]["params"], [0.0], SCALE)
        assert np.abs(with_spread).min() < 0.999                           # the envelope is there when the spread is


def test_images_with_weight_zero_do_not_contribute():
    N, S = 5, 16
    c, _ = inputs(N, S)
    w = c["weights"].copy()
    w[[1, 3]] = 0.0
    keep = [0, 2, 4]
    full = psiart.loss_and_gradients(up(c["images"]), up(c["amp"]), up(c["phase"]), up(c["params"]), LAM, SAMPLING, ramp=up(c["ramp"]),
                                     weights=up(w), offset_scale=SCALE)
    part = psiart.loss_and_gradients(up(c["images"][keep]), up(c["amp"]), up(c["phase"]), up(c["params"]), LAM, SAMPLING,
                                     ramp=up(c["ramp"][keep]), weights=up(w[keep]), offset_scale=SCALE)
    for k in ("g_amplitude", "g_phase", "g_params", "loss"):
        assert torch.equal(full[k], part[k]), k                            # bitwise: the others are unchanged, the two vanish
    assert torch.equal(full["losses"][keep], part["losses"]) and float(full["g_amplitude"].abs().max()) > 0


def test_an_all_zero_wave_under_normalisation_gives_nan_losses_and_zero_gradients():
    """mean|b_k| = 0: c_k = mean(r_k) / 0 is not finite, so the losses and the predictions are NaN, as the header documents; G_b is 0
    where |b_k| = 0, so every gradient is exactly 0 and a step leaves finite parameters behind."""
    N, S = 3, 16
    c, _ = inputs(N, S)
    zero = dict(c, amp=np.zeros((S, S)))
    out = host(psiart.loss_and_gradients(up(c["images"]), up(zero["amp"]), up(c["phase"]), up(c["params"]), LAM, SAMPLING, ramp=up(c["ramp"]),
                                         weights=up(c["weights"]), offset_scale=SCALE, predictions=True))
    assert np.isnan(out["losses"]).all() and np.isnan(out["loss"]) and np.isnan(out["predictions"]).all()
    for k in ("g_amplitude", "g_phase", "g_params"):
        assert not out[k].any(), k
    fit = make_fit(zero, step_rates(c)).step(2)
    s = fit_state(fit)
    assert not s["amp"].any() and np.array_equal(s["phase"], c["phase"]) and np.array_equal(s["params"], c["params"])
    plain = host(psiart.loss_and_gradients(up(c["images"]), up(zero["amp"]), up(c["phase"]), up(c["params"]), LAM, SAMPLING,
                                           ramp=up(c["ramp"]), weights=up(c["weights"]), offset_scale=SCALE, normalise=False))
    r = R.targets(c["images"])
    # without it p = 0 and loss_k = mean(r_k^2); two sums of S^2 positive terms, each within S^2 2^-53 whatever their order
    assert np.allclose(plain["losses"], (r * r).mean(axis=(1, 2)), rtol=2 * S * S * 2.0 ** -53, atol=0.0)


# ---- steps --------------------------------------------------------------------------------------------------------------------------

def step_rates(c):
    return np.concatenate([[0.01, 0.01], 1e-3 * np.abs(c["params"])])


def make_fit(c, rates, amps=False, **kw):
    fit = psiart.PsiArtFit(up(c["images"]), LAM, SAMPLING, ramp=up(c["ramp"]), rates=up(rates), offset_scale=SCALE, from_intensity=not amps,
                           **kw)
    fit._amp.copy_(up(c["amp"]))
    fit._phase.copy_(up(c["phase"]))
    fit._params.copy_(up(c["params"]))
    return fit.set_weights(up(c["weights"]))


def fit_state(fit):
    m = [t.cpu().numpy() for t in fit._moments]
    return {"amp": fit._amp.cpu().numpy(), "phase": fit._phase.cpu().numpy(), "params": fit._params.cpu().numpy(), "m_amp": m[0],
            "v_amp": m[1], "m_phase": m[2], "v_phase": m[3], "m_params": m[4], "v_params": m[5], "losses": fit._losses.cpu().numpy()}


@functools.lru_cache(maxsize=None)
def ref_trajectory(N, S, steps, second=False, **kw):
    c, _ = inputs(N, S)
    extra = dict(fft=R.Radix2FFT, ctf_dtype=np.longdouble) if second else {}
    f = R.Fit(c["images"], c["amp"], c["phase"], c["params"], c["ramp"], c["weights"], step_rates(c), LAM, SAMPLING, SCALE, **kw, **extra)
    for _ in range(steps):
        f.step()
    return f.state(), f.scale


def check_state(got, want, scale, bar, what):
    d = R.state_distance(got, want, scale)
    print(f"{what}: " + ", ".join(f"{k} {v:.2e}" for k, v in d.items()) + f"; bar {bar:.3e}")
    assert max(d.values()) <= bar, what


@pytest.mark.parametrize("case", STEP_CASES, ids=ids)
def test_twenty_steps(case):
    N, S = case
    c, _ = inputs(N, S)
    want, scale = ref_trajectory(N, S, 20, beta1=0.9, epsilon=1e-8)
    assert (step_rates(c) != 0).all()
    fit = make_fit(c, step_rates(c), beta1=0.9, epsilon=1e-8).step(20)
    assert fit.steps == 20
    check_state(fit_state(fit), want, scale, FACTOR * TRAJ_YARD, f"20 steps {case}")
    moved = R.rel_l2(want["phase"], c["phase"])
    print(f"  the phase moved by {moved:.3e} (relative L2) over the 20 steps")
    assert moved > 1e6 * FACTOR * TRAJ_YARD                                # an update that does nothing fails by far


def test_five_steps_with_the_reference_optimiser():
    N, S = 5, 16
    c, _ = inputs(N, S)
    want, scale = ref_trajectory(N, S, 5)                                  # beta1 = 0.99, epsilon = 0.1
    fit = make_fit(c, step_rates(c)).step(5)
    check_state(fit_state(fit), want, scale, FACTOR * TRAJ_YARD, "5 steps, beta1 = 0.99, epsilon = 0.1")


def test_rate_zero_freezes_a_parameter_and_its_moments():
    N, S = 3, 16
    c, _ = inputs(N, S)
    rates = step_rates(c)
    rates[0] = 0.0                                                          # the amplitude field
    rates[2 + 11] = rates[2 + R.I_SPREAD] = 0.0                             # a40 and the focal spread
    fit = make_fit(c, rates, beta1=0.9, epsilon=1e-8)
    idt, word = torch.int64, 0x7FF8A5C3A5C3A5C3                             # tests/guarded.py's NaN
    fit._moments[0].view(idt).fill_(word)                                   # a field with rate 0 is not written: sentinels stay
    fit._moments[1].view(idt).fill_(word)
    fit._moments[4][11] = 7.5
    fit._moments[5][R.I_SPREAD] = 8.5
    before = fit_state(fit)
    fit.step(3)
    after = fit_state(fit)
    assert np.array_equal(after["amp"], before["amp"])
    assert bool((fit._moments[0].view(idt) == word).all()) and bool((fit._moments[1].view(idt) == word).all())
    for i in (11, R.I_SPREAD):
        assert after["params"][i] == before["params"][i] and after["m_params"][i] == before["m_params"][i] \
            and after["v_params"][i] == before["v_params"][i]
    assert after["m_params"][11] == 7.5 and after["v_params"][R.I_SPREAD] == 8.5
    others = [i for i in range(R.NPARAM) if i not in (11, R.I_SPREAD)]
    assert (after["params"][others] != before["params"][others]).all() and not np.array_equal(after["phase"], before["phase"])


def conv_inputs():
    S, N = CONV["S"], CONV["N"]
    truth = np.zeros(R.NPARAM)
    truth[R.I_A20] = CONV["truth"]
    ramp = R.defocus_ramp(N)
    C, _ = R.ctf(S, SAMPLING, LAM, truth, ramp, 1.0)
    w = R.true_wave(S)
    images = np.stack([np.abs(np.fft.ifft2(C[k] * np.fft.fft2(w))) ** 2 for k in range(N)]).astype(np.float32)
    rates = np.zeros(R.NPARAM + 2)
    rates[0] = rates[1] = CONV["rate_fields"]
    rates[2 + R.I_A20] = CONV["rate_a20"]
    return images, ramp, rates, w


@functools.lru_cache(maxsize=None)
def conv_reference(second=False):
    images, ramp, rates, w = conv_inputs()
    S, N = CONV["S"], CONV["N"]
    p0 = np.zeros(R.NPARAM)
    p0[R.I_A20] = CONV["start"]
    extra = dict(fft=R.Radix2FFT, ctf_dtype=np.longdouble) if second else {}
    f = R.Fit(images, np.sqrt(images[N // 2].astype(np.float64)), np.zeros((S, S)), p0, ramp, np.full(N, 1.0 / N), rates, LAM, SAMPLING, 1.0,
              beta1=CONV["beta1"], epsilon=CONV["epsilon"], **extra)
    first = None
    for _ in range(CONV["steps"]):
        l = f.step()
        first = l[-1] if first is None else first
    return f.state(), f.scale, first


def wave_distance(amp, phase, w):
    psi = amp * np.exp(1j * phase)
    return R.rel_l2(np.vdot(psi, w) / np.vdot(psi, psi) * psi, w)


def conv_distance(got, want):
    """a20 relative, the fields by relative L2 (the trajectory is long: the losses near the minimum are not compared)."""
    return max(abs(got["params"][R.I_A20] / want["params"][R.I_A20] - 1.0), R.rel_l2(got["amp"], want["amp"]),
               R.rel_l2(got["phase"], want["phase"]))


def test_convergence_to_the_true_defocus():
    images, ramp, rates, w = conv_inputs()
    want, _, first = conv_reference()
    fit = psiart.PsiArtFit(up(images), LAM, SAMPLING, symbols=("a20",), estimates=(CONV["start"],), rates=up(rates), beta1=CONV["beta1"],
                           epsilon=CONV["epsilon"]).step(CONV["steps"])
    got = fit_state(fit)
    a20, loss, wd = got["params"][R.I_A20], got["losses"][-1], wave_distance(got["amp"], got["phase"], w)
    d = conv_distance(got, want)
    print(f"convergence: loss {first:.3e} -> {loss:.3e} (restatement {want['losses'][-1]:.3e}), a20 {CONV['start']} -> {a20:.5f} "
          f"(restatement {want['params'][R.I_A20]:.5f}, truth {CONV['truth']}), wave within {wd:.3e} of the truth; distance from the "
          f"restatement's end {d:.3e}; bar {FACTOR * CONV_YARD:.3e}")
    assert loss <= CONV_LOSS_MAX and abs(a20 - CONV["truth"]) <= CONV_A20_TOL and wd <= CONV_WAVE_MAX
    assert d <= FACTOR * CONV_YARD
    assert fit.aberrations["a20"] == a20 and fit.aberrations["a40"] == 0.0


# ---- house checks -------------------------------------------------------------------------------------------------------------------

def test_the_same_bits_twice():
    N, S = 4, 64
    a, b = device_lg(N, S), device_lg(N, S)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    c, _ = inputs(N, S)
    f1, f2 = make_fit(c, step_rates(c)).step(3), make_fit(c, step_rates(c)).step(3)
    s1, s2 = fit_state(f1), fit_state(f2)
    for k in s1:
        assert np.array_equal(s1[k], s2[k]), k


@pytest.mark.parametrize("case", [(3, 16), (2, 512)], ids=ids)
def test_guarded_workspace_and_outputs(case):
    """The workspace at its advertised size, filled with NaN, and every output between guards."""
    N, S = case
    c, _ = inputs(N, S)
    lib = _lib.load()
    nbytes = lib.emd_psiart_workspace_bytes(N, S)
    assert nbytes % 8 == 0 and nbytes > 0
    d = dev()
    g64 = lambda n, fill=None, name="": guarded(n, torch.float64, d, fill=fill, name=name)
    ws, ws_g = g64(nbytes // 8, name="workspace")
    names = ["amp", "phase", "params", "m_amp", "v_amp", "m_phase", "v_phase", "m_params", "v_params", "losses", "pred", "g_amp", "g_phase",
             "g_params"]
    sizes = [S * S, S * S, 27, S * S, S * S, S * S, S * S, 27, 27, N + 1, N * S * S, S * S, S * S, 27]
    fills = [c["amp"], c["phase"], c["params"], 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, None, None, None, None, None]
    bufs = {n: g64(s, f, n) for n, s, f in zip(names, sizes, fills)}
    step = torch.zeros(1, dtype=torch.int32, device=d)
    x, ramp, w, rates = up(c["images"]), up(c["ramp"]), up(c["weights"]), up(step_rates(c))
    p = lambda n: _lib.ptr(bufs[n][0])
    rc = lib.emd_psiart_step_f64(_lib.ptr(x), N, S, p("amp"), p("phase"), p("params"), _lib.ptr(ramp), _lib.ptr(w), LAM, SAMPLING, SCALE, 1,
                                 p("m_amp"), p("v_amp"), p("m_phase"), p("v_phase"), p("m_params"), p("v_params"), _lib.ptr(step),
                                 _lib.ptr(rates), 0.9, 0.999, 1e-8, p("losses"), p("pred"), p("g_amp"), p("g_phase"), p("g_params"),
                                 _lib.ptr(ws), nbytes, _lib.stream_ptr())
    _lib.check(rc, "emd_psiart_step_f64")
    torch.cuda.synchronize()
    ws_g()
    for n in names:
        bufs[n][1]()
        assert_written(bufs[n][0], n)
        assert bool(torch.isfinite(bufs[n][0]).all()), n                    # nothing read the workspace's NaN before writing it
    want = reference(N, S)
    assert int(step) == 1
    got = {"predictions": bufs["pred"][0].view(N, S, S), "g_amplitude": bufs["g_amp"][0].view(S, S), "g_phase": bufs["g_phase"][0].view(S, S),
           "g_params": bufs["g_params"][0], "losses": bufs["losses"][0][:N], "loss": bufs["losses"][0][N]}
    check_lg(host(got), want, f"guarded step {case}")
    rc = lib.emd_psiart_step_f64(_lib.ptr(x), N, S, p("amp"), p("phase"), p("params"), _lib.ptr(ramp), _lib.ptr(w), LAM, SAMPLING, SCALE, 1,
                                 p("m_amp"), p("v_amp"), p("m_phase"), p("v_phase"), p("m_params"), p("v_params"), _lib.ptr(step),
                                 _lib.ptr(rates), 0.9, 0.999, 1e-8, p("losses"), p("pred"), p("g_amp"), p("g_phase"), p("g_params"),
                                 _lib.ptr(ws), nbytes - 256, _lib.stream_ptr())
    assert rc == -1 and b"workspace too small" in lib.emd_last_error()


def test_a_captured_step_replays_with_new_images_weights_and_rates():
    N, S = 5, 16
    c, _ = inputs(N, S)
    images, weights, rates = up(c["images"]), up(c["weights"]), up(step_rates(c))
    fit = psiart.PsiArtFit(images, LAM, SAMPLING, ramp=up(c["ramp"]), rates=rates, offset_scale=SCALE, beta1=0.9, epsilon=1e-8)
    fit.set_weights(weights)
    assert fit.images.data_ptr() == images.data_ptr() and fit._weights.data_ptr() == weights.data_ptr() \
        and fit._rates.data_ptr() == rates.data_ptr()                       # used where they are
    fit._params.copy_(up(c["params"]))
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fit.step()                                                          # warm-up
        with torch.cuda.graph(graph, stream=side):
            fit.step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert fit.steps == 1                                                   # capturing runs nothing
    new_images = np.roll(c["images"], 1, axis=0) * np.float32(1.1)
    new_w = R.boot_weights(N, N // 2, 3)
    images.copy_(up(new_images))
    weights.copy_(up(new_w))
    rates.mul_(0.5)
    twin = psiart.PsiArtFit(up(new_images), LAM, SAMPLING, ramp=up(c["ramp"]), rates=rates.clone(), offset_scale=SCALE, beta1=0.9,
                            epsilon=1e-8).set_weights(new_w)
    for a, b in zip([twin._amp, twin._phase, twin._params, twin._step] + twin._moments,
                    [fit._amp, fit._phase, fit._params, fit._step] + fit._moments):
        a.copy_(b)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    twin.step(2)
    s1, s2 = fit_state(fit), fit_state(twin)
    assert fit.steps == 3 and twin.steps == 3
    for k in s1:
        assert np.array_equal(s1[k], s2[k]), k
    assert abs(s1["losses"][N] / float(np.dot(new_w, s1["losses"][:N])) - 1.0) < 1e-12      # L is weighted with the new weights


def test_numpy_and_tensor_conventions():
    N, S = 3, 16
    c, _ = inputs(N, S)
    out = psiart.loss_and_gradients(c["images"], c["amp"], c["phase"], c["params"], LAM, SAMPLING, ramp=c["ramp"], weights=c["weights"],
                                    offset_scale=SCALE)
    assert all(isinstance(v, np.ndarray) for v in out.values()) and out["g_amplitude"].shape == (S, S) and out["g_params"].shape == (27,)
    t = device_lg(N, S)
    assert all(v.is_cuda for v in t.values())
    for k in out:
        assert np.array_equal(out[k], t[k].cpu().numpy()), k
    only = psiart.loss_and_gradients(c["images"], c["amp"], c["phase"], c["params"], LAM, SAMPLING, ramp=c["ramp"], weights=c["weights"],
                                     offset_scale=SCALE, gradients=False)
    assert sorted(only) == ["loss", "losses"] and np.array_equal(only["losses"], out["losses"])
    fit = psiart.PsiArtFit(c["images"], LAM, SAMPLING)
    assert isinstance(fit.amplitude, np.ndarray) and isinstance(fit.loss, float) and fit.wave.dtype == np.complex128
    assert np.array_equal(fit.amplitude, np.sqrt(np.maximum(c["images"][N // 2].astype(np.float64), 0.0))) and not fit.phase.any()
    assert fit.aberrations["a20"] == 50.0 and fit.aberrations["a40"] == 0.0 and set(fit.aberrations) == set(psiart.PARAM_NAMES)
    r = fit._rates.cpu().numpy()
    assert r[0] == r[1] == r[2 + 2] == r[2 + 11] == r[28] == 1e-3 and r.sum() == 5e-3      # the symbols named are trained
    fit.step(2)
    assert fit.steps == 2 and fit.losses.shape == (N,) and np.isfinite(fit.loss)
    fit.set_rates(a20=0.0)
    a20 = fit.aberrations["a20"]
    fit.step()
    assert fit.aberrations["a20"] == a20
    dfit = psiart.PsiArtFit(up(c["images"]), LAM, SAMPLING)
    assert dfit.amplitude.is_cuda and dfit.loss.is_cuda and dfit.wave.dtype == torch.complex128
    with pytest.raises(ValueError):
        psiart.PsiArtFit(up(c["images"]), LAM, SAMPLING, rates=up(np.zeros(28)))


# ---- the yardsticks (CPU) -----------------------------------------------------------------------------------------------------------

def yardsticks(large=True, conv=True):
    """-> (field, scalar, trajectory, convergence).  ``large=False`` leaves LARGE_CASES out and ``conv=False`` the 400-step run on the
    radix-2 transform (convergence is then None): tests/test_psiart.py recomputes the rest on every run and holds the constants above
    against it (the scalar and trajectory yardsticks are attained there)."""
    field = scalar = traj = 0.0
    lg_cases = [c for c in LG_CASES if large or c[:2] not in LARGE_CASES]
    for S in CTF_SIZES:
        p, ramp = R.all_coefficient_point(S), R.defocus_ramp(3)
        e = R.rel_l2(R.ctf(S, SAMPLING, LAM, p, ramp, SCALE, np.longdouble)[0], R.ctf(S, SAMPLING, LAM, p, ramp, SCALE)[0])
        print(f"yardstick ctf {S}: {e:.3e}")
        field = max(field, e)
    for case in [(N, S, norm, "all") for N, S, norm in lg_cases] + [(N, S, True, v) for N, S, v in VARIANTS]:
        a, b = reference(*case, second=True), reference(*case)
        e = {k: R.rel_l2(a[k], b[k]) for k in ("C", "p", "g_amp", "g_phase")}
        with np.errstate(invalid="ignore", divide="ignore"):
            s = float(np.nanmax(np.where(b["abs_terms"] > 0, np.abs(a["g_params"] - b["g_params"]) / b["abs_terms"], 0.0)))
        print(f"yardstick loss_and_gradients {case}: " + ", ".join(f"{k} {v:.3e}" for k, v in e.items()) + f", scalars {s:.3e}; "
              f"losses {np.abs(a['losses'] / b['losses'] - 1).max():.3e}; ratio {b['ratio']:.3f}, max|chi| {b['chimax']:.1f}, kappa "
              f"{b['kappa'].max():.3e}")
        field, scalar = max(field, *e.values()), max(scalar, s)
    for (N, S), steps, kw in [(c, 20, dict(beta1=0.9, epsilon=1e-8)) for c in STEP_CASES] + [((5, 16), 5, {})]:
        (a, _), (b, scale) = ref_trajectory(N, S, steps, second=True, **kw), ref_trajectory(N, S, steps, **kw)
        d = R.state_distance(a, b, scale)
        print(f"yardstick {steps} steps {(N, S)} {kw}: " + ", ".join(f"{k} {v:.2e}" for k, v in d.items()))
        traj = max(traj, *d.values())
    if not conv:
        return field, scalar, traj, None
    (a, _, _), (b, _, first) = conv_reference(True), conv_reference()
    w = conv_inputs()[3]
    conv = conv_distance(a, b)
    print(f"convergence on the restatement: loss {first:.3e} -> {b['losses'][-1]:.3e}, a20 -> {b['params'][R.I_A20]:.5f}, wave within "
          f"{wave_distance(b['amp'], b['phase'], w):.3e}; the two restatements end {conv:.3e} apart")
    return field, scalar, traj, conv


if __name__ == "__main__":
    print("FIELD_YARD = %.3e\nSCALAR_YARD = %.3e\nTRAJ_YARD = %.3e\nCONV_YARD = %.3e" % yardsticks())
