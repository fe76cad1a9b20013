"""GPU tests of the focal-series reconstruction (csrc/exitwave.hip, emdenoise.exitwave) against the float64 numpy
restatement of tests/exitwave_ref.py (the reference's order: real-space mean, two full propagations per image per iteration).

Inputs: a simulated series.  From two images u, v of ``synthetic_lq`` the true wave is (1 + 0.1 (u - mean u)) exp(0.3 i (v - mean v));
the images are |P(wave, df_k)| as float32 with lambda = 2.51e-12, px = 1e-10 and df_k = 2e-8 sign(k - mid) (k - mid)^2 + 1e-8.
Condition, asserted on the CPU before the GPU is touched: min |b_k| / mean |b_k| >= 0.2 in every iteration of the restatement, so the
modulus division never amplifies.

The bars are not derived from the device's output.

* Waves (fft2, propagate, reconstruct, stack): relative L2 against the restatement; the bar is FACTOR = 4 times YARD, the LARGEST
  relative L2 distance, over the cases of this file, between the restatement run with ``numpy.fft`` and the same restatement run with
  the plain float64 radix-2 FFT of tests/fft_ref.py: two honest float64 evaluations of the same formulas.  Computed on the CPU by
  ``python -m tests.test_exitwave_gpu`` (no GPU) and written below.
* Transfer function: absolute 2^-50 per component against the fmod-reduced restatement: the reduction is exact, pi r rounds below
  2^-51, and each library's sin / cos is within 2 ulp.
* Losses: relative 4 x (wave bar) x sqrt(kappa), kappa = sum image^2 / sum (image - c I)^2, asserted <= 1e6 on the CPU first; the
  loss tests run with the defocuses scaled by 1.5, so that the residual is not rounding noise.

Every figure is printed before it is asserted."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from emdenoise import _lib, exitwave, harvest
from tests import exitwave_ref as R
from tests.synth_inputs import synthetic_lq

pytestmark = pytest.mark.gpu

FACTOR = 4.0
YARD = 5.882e-16           # the largest distance of the two float64 restatements over the cases below (python -m tests.test_exitwave_gpu)
TF_BAR = 2.0 ** -50
RATIO_MIN, KAPPA_MAX = 0.2, 1e6
LAM, PX = R.WAVELENGTH, R.PX
FFT_SIZES = [(2, 8), (2, 16), (2, 32), (2, 64), (2, 128), (2, 256), (2, 1024)]
PROP_CASES = [(2, 8, 0), (3, 32, 0), (2, 256, 0), (2, 8, 1), (2, 32, 1), (2, 16, 3), (1, 1024, 0)]
RECON_CASES = [(1, 8, 0, 1), (2, 8, 0, 2), (3, 16, 0, 5), (5, 32, 0, 5), (3, 64, 0, 5), (3, 128, 0, 10), (2, 8, 1, 2), (3, 32, 1, 3),
               (3, 16, 3, 2), (9, 256, 0, 2)]
CS = 1e-3                                                                  # with it H(-df) is far from conj H(df): see test_exitwave.py
CS_PROP_CASES = [(3, 32, 0), (2, 16, 1)]
CS_RECON_CASES = [(3, 32, 0, 3), (2, 16, 1, 2)]
LARGE_CASES = [(2, 512, 0, 3), (2, 1024, 0, 2)]                           # 2 and 4 elements of a line per thread in the column kernel
SENTINEL = -12345.5
# Five increments around the true one (1e-8), N = 3, s = 32, 5 iterations.  The reference's loss compares the image with an INTENSITY,
# c |b|^2.  On the amplitude series of this file it therefore does not vanish at the true defocuses and its minimum is shallow: the
# restatement gives 5.495e-4, 5.519e-4, 5.452e-4, 5.544e-4, 5.714e-4 over the geometric increments below (smallest at the true one)
# but 5.519e-4, 5.283e-4, 5.452e-4, 5.392e-4, 5.332e-4 over 0.5, 0.75, 1, 1.25, 1.5 x 1e-8 (not at the true one: a property of the
# formulas, not of the device).  On the squared images with from_intensity the minimum is deep at either spacing: 2.30e-4, 1.18e-4,
# 5.27e-5, 1.12e-4, 1.75e-4.
SWEEPS = [("amplitude", lambda im: im, (0.25e-8, 0.5e-8, 1e-8, 2e-8, 4e-8), False),
          ("intensity", lambda im: (im.astype(np.float64) ** 2).astype(np.float32), (0.5e-8, 0.75e-8, 1e-8, 1.25e-8, 1.5e-8), True)]


def wave_bar():
    return FACTOR * YARD


def loss_bar(kappa):
    return 4.0 * wave_bar() * float(np.sqrt(kappa))


def ids(c):
    return "x".join(str(v) for v in c)


def dev():
    return torch.device("cuda", 0)


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def bits(t):
    return torch.view_as_real(t) if t.is_complex() else t


@functools.lru_cache(maxsize=None)
def waves(B, S):
    """[B,S,S] complex128 test waves.  Cached: do not write into the result."""
    x = synthetic_lq(2 * B, S, S, seed=900 + S)[..., 0].astype(np.float64)
    return (x[:B] - 0.5) + 1j * (x[B:] - 0.3)


def prop_defocuses(B):
    return np.array([3e-8, -5e-8, 1.2e-7])[:B]


@functools.lru_cache(maxsize=None)
def prop_ref(B, s, pad, fft=R.NumpyFFT, cs=0.0):
    return np.stack([R.propagate(w, d, LAM, PX, cs, pad, fft) for w, d in zip(waves(B, s), prop_defocuses(B))])


@functools.lru_cache(maxsize=None)
def recon_ref(N, s, pad, iters, fft=R.NumpyFFT, order="real", scale=1.0, from_intensity=False, cs=0.0):
    images, df = R.series(N, s)
    return R.reconstruct(images, scale * df, LAM, PX, cs, iters, pad, from_intensity, fft, order)


def check_wave(got, want, what):
    e = R.rel_l2(got, want)
    print(f"{what}: rel L2 {e:.3e}; bar {wave_bar():.3e} (the two restatements' largest distance {YARD:.3e})")
    assert e <= wave_bar(), what


def yardstick():
    """The largest relative L2 distance between the restatement on numpy.fft and on the radix-2 FFT, over this file's cases (CPU)."""
    worst = 0.0

    def note(what, a, b):
        nonlocal worst
        e = R.rel_l2(a, b)
        print(f"yardstick {what}: {e:.3e}")
        worst = max(worst, e)

    for B, S in FFT_SIZES + [(1, 4096)]:
        z = waves(B, S)
        note(f"fft2 {B}x{S}", R.Radix2FFT.fft2(z), np.fft.fft2(z))
        if S <= 1024:
            note(f"ifft2 {B}x{S}", R.Radix2FFT.ifft2(z), np.fft.ifft2(z))
    for c in PROP_CASES:
        note(f"propagate {c}", prop_ref(*c, fft=R.Radix2FFT), prop_ref(*c))
    for c in RECON_CASES + LARGE_CASES:
        a, b = recon_ref(*c, fft=R.Radix2FFT), recon_ref(*c)
        note(f"reconstruct E {c}", a["E"], b["E"])
        note(f"reconstruct stack {c}", a["stack"], b["stack"])
        if c[2] == 0:
            f = recon_ref(*c, order="freq")
            print(f"  frequency-domain order vs real-space order {c}: E {R.rel_l2(f['E'], b['E']):.3e}, stack "
                  f"{R.rel_l2(f['stack'], b['stack']):.3e}")
        print(f"  min |b| / mean |b| {c}: {b['ratio']:.3f}")
    for c in CS_PROP_CASES:
        note(f"propagate, Cs = {CS}, {c}", prop_ref(*c, fft=R.Radix2FFT, cs=CS), prop_ref(*c, cs=CS))
    for c in CS_RECON_CASES:
        a, b = recon_ref(*c, fft=R.Radix2FFT, cs=CS), recon_ref(*c, cs=CS)
        note(f"reconstruct E, Cs = {CS}, {c}", a["E"], b["E"])
        note(f"reconstruct stack, Cs = {CS}, {c}", a["stack"], b["stack"])
        print(f"  min |b| / mean |b|, Cs = {CS}, {c}: {b['ratio']:.3f}")
    return worst


# ---- fft2 / ifft2 -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", FFT_SIZES, ids=ids)
def test_fft2_and_ifft2(case):
    B, S = case
    z = waves(B, S)
    zd = up(z)
    f, i = exitwave.fft2(zd), exitwave.ifft2(zd)
    assert f.is_cuda and f.dtype == torch.complex128 and tuple(f.shape) == (B, S, S) and tuple(i.shape) == (B, S, S)
    check_wave(f.cpu().numpy(), np.fft.fft2(z), f"fft2 [{B},{S},{S}]")
    check_wave(i.cpu().numpy(), np.fft.ifft2(z), f"ifft2 [{B},{S},{S}]")
    check_wave(exitwave.ifft2(f).cpu().numpy(), z, f"ifft2(fft2(z)) [{B},{S},{S}]")


def test_fft2_4096_forward():
    z = waves(1, 4096)
    check_wave(exitwave.fft2(up(z)).cpu().numpy(), np.fft.fft2(z), "fft2 [1,4096,4096]")


@pytest.mark.parametrize("S", [8, 32, 64, 1024])
def test_impulse_gives_the_phase_ramp_in_both_directions(S):
    x = np.zeros((S, S), np.complex128)
    x[1, 2] = 1.0
    ky, kx = np.arange(S)[:, None], np.arange(S)[None, :]
    ramp = np.exp(-2j * np.pi * ((ky * 1 + kx * 2) % S) / S)
    swapped = np.exp(-2j * np.pi * ((ky * 2 + kx) % S) / S)
    f, i = exitwave.fft2(up(x)).cpu().numpy(), exitwave.ifft2(up(x)).cpu().numpy() * (S * S)
    ef, ei = np.abs(f - ramp).max(), np.abs(i - np.conj(ramp)).max()
    print(f"impulse at (1, 2), S = {S}: forward distance from exp(-2 pi i (ky + 2 kx) / S) {ef:.3e}, inverse from its conjugate {ei:.3e}; "
          f"bound {S * 2.0 ** -52:.3e}")
    assert f.shape == (S, S) and ef <= S * 2.0 ** -52 and ei <= S * 2.0 ** -52
    assert np.abs(f - np.conj(ramp)).max() > 0.5 and np.abs(f - swapped).max() > 0.5
    assert np.abs(i - ramp).max() > 0.5 and np.abs(i - np.conj(swapped)).max() > 0.5


@pytest.mark.parametrize("S", [8, 64, 256])
def test_fft2_of_a_real_image_agrees_with_rfft2(S):
    x = (np.float32(900) * synthetic_lq(2, S, S, seed=300 + 2 * S)[..., 0] - np.float32(40)).astype(np.float32)
    full = exitwave.fft2(up(x)).cpu().numpy()
    half = harvest.rfft2(up(x)).cpu().numpy()
    check_wave(full, np.fft.fft2(x.astype(np.float64)), f"fft2 of a real image {S}")
    check_wave(full[:, :, :S // 2 + 1], half, f"fft2 against harvest.rfft2 on the half spectrum {S}")


# ---- the transfer function ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [8, 64, 256])
@pytest.mark.parametrize("cs", [0.0, 1e-3])
def test_transfer_function(S, cs):
    dfs = [4e-8, -4e-8, 1.3e-7, -2.5e-6]
    got = exitwave.transfer_function(S, LAM, dfs, px=PX, cs=cs)
    assert isinstance(got, np.ndarray) and got.dtype == np.complex128 and got.shape == (4, S, S)
    for g, d in zip(got, dfs):
        want = R.transfer_function(S, LAM, d, PX, cs)
        e = max(np.abs(g.real - want.real).max(), np.abs(g.imag - want.imag).max())
        print(f"H S = {S}, df = {d}, Cs = {cs}: largest component distance {e:.3e}; bar {TF_BAR:.3e}; largest |t| "
              f"{np.abs(R.transfer_phase(S, LAM, d, PX, cs)).max():.3f}")
        assert e <= TF_BAR
        assert g[0, 0] == 1.0 + 0.0j                                        # q = 0
        one = exitwave.transfer_function(S, LAM, d, px=PX, cs=cs)
        assert one.shape == (S, S) and np.array_equal(one, g)
    if cs == 0.0:                                                          # with Cs the phase is not odd in df
        assert np.array_equal(got[1], np.conj(got[0]))                     # H(-df) = conj H(df), bit for bit
    t = exitwave.transfer_function(S, LAM, up(np.array(dfs)), px=PX, cs=cs)
    assert t.is_cuda and np.array_equal(t.cpu().numpy(), got)


# ---- propagate ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", PROP_CASES, ids=ids)
def test_propagate(case):
    B, s, pad = case
    w, df = waves(B, s), prop_defocuses(B)
    assert len(set(df.tolist())) == B                                      # a kernel that reads defocus[0] for every image fails
    got = exitwave.propagate(up(w), df, LAM, px=PX, pad_periods=pad)
    assert got.is_cuda and got.dtype == torch.complex128 and tuple(got.shape) == (B, s, s)
    check_wave(got.cpu().numpy(), prop_ref(B, s, pad), f"propagate {case}")
    for b in range(B):
        check_wave(got[b].cpu().numpy(), prop_ref(B, s, pad)[b], f"propagate {case} image {b}")
    if pad == 0:
        back = exitwave.propagate(got, -df, LAM, px=PX)
        check_wave(back.cpu().numpy(), w, f"P(P(psi, df), -df) {case}")
        same = exitwave.propagate(up(w), 0.0, LAM, px=PX)
        check_wave(same.cpu().numpy(), w, f"P(psi, 0) {case}")
    if s <= 32:                                                            # a real float32 image has a zero imaginary part
        x = w.real.astype(np.float32)
        want = np.stack([R.propagate(x[b].astype(np.float64), df[b], LAM, PX, 0.0, pad) for b in range(B)])
        check_wave(exitwave.propagate(up(x), df, LAM, px=PX, pad_periods=pad).cpu().numpy(), want, f"propagate of float32 {case}")


@pytest.mark.parametrize("case", CS_PROP_CASES, ids=ids)
def test_propagate_with_spherical_aberration(case):
    B, s, pad = case
    w, df = waves(B, s), prop_defocuses(B)
    want = prop_ref(B, s, pad, cs=CS)
    apart = R.rel_l2(prop_ref(B, s, pad), want)
    print(f"propagate {case}: Cs = {CS} moves the restatement by {apart:.3e} from Cs = 0")
    assert apart > 1e3 * wave_bar()                                        # a kernel that drops the Cs term fails by far
    got = exitwave.propagate(up(w), df, LAM, px=PX, cs=CS, pad_periods=pad)
    check_wave(got.cpu().numpy(), want, f"propagate, Cs = {CS}, {case}")


# ---- reconstruct --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", RECON_CASES, ids=ids)
def test_reconstruct(case):
    N, s, pad, iters = case
    images, df = R.series(N, s)
    want = recon_ref(*case)
    print(f"reconstruct {case}: min |b| / mean |b| over the restatement's iterations {want['ratio']:.3f}")
    assert want["ratio"] >= RATIO_MIN                                      # before the GPU is touched
    E, stack = exitwave.reconstruct(up(images), df, LAM, px=PX, iterations=iters, pad_periods=pad, return_stack=True)
    assert E.is_cuda and E.dtype == torch.complex128 and tuple(E.shape) == (s, s) and tuple(stack.shape) == (N, s, s)
    check_wave(E.cpu().numpy(), want["E"], f"E {case}")
    check_wave(stack.cpu().numpy(), want["stack"], f"stack {case}")
    check_wave(stack.abs().cpu().numpy(), np.abs(images.astype(np.float64)), f"|stack| against the amplitudes {case}")
    alone = exitwave.reconstruct(up(images), df, LAM, px=PX, iterations=iters, pad_periods=pad)
    assert torch.equal(bits(alone), bits(E))                               # without the stack: the same exit wave, the same bits
    if pad == 0:
        Ec, sc = exitwave.reconstruct(up(images), df, LAM, px=PX, iterations=iters, return_stack=True, _composed=True)
        check_wave(Ec.cpu().numpy(), want["E"], f"E, composed path {case}")
        check_wave(sc.cpu().numpy(), want["stack"], f"stack, composed path {case}")
        check_wave(E.cpu().numpy(), Ec.cpu().numpy(), f"E, fused against composed {case}")
        check_wave(stack.cpu().numpy(), sc.cpu().numpy(), f"stack, fused against composed {case}")


@pytest.mark.parametrize("case", CS_RECON_CASES, ids=ids)
def test_reconstruct_with_spherical_aberration(case):
    """With Cs != 0 the back-propagation multiplies by H(-df), which is not conj H(df): the restatement with conj H instead is far
    from the restatement (asserted on the CPU), so a kernel that conjugates, or drops the Cs term, fails."""
    N, s, pad, iters = case
    images, df = R.series(N, s)
    want = recon_ref(*case, cs=CS)
    print(f"reconstruct, Cs = {CS}, {case}: min |b| / mean |b| {want['ratio']:.3f}")
    assert want["ratio"] >= RATIO_MIN
    S = s * (1 + pad)
    conj = np.stack([R.propagate(images[k].astype(np.float64), -df[k], LAM, PX, -CS, pad) for k in range(N)]).mean(0)   # conj H(df) = H(-df; -Cs)
    first = recon_ref(N, s, pad, 1, cs=CS)["E"]
    apart = min(R.rel_l2(conj, first), R.rel_l2(recon_ref(*case)["E"], want["E"]))
    print(f"  conj H(df) for H(-df) moves the first exit wave, and Cs = 0 the last, by at least {apart:.3e} (S = {S})")
    assert apart > 1e3 * wave_bar()
    E, stack = exitwave.reconstruct(up(images), df, LAM, px=PX, cs=CS, iterations=iters, pad_periods=pad, return_stack=True)
    check_wave(E.cpu().numpy(), want["E"], f"E, Cs = {CS}, {case}")
    check_wave(stack.cpu().numpy(), want["stack"], f"stack, Cs = {CS}, {case}")
    if pad == 0:
        Ec, sc = exitwave.reconstruct(up(images), df, LAM, px=PX, cs=CS, iterations=iters, return_stack=True, _composed=True)
        check_wave(Ec.cpu().numpy(), want["E"], f"E, composed path, Cs = {CS}, {case}")
        check_wave(sc.cpu().numpy(), want["stack"], f"stack, composed path, Cs = {CS}, {case}")


@pytest.mark.parametrize("case", LARGE_CASES, ids=ids)
def test_reconstruct_with_several_elements_per_thread(case):
    """S = 512 and 1024: the column kernel's instances with 2 and 4 accumulators per thread."""
    N, s, _, iters = case
    images, df = R.series(N, s)
    want = recon_ref(*case)
    print(f"reconstruct {case}: min |b| / mean |b| {want['ratio']:.3f}")
    assert want["ratio"] >= RATIO_MIN
    E, stack = exitwave.reconstruct(up(images), df, LAM, px=PX, iterations=iters, return_stack=True)
    check_wave(E.cpu().numpy(), want["E"], f"E {case}")
    check_wave(stack.cpu().numpy(), want["stack"], f"stack {case}")


@pytest.mark.parametrize("s", [2048, 4096])
def test_reconstruct_of_one_large_image(s):
    """S = 2048 and 4096: the column kernel's instances with 8 and 16 accumulators per thread, and the 64 KiB line.  One image, two
    iterations: b = P(P(image, -df), df) is the image itself (positive, so min |b| / mean |b| >= 0.9 without a restatement), hence
    psi = image and E = P(image, -df) in both iterations, each within the waves' bar.  Compared on the device, in double."""
    rng = np.random.default_rng(s)
    image = up((1.0 + 0.1 * (rng.random((1, s, s)) - 0.5)).astype(np.float32))
    d = up(np.array([4e-8]))
    rel = lambda a, b: float(torch.linalg.norm((a - b).reshape(-1)) / torch.linalg.norm(b.reshape(-1)))
    E, stack = exitwave.reconstruct(image, d, LAM, px=PX, iterations=2, return_stack=True)
    es = rel(stack, image.to(torch.complex128))
    print(f"one image of {s}: stack against the image, rel L2 {es:.3e}; bar {wave_bar():.3e}")
    assert es <= wave_bar()
    del stack
    Ec = exitwave.reconstruct(image, d, LAM, px=PX, iterations=2, _composed=True)
    ee = rel(E, Ec)
    print(f"one image of {s}: E, fused against composed, rel L2 {ee:.3e}; bar {wave_bar():.3e}")
    assert ee <= wave_bar()
    back = exitwave.propagate(E, d, LAM, px=PX)                            # P(E, +df) is the image again
    eb = rel(back, image.to(torch.complex128))
    print(f"one image of {s}: P(E, df) against the image, rel L2 {eb:.3e}; bar {wave_bar():.3e}")
    assert eb <= wave_bar()


def test_one_iteration_of_one_image_is_a_propagation():
    images, df = R.series(1, 8)
    E = exitwave.reconstruct(up(images), df, LAM, px=PX, iterations=1)
    P = exitwave.propagate(up(images), -df, LAM, px=PX)[0]
    check_wave(E.cpu().numpy(), P.cpu().numpy(), "reconstruct(N = 1, iterations = 1) against propagate(image, -df)")


@pytest.mark.parametrize("pad", [0, 1])
def test_from_intensity_on_squared_images(pad):
    images, df = R.series(3, 16)
    q = np.round(images * 2048.0) / 2048.0                                  # 12 significant bits: the square is exact in float32
    q = q.astype(np.float32)
    sq = (q * q).astype(np.float32)
    assert np.array_equal(np.sqrt(sq.astype(np.float64)), q.astype(np.float64)) and (q > 0).all()
    want = R.reconstruct(q, df, LAM, PX, 0.0, 5, pad)
    assert want["ratio"] >= RATIO_MIN
    plain = exitwave.reconstruct(up(q), df, LAM, px=PX, iterations=5, pad_periods=pad, return_stack=True)
    fi = exitwave.reconstruct(up(sq), df, LAM, px=PX, iterations=5, pad_periods=pad, return_stack=True, from_intensity=True)
    for name, a, b, w in (("E", fi[0], plain[0], want["E"]), ("stack", fi[1], plain[1], want["stack"])):
        check_wave(a.cpu().numpy(), w, f"from_intensity {name}, pad {pad}")
        check_wave(a.cpu().numpy(), b.cpu().numpy(), f"from_intensity {name} against the plain run, pad {pad}")


# ---- losses and the sweep -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pad", [0, 1])
def test_losses(pad):
    images, df = R.series(3, 32)
    want = recon_ref(3, 32, pad, 5, scale=1.5)
    print(f"losses, pad {pad}: kappa {want['kappa']}, min |b| / mean |b| {want['ratio']:.3f}")
    assert want["kappa"].max() <= KAPPA_MAX and want["ratio"] >= RATIO_MIN
    E, losses = exitwave.reconstruct(up(images), 1.5 * df, LAM, px=PX, iterations=5, pad_periods=pad, return_losses=True)
    got = losses.cpu().numpy()
    check_wave(E.cpu().numpy(), want["E"], f"E of the loss run, pad {pad}")
    for k in range(3):
        e = abs(got[k] - want["losses"][k]) / want["losses"][k]
        print(f"  loss[{k}] = {got[k]!r} (numpy {want['losses'][k]!r}): relative distance {e:.3e}; bar {loss_bar(want['kappa'][k]):.3e}")
        assert e <= loss_bar(want["kappa"][k])
    worst = exitwave.reconstruction_loss(up(images), 1.5 * df, LAM, px=PX, iterations=5, pad_periods=pad)
    assert float(worst) == got.max()
    if pad == 0:
        lc = exitwave.reconstruction_loss(up(images), 1.5 * df, LAM, per_image=True, px=PX, iterations=5, _composed=True).cpu().numpy()
        for k in range(3):
            assert abs(lc[k] - want["losses"][k]) / want["losses"][k] <= loss_bar(want["kappa"][k])


@pytest.mark.parametrize("sweep", SWEEPS, ids=lambda s: s[0])
def test_defocus_sweep_finds_the_true_increment(sweep):
    name, x, incs, fi = sweep
    images, df = R.series(3, 32)
    images = x(images)
    ramp = df / 1e-8                                                       # the true increment is 1e-8
    refs = [R.reconstruct(images, i * ramp, LAM, PX, 0.0, 5, from_intensity=fi) for i in incs]
    for r in refs:
        assert r["kappa"].max() <= KAPPA_MAX and r["ratio"] >= RATIO_MIN
    want = np.array([r["losses"].max() for r in refs])
    assert int(np.argmin(want)) == 2 and incs[2] == 1e-8                   # the restatement, before the GPU is touched
    got = exitwave.defocus_sweep(images, LAM, incs, ramp, px=PX, iterations=5, from_intensity=fi)
    assert isinstance(got, np.ndarray) and got.shape == (5,)
    for i, r in enumerate(refs):
        k = int(np.argmax(r["losses"]))
        e = abs(got[i] - want[i]) / want[i]
        print(f"sweep of {name} images, increment {incs[i]:.2e}: loss {got[i]!r} (numpy {want[i]!r}); relative distance {e:.3e}; bar "
              f"{loss_bar(r['kappa'][k]):.3e}")
        assert e <= loss_bar(r["kappa"][k])
    assert int(np.argmin(got)) == 2
    t = exitwave.defocus_sweep(up(images), LAM, incs, ramp, px=PX, iterations=5, from_intensity=fi)
    assert t.is_cuda and np.array_equal(t.cpu().numpy(), got)


# ---- conventions, bits and safety ---------------------------------------------------------------------------------------------------

def test_numpy_and_tensor_conventions():
    z = waves(2, 16)
    images, df = R.series(3, 16)
    for a in (z, z[0]):
        keep = a.copy()
        for fn in (exitwave.fft2, exitwave.ifft2, lambda v: exitwave.propagate(v, 2e-8, LAM, px=PX)):
            n, t = fn(a), fn(up(a))
            assert isinstance(n, np.ndarray) and n.dtype == np.complex128 and n.shape == a.shape and np.array_equal(a, keep)
            assert isinstance(t, torch.Tensor) and t.is_cuda and tuple(t.shape) == a.shape and np.array_equal(n, t.cpu().numpy())
    n = exitwave.reconstruct(images, df, LAM, px=PX, iterations=2, return_stack=True, return_losses=True)
    t = exitwave.reconstruct(up(images), up(df), LAM, px=PX, iterations=2, return_stack=True, return_losses=True)
    assert len(n) == 3 and [v.shape for v in n] == [(16, 16), (3, 16, 16), (3,)] and n[2].dtype == np.float64
    assert all(isinstance(v, np.ndarray) for v in n) and all(v.is_cuda for v in t)
    assert all(np.array_equal(a, b.cpu().numpy()) for a, b in zip(n, t))
    assert isinstance(exitwave.reconstruction_loss(images, df, LAM, px=PX, iterations=2), float)


def test_bitwise_reproducible():
    images, df = R.series(3, 64)
    for kw in ({}, {"_composed": True}, {"pad_periods": 1}):
        run = lambda: exitwave.reconstruct(up(images), df, LAM, px=PX, iterations=3, return_stack=True, return_losses=True, **kw)
        a, b = run(), run()
        assert all(torch.equal(bits(p), bits(q)) for p, q in zip(a, b)), kw
        assert not any(torch.isnan(bits(p)).any() for p in a)
    w = up(waves(2, 64))
    assert torch.equal(bits(exitwave.propagate(w, 3e-8, LAM, px=PX)), bits(exitwave.propagate(w, 3e-8, LAM, px=PX)))
    assert torch.equal(bits(exitwave.fft2(w)), bits(exitwave.fft2(w)))


class Guarded:
    """`nbytes` bytes, 256-byte aligned, inside a sentinel-filled buffer with 4 KiB of guard on either side."""
    GUARD = 1024   # floats

    def __init__(self, nbytes, fill=SENTINEL):
        self.n = (nbytes + 3) // 4
        self.buf = torch.full((self.n + 2 * self.GUARD + 64,), SENTINEL, dtype=torch.float32, device=dev())
        self.off = self.GUARD + (-(self.buf.data_ptr() // 4 + self.GUARD)) % 64
        self.view = self.buf[self.off:self.off + self.n]
        self.view.fill_(fill)
        assert self.view.data_ptr() % 256 == 0

    def ptr(self):
        return C.c_void_p(self.view.data_ptr())

    def intact(self):
        return bool((self.buf[:self.off] == SENTINEL).all()) and bool((self.buf[self.off + self.n:] == SENTINEL).all())

    def bits(self):
        return self.view.view(torch.int32)                                 # halves of doubles are not compared as float32: some are NaN

    def f64(self):
        return self.view.view(torch.float64)

    def complex(self, *shape):
        return torch.view_as_complex(self.view.view(torch.float64).reshape(*shape, 2))


@contextlib.contextmanager
def composed_path(on):
    """The development knob that sends pad_periods == 0 through the composed path (include/emdenoise_dev.h); back to 0 afterwards."""
    _lib.knob(exitwave.COMPOSED_KNOB, int(on))
    try:
        yield
    finally:
        _lib.knob(exitwave.COMPOSED_KNOB, 0)


def recon_bytes(lib, N, s, pad, composed):
    with composed_path(composed):
        return lib.emd_exitwave_workspace_bytes(N, s, pad)


def c_reconstruct(lib, x, d, N, s, pad, iters, composed, ws, nbytes, want_stack=True, want_losses=True):
    E, stack, losses = Guarded(s * s * 16), Guarded(N * s * s * 16), Guarded(N * 8)
    with composed_path(composed):
        rc = lib.emd_exitwave_reconstruct_f64(x.data_ptr(), N, s, pad, d.data_ptr(), LAM, PX, 0.0, iters, 0, E.ptr(),
                                              stack.ptr() if want_stack else None, losses.ptr() if want_losses else None, ws.ptr(),
                                              nbytes, _lib.stream_ptr())
    _lib.check(rc, "reconstruct")
    torch.cuda.synchronize()
    return E, stack, losses


def test_outputs_and_workspace_stay_inside_their_advertised_sizes():
    lib = _lib.load()
    st = _lib.stream_ptr()
    for B, S in ((2, 8), (3, 32), (2, 128)):
        z = up(waves(3, S)[:B])
        nbytes = lib.emd_cfft2_workspace_bytes(B, S)
        for inverse in (0, 1):
            out, ws = Guarded(B * S * S * 16), Guarded(nbytes)
            _lib.check(lib.emd_cfft2_f64(z.data_ptr(), B, S, inverse, out.ptr(), ws.ptr(), nbytes, st), "cfft2")
            torch.cuda.synchronize()
            assert out.intact() and ws.intact(), f"cfft2 {B} x {S} wrote outside its output or its {nbytes}-byte workspace"
            assert torch.equal(bits(out.complex(B, S, S)), bits(exitwave.ifft2(z) if inverse else exitwave.fft2(z)))
    for B, s, pad in ((2, 8, 0), (3, 32, 1), (2, 16, 3), (2, 128, 0)):
        w, d = up(waves(3, s)[:B]), up(prop_defocuses(B))
        nbytes = lib.emd_propagate_workspace_bytes(B, s, pad)
        out, ws = Guarded(B * s * s * 16), Guarded(nbytes)
        _lib.check(lib.emd_propagate_f64(w.data_ptr(), 0, B, s, pad, d.data_ptr(), LAM, PX, 0.0, out.ptr(), ws.ptr(), nbytes, st), "propagate")
        torch.cuda.synchronize()
        assert out.intact() and ws.intact(), f"propagate {B} x {s} pad {pad} wrote outside its output or its {nbytes}-byte workspace"
        assert torch.equal(bits(out.complex(B, s, s)), bits(exitwave.propagate(w, d, LAM, px=PX, pad_periods=pad)))
    for n, S in ((1, 8), (3, 32), (2, 128)):
        d = up(prop_defocuses(n))
        H = Guarded(n * S * S * 16)
        _lib.check(lib.emd_transfer_function_f64(S, n, d.data_ptr(), LAM, PX, CS, H.ptr(), st), "transfer_function")
        torch.cuda.synchronize()
        assert H.intact(), f"transfer_function {n} x {S} wrote outside [n][S][S][2]"
        assert torch.equal(bits(H.complex(n, S, S)), bits(exitwave.transfer_function(S, LAM, d, px=PX, cs=CS)))
    for N, s, pad, flags in ((2, 8, 0, False), (3, 32, 0, False), (3, 32, 0, True), (2, 16, 1, False), (3, 8, 3, False)):
        images, df = R.series(N, s)
        x, d = up(images), up(df)
        nbytes = recon_bytes(lib, N, s, pad, flags)
        ws = Guarded(nbytes)
        E, stack, losses = c_reconstruct(lib, x, d, N, s, pad, 2, flags, ws, nbytes)
        what = f"reconstruct {N} x {s} pad {pad} composed {flags}"
        assert E.intact() and stack.intact() and losses.intact() and ws.intact(), f"{what} wrote outside an output or its {nbytes}-byte workspace"
        want = exitwave.reconstruct(x, d, LAM, px=PX, iterations=2, pad_periods=pad, return_stack=True, return_losses=True,
                                    _composed=bool(flags))
        assert torch.equal(bits(E.complex(s, s)), bits(want[0])) and torch.equal(bits(stack.complex(N, s, s)), bits(want[1])), what
        assert torch.equal(losses.f64(), want[2]), what
        E2, stack2, losses2 = c_reconstruct(lib, x, d, N, s, pad, 2, flags, Guarded(nbytes), nbytes, want_stack=False, want_losses=False)
        assert torch.equal(E2.bits(), E.bits()) and bool((stack2.view == SENTINEL).all()) and bool((losses2.view == SENTINEL).all()), what


def test_a_stack_alone_equals_itself_after_other_calls_on_the_same_workspace():
    lib = _lib.load()
    cases = [(3, 32, 0, False), (2, 16, 1, False), (3, 32, 0, True), (5, 16, 0, False)]
    nbytes = max(recon_bytes(lib, N, s, pad, f) for N, s, pad, f in cases)
    ws = Guarded(nbytes, fill=float("nan"))                                # whatever a call reads, it has written itself
    first = []
    for N, s, pad, f in cases + cases[::-1]:
        images, df = R.series(N, s)
        E, stack, losses = c_reconstruct(lib, up(images), up(df), N, s, pad, 3, f, ws, nbytes)
        assert not torch.isnan(E.f64()).any() and not torch.isnan(stack.f64()).any() and not torch.isnan(losses.f64()).any()
        first.append((E.bits().clone(), stack.bits().clone(), losses.bits().clone()))
    for a, b in zip(first[:len(cases)], first[:len(cases) - 1:-1]):
        assert all(torch.equal(p, q) for p, q in zip(a, b))


def test_captured_in_one_graph_and_replayed_on_new_contents_and_new_defocuses():
    images, df = R.series(3, 32)
    x0, d0 = up(images), up(df)
    x1, d1 = up(images[::-1].copy() * np.float32(0.75)), up(df[::-1].copy() * 1.25)

    def run(x, d):
        E, stack, losses = exitwave.reconstruct(x, d, LAM, px=PX, iterations=3, return_stack=True, return_losses=True)
        Ep = exitwave.reconstruct(x, d, LAM, px=PX, iterations=2, pad_periods=1)
        return bits(exitwave.propagate(x, d, LAM, px=PX, pad_periods=1)), bits(E), bits(stack), losses, bits(Ep)

    want0, want1 = run(x0, d0), run(x1, d1)                                # eager
    sx, sd = x0.clone(), d0.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = run(sx, sd)
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs, want0))
    sx.copy_(x1)
    sd.copy_(d1)
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs, want1))
    assert not torch.equal(want0[1], want1[1])


if __name__ == "__main__":
    y = yardstick()
    print(f"waves: the two float64 restatements' largest distance {y:.3e}; bar {FACTOR * y:.3e}")
    for pad in (0, 1):
        r = recon_ref(3, 32, pad, 5, scale=1.5)
        print(f"loss run pad {pad}: kappa {r['kappa']}, losses {r['losses']}, ratio {r['ratio']:.3f}")
