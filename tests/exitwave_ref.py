"""The float64 numpy restatement of the focal-series reconstruction (emdenoise.exitwave; include/emdenoise.h "Exit-wave
reconstruction"), written from ewrec_class.py:100-110 and :272-380 in the REFERENCE's order -- a real-space mean and two full
propagations per image per iteration -- and independent of the library.  ArrayFire is not needed; the reference does not run as
committed, so the formulas are the specification.

Two FFT back ends evaluate the same formulas: ``numpy.fft`` and the plain recursive radix-2 transform of tests/fft_ref.py; their
distance is the yardstick of the waves' bar (tests/test_exitwave_gpu.py).  ``order="freq"`` (pad_periods = 0) restates the iteration in
the frequency domain, as the device's fused path runs it."""
import functools

import numpy as np

from tests import fft_ref
from tests.synth_inputs import synthetic_lq

WAVELENGTH, PX = 2.51e-12, 1e-10


class NumpyFFT:
    fft2 = staticmethod(np.fft.fft2)
    ifft2 = staticmethod(np.fft.ifft2)


class Radix2FFT:
    @staticmethod
    def fft2(z):
        return fft_ref.fft_radix2(fft_ref.fft_radix2(np.asarray(z, np.complex128)).swapaxes(-1, -2)).swapaxes(-1, -2)

    @staticmethod
    def ifft2(z):
        z = np.asarray(z, np.complex128)
        return np.conj(Radix2FFT.fft2(np.conj(z))) / float(z.shape[-1] * z.shape[-2])


def transfer_phase(S, wavelength, defocus, px=1.0, cs=0.0):
    """t [S,S] in FFT order, every operation in the order of include/emdenoise.h."""
    j = np.arange(S)
    q = np.where(j < S // 2, j, j - S).astype(np.float64) / (float(S) * px)
    qy, qx = q[:, None], q[None, :]
    q2 = qy * qy + qx * qx
    lam3 = wavelength * wavelength * wavelength
    return wavelength * defocus * q2 + 0.5 * lam3 * cs * q2 * q2


def transfer_function(S, wavelength, defocus, px=1.0, cs=0.0):
    """H = exp(i pi t); t is reduced by fmod(t, 2) (exact) before it meets pi."""
    r = np.fmod(transfer_phase(S, wavelength, float(defocus), px, cs), 2.0)
    return np.cos(np.pi * r) + 1j * np.sin(np.pi * r)


def propagate(psi, defocus, wavelength, px=1.0, cs=0.0, pad_periods=0, fft=NumpyFFT):
    """One wave [s,s] -> ifft2(fft2(pad) H)[:s, :s]."""
    s = psi.shape[-1]
    S = s * (1 + pad_periods)
    padded = np.zeros((S, S), np.complex128)
    padded[:s, :s] = psi
    return fft.ifft2(fft.fft2(padded) * transfer_function(S, wavelength, defocus, px, cs))[:s, :s]


def amplitudes(images, from_intensity=False):
    x = np.asarray(images, np.float64)
    return np.sqrt(np.maximum(x, 0.0)) if from_intensity else np.abs(x)


def losses_of(images, b):
    """loss_k = mean((image_k - c I)^2), I = |b_k|^2, c = mean(image_k) / mean(I); also kappa_k = sum image^2 / sum (image - c I)^2."""
    out, kappa = [], []
    for img, bk in zip(np.asarray(images, np.float64), b):
        inten = bk.real * bk.real + bk.imag * bk.imag
        c = img.mean() / inten.mean()
        r = (img - c * inten) ** 2
        out.append(r.mean())
        kappa.append((img ** 2).sum() / r.sum())
    return np.array(out), np.array(kappa)


def reconstruct(images, defocuses, wavelength, px=1.0, cs=0.0, iterations=50, pad_periods=0, from_intensity=False, fft=NumpyFFT,
                order="real"):
    """-> dict(E [s,s], stack [N,s,s], b [N,s,s] (the last iteration's), losses [N], kappa [N], ratio: the smallest
    min|b_k| / mean|b_k| over all images and iterations)."""
    images = np.asarray(images, np.float32)
    N, s = images.shape[0], images.shape[-1]
    a = amplitudes(images, from_intensity)
    psi = [(a[k] if from_intensity else images[k]).astype(np.complex128) for k in range(N)]
    ratio = np.inf
    if order == "freq":
        assert pad_periods == 0
        Hm = [transfer_function(s, wavelength, -defocuses[k], px, cs) for k in range(N)]
        Hp = [transfer_function(s, wavelength, defocuses[k], px, cs) for k in range(N)]
    for _ in range(iterations):
        if order == "freq":
            Eh = 0
            for k in range(N):
                Eh = Eh + fft.fft2(psi[k]) * Hm[k]
            Eh = Eh / N
            E = fft.ifft2(Eh)
            b = [fft.ifft2(Eh * Hp[k]) for k in range(N)]
        else:
            E = 0
            for k in range(N):
                E = E + propagate(psi[k], -defocuses[k], wavelength, px, cs, pad_periods, fft)
            E = E / N
            b = [propagate(E, defocuses[k], wavelength, px, cs, pad_periods, fft) for k in range(N)]
        for k in range(N):
            m = np.abs(b[k])
            ratio = min(ratio, float(m.min() / m.mean()))
            with np.errstate(invalid="ignore", divide="ignore"):
                psi[k] = np.where(m > 0, a[k] * b[k] / m, a[k])
    losses, kappa = losses_of(images, b)
    return {"E": E, "stack": np.stack(psi), "b": np.stack(b), "losses": losses, "kappa": kappa, "ratio": ratio}


def focal_ramp(n, series_type="cubic", middle=None, alternating=True, increasing=True):
    """ewrec_class.py:387-404, as it is written there."""
    if series_type == "linear":
        gen = lambda x: x
    elif series_type == "quadratic":
        gen = lambda x: x ** 2
    elif series_type == "cubic":
        gen = lambda x: x ** 3
    mid = (middle if middle else n // 2) if alternating else 0
    defocus_dir = 1.0 if increasing else -1.0
    return np.array([defocus_dir * np.sign(x - mid) * gen(x - mid) for x in range(n)], np.float64)


# ---- the simulated series of the tests ----------------------------------------------------------------------------------------

def series_defocuses(N):
    k = np.arange(N, dtype=np.float64) - N // 2
    return 2e-8 * np.sign(k) * k ** 2 + 1e-8


@functools.lru_cache(maxsize=None)
def true_wave(s):
    u, v = synthetic_lq(2, s, s, seed=700 + s)[..., 0].astype(np.float64)
    return (1.0 + 0.1 * (u - u.mean())) * np.exp(0.3j * (v - v.mean()))


@functools.lru_cache(maxsize=None)
def series(N, s):
    """Images = |P(wave, df_k)| as float32 [N,s,s] and their defocuses.  Cached: do not write into the result."""
    df = series_defocuses(N)
    w = true_wave(s)
    return np.stack([np.abs(propagate(w, d, WAVELENGTH, PX)) for d in df]).astype(np.float32), df


def rel_l2(a, b):
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))
