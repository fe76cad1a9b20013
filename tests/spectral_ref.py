"""The float64 numpy restatement of the 2-D FFT of any side (emdenoise.spectral; include/emdenoise.h "2-D FFT of any side"), operation
by operation and independent of the library: the line length, the chirp with its phase reduced in integers, Bluestein's line on two
power-of-two transforms (the plain recursive radix-2 FFT of tests/fft_ref.py), the 2-D order (rows, then columns; the inverse by
conjugation with one division per axis), the real-input transform and the propagation between a forward and an inverse transform.

Also here: the direct 2-D DFT and the spectrum of a unit impulse in ``numpy.longdouble`` with integer-reduced phases, for small sides,
and the transfer function with its phase formed in ``longdouble``.  The distance between the restatement and ``numpy.fft`` is the
yardstick of the device's bar (tests/test_spectral.py computes it, tests/test_spectral_gpu.py holds the constants)."""
import functools

import numpy as np

from tests import fft_ref

LD, CLD = np.longdouble, np.clongdouble
PI_LD = np.arccos(LD(-1))
CHUNK = 128   # lines transformed at a time: the temporaries of a chunk stay in the cache


def line_length(n):
    """emd_fft_any_line: n for a power of two 8..4096; max(8, the smallest power of two >= 2 n - 1) for any other n in 2..2048; else 0."""
    if 8 <= n <= 4096 and n & (n - 1) == 0:
        return n
    if not 2 <= n <= 2048:
        return 0
    M = 8
    while M < 2 * n - 1:
        M <<= 1
    return M


def is_plain(n):
    return line_length(n) == n


def cis_turns(num, den):
    """exp(-i pi num / den) for integer arrays 0 <= num < 2 den, in float64, the angle folded in integers into [0, pi / 2] before it
    meets pi: (cos, -sin) of pi num / den."""
    num = np.asarray(num, np.int64)
    half = num >= den                      # + pi: both change sign
    u = np.where(half, num - den, num)     # [0, den)
    fold = 2 * u > den                     # pi - x: the cosine changes sign
    v = np.where(fold, den - u, u)         # [0, den / 2]
    ang = np.pi * (v.astype(np.float64) / float(den))
    c, s = np.cos(ang), np.sin(ang)
    c = np.where(fold, -c, c)
    sign = np.where(half, -1.0, 1.0)
    return sign * c - 1j * (sign * s)


@functools.lru_cache(maxsize=None)
def chirp(n):
    """w[k] = exp(-i pi k^2 / n), k < n, through t = k^2 mod 2 n in integers.  Cached: do not write into the result."""
    k = np.arange(n, dtype=np.int64)
    return cis_turns((k * k) % (2 * n), n)


@functools.lru_cache(maxsize=None)
def filter_spectrum(n):
    """Bf = FFT_M(b): b[j] = conj w[j] for j < n, b[M - j] = conj w[j] for 1 <= j < n, 0 elsewhere.  Cached."""
    M, w = line_length(n), chirp(n)
    b = np.zeros(M, np.complex128)
    b[:n] = np.conj(w)
    b[M - np.arange(1, n)] = np.conj(w[1:])
    return fft_ref.fft_radix2(b)


def bluestein_line(x):
    """Forward, unnormalised DFT along the last axis (any length 2..2048) by the chirp-z algorithm, as the device runs it."""
    x = np.asarray(x, np.complex128)
    n = x.shape[-1]
    M, w, Bf = line_length(n), chirp(n), filter_spectrum(n)
    a = np.zeros(x.shape[:-1] + (M,), np.complex128)
    a[..., :n] = x * w
    c = np.conj(fft_ref.fft_radix2(a) * Bf)
    d = np.conj(fft_ref.fft_radix2(c)) * (1.0 / M)      # IFFT_M by conjugation, 1 / M exact
    return d[..., :n] * w


def line_dft(x):
    """Forward, unnormalised DFT along the last axis: the plain power-of-two line, or Bluestein's; in chunks of lines."""
    x = np.asarray(x, np.complex128)
    n = x.shape[-1]
    assert line_length(n), n
    one = fft_ref.fft_radix2 if is_plain(n) else bluestein_line
    flat = x.reshape(-1, n)
    out = np.empty_like(flat)
    for i in range(0, flat.shape[0], CHUNK):
        out[i:i + CHUNK] = one(flat[i:i + CHUNK])
    return out.reshape(x.shape)


def line_idft(y):
    """x = conj(F(conj y)) / n, one division per component."""
    return np.conj(line_dft(np.conj(y))) / float(np.shape(y)[-1])


def _t(z):
    return np.ascontiguousarray(np.swapaxes(z, -1, -2))


def fft2(z):
    """Lines along W, transposed, lines along H, transposed again."""
    return _t(line_dft(_t(line_dft(z))))


def ifft2(z):
    return _t(line_idft(_t(line_idft(z))))


def rfft2(x):
    """Every real (float32) row as a complex line of which W // 2 + 1 elements are kept, then the columns."""
    x = np.asarray(x, np.float32).astype(np.float64)
    K = x.shape[-1] // 2 + 1
    return _t(line_dft(_t(line_dft(x)[..., :K])))


def fftfreq_index(n):
    """j = i below (n + 1) // 2, else i - n: numpy.fft.fftfreq's numerators."""
    i = np.arange(n)
    return np.where(i < (n + 1) // 2, i, i - n)


def transfer_phase(H, W, wavelength, defocus, px=1.0, cs=0.0, dtype=np.float64):
    """t [H,W] in FFT order, every operation in the order of include/emdenoise.h, in ``dtype``."""
    f = dtype
    qy = (fftfreq_index(H).astype(f) / (f(H) * f(px)))[:, None]
    qx = (fftfreq_index(W).astype(f) / (f(W) * f(px)))[None, :]
    q2 = qy * qy + qx * qx
    lam = f(wavelength)
    return lam * f(defocus) * q2 + f(0.5) * (lam * lam * lam) * f(cs) * q2 * q2


def transfer_function(H, W, wavelength, defocus, px=1.0, cs=0.0, dtype=np.float64):
    """Hf = exp(i pi t), complex128; t is reduced by fmod(t, 2) (exact) before it meets pi.  dtype=longdouble: the phase, its reduction
    and the sine and cosine in long double, rounded to double at the end."""
    r = np.fmod(transfer_phase(H, W, wavelength, float(defocus), px, cs, dtype), dtype(2))
    pi = PI_LD if dtype is LD else np.pi
    return (np.cos(pi * r)).astype(np.float64) + 1j * (np.sin(pi * r)).astype(np.float64)


def spectrum_along_rows_then_columns(psi):
    """The first half of propagate, [kx][ky] (transposed): rows forward, transposed, columns forward."""
    return line_dft(_t(line_dft(psi)))


def propagate_from(spec_t, defocus, wavelength, px=1.0, cs=0.0, dtype=np.float64):
    """The second half: times Hf, columns inverse, transposed, rows inverse.  spec_t [W][H] of one wave."""
    W, H = spec_t.shape
    Hf = transfer_function(H, W, wavelength, defocus, px, cs, dtype)
    return line_idft(_t(line_idft(spec_t * Hf.T)))


def propagate(psi, defocus, wavelength, px=1.0, cs=0.0, dtype=np.float64):
    """One wave [H,W] -> ifft2(fft2(psi) Hf), in the device's order."""
    return propagate_from(spectrum_along_rows_then_columns(np.asarray(psi, np.complex128)), defocus, wavelength, px, cs, dtype)


# ---- long double, integer-reduced phases ------------------------------------------------------------------------------------

def _dft_matrix(n):
    kj = (np.arange(n, dtype=np.int64)[:, None] * np.arange(n, dtype=np.int64)[None, :]) % n
    ang = -(LD(2) * PI_LD) * kj.astype(LD) / LD(n)
    return np.cos(ang) + 1j * np.sin(ang)


def dft2_longdouble(z):
    """The direct 2-D DFT of [H,W] in numpy.clongdouble: E_H z E_W^T with E_n[k, j] = exp(-2 pi i ((k j) mod n) / n)."""
    z = np.asarray(z, CLD)
    return _dft_matrix(z.shape[0]) @ z @ _dft_matrix(z.shape[1]).T


def impulse_spectrum(H, W, y0, x0):
    """fft2 of the unit impulse at (y0, x0), exp(-2 pi i (ky y0 / H + kx x0 / W)), in clongdouble: the phase's numerator
    (ky y0 W + kx x0 H) mod (H W) in integers."""
    ky, kx = np.arange(H, dtype=np.int64)[:, None], np.arange(W, dtype=np.int64)[None, :]
    num = (ky * y0 * W + kx * x0 * H) % (H * W)
    ang = -(LD(2) * PI_LD) * num.astype(LD) / LD(H * W)
    return np.cos(ang) + 1j * np.sin(ang)


# ---- inputs and distances ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def noise(B, H, W, seed=0):
    """Seeded white noise, complex128 [B,H,W].  Cached: do not write into the result."""
    rng = np.random.default_rng([seed, B, H, W])
    return rng.standard_normal((B, H, W)) + 1j * rng.standard_normal((B, H, W))


def rel_l2(a, b):
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    return float(np.linalg.norm(a - b) / max(float(np.linalg.norm(b)), 1e-300))
