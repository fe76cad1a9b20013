"""The numpy restatement of the harvester's frequency fields (emdenoise.harvest.rfft2 / radial_profile / freq_stats;
include/emdenoise.h "The 2-D FFT and the radial frequency profile"), written from DM3stoTIFs-batch/img_params.m:53-77 and
independent of the library: ``fft2(double(x))``, the radial profile of ``|fftshift(.)|`` with the reference's bins and its
last-visited-pixel ``radialFreqs``, and the four moments.  float64 throughout.  MATLAB itself is not available.

Also here: a plain recursive radix-2 FFT in float64 and a direct DFT in ``numpy.longdouble``, whose distance is the yardstick of the
spectrum's bar (tests/test_fft_gpu.py)."""
import functools
import math

import numpy as np

FREQ_NAMES = ["mean", "std", "skewness", "kurtosis"]


def valid_sizes():
    return [8 << i for i in range(10)]   # 8 .. 4096


def radial_bins(S):
    """R = ceil(sqrt(mid^2 + mid^2)), mid = S / 2 + 1, in integers: the smallest r with r^2 >= 2 mid^2."""
    n = 2 * (S // 2 + 1) ** 2
    r = math.isqrt(n)
    return r if r * r == n else r + 1


def ceil_sqrt(n):
    """ceil(sqrt(n)) of an integer array, exactly: the smallest integer r with r^2 >= n."""
    n = np.asarray(n, np.int64)
    r = np.floor(np.sqrt(n.astype(np.float64))).astype(np.int64)
    r = np.where(r * r > n, r - 1, r)
    r = np.where((r + 1) * (r + 1) <= n, r + 1, r)          # r = floor(sqrt(n))
    return np.where(r * r == n, r, r + 1)


def shifted_magnitude(x):
    return np.abs(np.fft.fftshift(np.fft.fft2(np.asarray(x, np.float64))))


def profile_loop(mag):
    """img_params.m:59-69, literally: col outer, row inner, 1-based.  -> (radialProfile, radialFreqs), 0-based arrays of R."""
    S = mag.shape[0]
    mid = S // 2 + 1
    R = math.ceil(math.sqrt(mid ** 2 + mid ** 2))
    prof, freqs = np.zeros(R), np.zeros(R)
    for col in range(1, S + 1):
        for row in range(1, S + 1):
            radius = math.sqrt((row - mid) ** 2 + (col - mid) ** 2)
            this = math.ceil(radius) + 1
            prof[this - 1] += mag[row - 1, col - 1]
            freqs[this - 1] = radius / R
    return prof, freqs


def geometry(S):
    """(bin [S,S] 0-based, n = (row - mid)^2 + (col - mid)^2 [S,S], R) of the shifted S x S spectrum, in integers."""
    k = np.arange(S, dtype=np.int64) - S // 2           # row - mid, col - mid
    n = k[:, None] ** 2 + k[None, :] ** 2
    return ceil_sqrt(n), n, radial_bins(S)


@functools.lru_cache(maxsize=None)
def radial_freqs(S):
    """radialFreqs [R]: for every bin its last-visited member, found explicitly as the lexicographic maximum of (col, row); 0 for
    a bin without a member.  Also the boolean mask of the non-empty bins.  Cached: do not write into the result."""
    bins, n, R = geometry(S)
    rows, cols = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    key = (cols * S + rows).ravel()                      # the loop's visiting order
    freqs, nonempty = np.zeros(R), np.zeros(R, bool)
    b = bins.ravel()
    order = np.lexsort((key, b))                         # by bin, and inside a bin by visiting order: a group's last entry is its
    bs = b[order]                                        # lexicographic maximum of (col, row), explicitly
    for e in np.flatnonzero(np.r_[bs[1:] != bs[:-1], True]):
        freqs[bs[e]] = math.sqrt(int(n.ravel()[order[e]])) / R
        nonempty[bs[e]] = True
    return freqs, nonempty


def profile_vectorised(mag):
    """The same as profile_loop: the sums by np.add.at in the loop's visiting order, the frequencies by radial_freqs."""
    S = mag.shape[0]
    bins, _, R = geometry(S)
    prof = np.zeros(R)
    np.add.at(prof, bins.T.ravel(), mag.T.ravel())      # col outer, row inner
    return prof, radial_freqs(S)[0]


def moments(p):
    """(sum, std with N - 1, skewness, kurtosis) of the R entries: img_params.m:74-77 (the "mean" is the sum)."""
    R = p.size
    d = p - p.sum() / R
    m2, m3, m4 = (d ** 2).sum() / R, (d ** 3).sum() / R, (d ** 4).sum() / R
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.array([p.sum(), np.sqrt((d ** 2).sum() / (R - 1)), m3 / m2 ** 1.5, m4 / m2 ** 2])


def radial_profile(x):
    """One image [S,S] -> p = radialProfile / sum(radialProfile) * radialFreqs, [R]."""
    prof, freqs = profile_vectorised(shifted_magnitude(x))
    with np.errstate(invalid="ignore", divide="ignore"):
        return prof / prof.sum() * freqs


def freq_stats(x):
    return moments(radial_profile(x))


def condition_numbers(x):
    """sum |t| / |sum t| of every sum behind the four moments: the profile's sum, sum p, and the centred sums (the third included)."""
    prof, freqs = profile_vectorised(shifted_magnitude(x))
    p = prof / prof.sum() * freqs
    d = p - p.sum() / p.size
    cond = lambda t: float(np.abs(t).sum() / abs(t.sum()))
    return {"profile": cond(prof), "p": cond(p), "mean": cond(p), "m2": cond(d ** 2), "m3": cond(d ** 3), "m4": cond(d ** 4)}


# ---- the yardstick of the spectrum ------------------------------------------------------------------------------------------

def fft_radix2(v):
    """Plain recursive radix-2 decimation in time, complex128, along the last axis (a power of two)."""
    v = np.asarray(v, np.complex128)
    n = v.shape[-1]
    if n == 1:
        return v
    e, o = fft_radix2(v[..., 0::2]), fft_radix2(v[..., 1::2])
    w = np.exp(-2j * np.pi * np.arange(n // 2) / n)
    return np.concatenate([e + w * o, e - w * o], axis=-1)


def fft2_radix2(x):
    return fft_radix2(fft_radix2(np.asarray(x, np.float64)).swapaxes(-1, -2)).swapaxes(-1, -2)


def dft2_longdouble(x):
    """The direct 2-D DFT in numpy.longdouble: (re, im) of W x W^T with W[k, j] = exp(-2 pi i ((k j) mod S) / S)."""
    S = x.shape[-1]
    ld = np.longdouble
    kj = (np.arange(S)[:, None] * np.arange(S)[None, :]) % S
    ang = -(ld(2) * np.arccos(ld(-1))) * kj.astype(ld) / ld(S)      # pi in long double
    c, s = np.cos(ang), np.sin(ang)
    xl = np.asarray(x, ld)
    ar, ai = c @ xl, s @ xl                              # rows of W x
    return ar @ c.T - ai @ s.T, ar @ s.T + ai @ c.T
