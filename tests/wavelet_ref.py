"""CPU restatement of the 2-D orthogonal wavelet transform and of wavelet-shrinkage denoising for the tests (emdenoise.filters
wavedec2 / waverec2 / denoise_wavelet, csrc/wavelet.hip).

Neither skimage nor pywt is a dependency: this file is written from the formulas of include/emdenoise.h (pywt's "symmetric" mode,
its waverecn cropping rule, skimage's _sigma_est_dwt, _bayes_thresh and _universal_thresh) and IS the specification the device is
checked against.  Every function takes one image ``[H,W]`` or a batch ``[B,H,W]`` (each image on its own) and a ``dtype``:
numpy.float64 is the reference; numpy.float32 (every array and every tap in float32) is used only as a yardstick -- its own distance
from the float64 result sets the tolerances."""
import numpy as np

MAD_TO_SIGMA = 0.6744897501960817
METHODS = ("BayesShrink", "VisuShrink")


def rec_lo_of(wavelet):
    """Reconstruction low-pass taps (float64) of a named wavelet or of a tap array."""
    if isinstance(wavelet, str):
        if wavelet in ("haar", "db1"):
            return np.array([1.0, 1.0]) / np.sqrt(2.0)
        if wavelet == "db2":
            s3 = np.sqrt(3.0)
            return np.array([1 + s3, 3 + s3, 3 - s3, 1 - s3]) / (4 * np.sqrt(2.0))
        raise ValueError(wavelet)
    return np.asarray(wavelet, np.float64)


def daubechies(N):
    """rec_lo of the Daubechies wavelet with N vanishing moments (2N taps) by spectral factorisation: |H(w)|^2 = 2 cos^2N(w/2)
    P(sin^2(w/2)) with P(y) = sum_k C(N-1+k, k) y^k; every root y of P gives z + 1/z = 2 - 4y, and the roots z inside the unit circle
    go with the N-fold zero at z = -1."""
    from math import comb

    p = [comb(N - 1 + k, k) for k in range(N)]                           # ascending powers of y
    zs = []
    for y in np.roots(p[::-1]):
        z = np.roots([1.0, -(2.0 - 4.0 * y), 1.0])
        zs.append(z[np.argmin(np.abs(z))])
    h = np.poly(np.concatenate([-np.ones(N), np.array(zs, dtype=complex)]))
    h = np.real(h)
    return h * (np.sqrt(2.0) / h.sum())


def filter_bank(wavelet, dtype=np.float64):
    """(dec_lo, dec_hi, rec_lo, rec_hi), each rounded to dtype once."""
    rec_lo = rec_lo_of(wavelet)
    L = len(rec_lo)
    dec_lo = rec_lo[::-1].copy()
    dec_hi = np.array([(-1.0) ** (k + 1) * rec_lo[k] for k in range(L)])
    rec_hi = dec_hi[::-1].copy()
    return tuple(f.astype(dtype) for f in (dec_lo, dec_hi, rec_lo, rec_hi))


def max_levels(H, W, L):
    k = -1
    while (L - 1) * 2 ** (k + 1) <= min(H, W):
        k += 1
    return k


def default_levels(H, W, L):
    return max(max_levels(H, W, L) - 3, 1)


def _sym(idx, N):
    m = np.mod(idx, 2 * N)
    return np.where(m < N, m, 2 * N - 1 - m)


def _analysis(x, dec, axis):
    """c[i] = sum_k dec[k] x~[2i + 1 - k], i < (N + L - 1) // 2, x~ the half-sample symmetric extension."""
    N, L = x.shape[axis], len(dec)
    i = np.arange((N + L - 1) // 2)
    out = None
    for k in range(L):
        term = dec[k] * np.take(x, _sym(2 * i + 1 - k, N), axis=axis)
        out = term if out is None else out + term
    return out


def _synthesis(a, d, rec_lo, rec_hi, axis, n_out):
    """x[j] = sum_i a[i] rec_lo[j + L - 2 - 2i] + d[i] rec_hi[j + L - 2 - 2i], j < n_out <= 2n - L + 2."""
    a, d = np.moveaxis(a, axis, 0), np.moveaxis(d, axis, 0)
    n, L = a.shape[0], len(rec_lo)
    assert n_out <= 2 * n - L + 2, (n_out, n, L)
    out = np.zeros((n_out,) + a.shape[1:], a.dtype)
    for k in range(L):
        j = 2 * np.arange(n) + k - (L - 2)
        ok = (j >= 0) & (j < n_out)
        out[j[ok]] += a[ok] * rec_lo[k] + d[ok] * rec_hi[k]
    return np.moveaxis(out, 0, axis)


def dwt2(x, bank):
    dec_lo, dec_hi = bank[0], bank[1]
    lo, hi = _analysis(x, dec_lo, 0), _analysis(x, dec_hi, 0)
    return _analysis(lo, dec_lo, 1), {"ad": _analysis(lo, dec_hi, 1), "da": _analysis(hi, dec_lo, 1), "dd": _analysis(hi, dec_hi, 1)}


def idwt2(cA, det, bank, shape):
    """Along W first, then along H; cropped to shape."""
    rec_lo, rec_hi = bank[2], bank[3]
    lo = _synthesis(cA, det["ad"], rec_lo, rec_hi, 1, shape[1])
    hi = _synthesis(det["da"], det["dd"], rec_lo, rec_hi, 1, shape[1])
    return _synthesis(lo, hi, rec_lo, rec_hi, 0, shape[0])


def _levels_of(shape, L, levels):
    if levels is None:
        return default_levels(shape[0], shape[1], L)
    assert 1 <= levels <= max_levels(shape[0], shape[1], L), levels
    return levels


def _wavedec2_one(x, bank, levels):
    coeffs, a = [], x
    for _ in range(levels):
        a, det = dwt2(a, bank)
        coeffs.insert(0, det)
    return [a] + coeffs


def _waverec2_one(coeffs, bank, shape):
    """The shapes of the levels below follow from the detail bands (the approximation of a level is cropped to them)."""
    a = coeffs[0]
    for i, det in enumerate(coeffs[1:]):
        target = coeffs[i + 2]["ad"].shape if i + 2 < len(coeffs) else tuple(shape)
        a = idwt2(a[:det["ad"].shape[0], :det["ad"].shape[1]], det, bank, target)
    return a


def wavedec2(x, wavelet="db1", levels=None, dtype=np.float64):
    """-> [cA_n, {"ad","da","dd"}_n, ..., {...}_1]; a batch gives batched bands."""
    x = np.asarray(x).astype(dtype)
    bank = filter_bank(wavelet, dtype)
    levels = _levels_of(x.shape[-2:], len(bank[0]), levels)
    if x.ndim == 2:
        return _wavedec2_one(x, bank, levels)
    per = [_wavedec2_one(im, bank, levels) for im in x]
    return [np.stack([p[0] for p in per])] + [{k: np.stack([p[i][k] for p in per]) for k in ("ad", "da", "dd")}
                                              for i in range(1, levels + 1)]


def waverec2(coeffs, wavelet, shape, dtype=np.float64):
    bank = filter_bank(wavelet, dtype)
    cast = lambda c: {k: np.asarray(v).astype(dtype) for k, v in c.items()} if isinstance(c, dict) else np.asarray(c).astype(dtype)
    coeffs = [cast(c) for c in coeffs]
    if coeffs[0].ndim == 2:
        return _waverec2_one(coeffs, bank, shape[-2:])
    one = lambda b: [coeffs[0][b]] + [{k: v[b] for k, v in c.items()} for c in coeffs[1:]]
    return np.stack([_waverec2_one(one(b), bank, shape[-2:]) for b in range(coeffs[0].shape[0])])


def sigma_est(dd1):
    """skimage's _sigma_est_dwt: the median of |dd_1| over the coefficients that are not exactly 0, / 0.6745; none: 0."""
    a = np.abs(dd1[dd1 != 0])
    if a.size == 0:
        return dd1.dtype.type(0)
    return np.median(a) / dd1.dtype.type(MAD_TO_SIGMA)


def bayes_threshold(d, var):
    """var / sqrt(max(mean(d^2) - var, float32's epsilon))."""
    return var / np.sqrt(max(np.mean(d * d) - var, d.dtype.type(np.finfo(np.float32).eps)))


def visu_threshold(sigma, shape):
    return sigma * np.sqrt(2.0 * np.log(float(shape[0]) * float(shape[1])))


def soft(d, t):
    return np.sign(d) * np.maximum(np.abs(d) - t, 0)


def denoise_wavelet(x, wavelet="db1", levels=None, method="BayesShrink", sigma=None, dtype=np.float64, return_sigma=False):
    """Soft-threshold every detail band of every level (never cA) and transform back; no clip."""
    assert method in METHODS, method
    x = np.asarray(x)
    if x.ndim == 3:
        res = [denoise_wavelet(im, wavelet, levels, method, sigma, dtype, True) for im in x]
        y, s = np.stack([r[0] for r in res]), np.array([r[1] for r in res], dtype)
        return (y, s) if return_sigma else y
    x = x.astype(dtype)
    bank = filter_bank(wavelet, dtype)
    coeffs = _wavedec2_one(x, bank, _levels_of(x.shape, len(bank[0]), levels))
    s = dtype(sigma) if sigma is not None else dtype(sigma_est(coeffs[-1]["dd"]))
    var = s * s
    out = [coeffs[0]]
    for det in coeffs[1:]:
        if method == "BayesShrink":
            out.append({k: soft(d, dtype(bayes_threshold(d, var))) for k, d in det.items()})
        else:
            out.append({k: soft(d, dtype(visu_threshold(s, x.shape))) for k, d in det.items()})
    y = _waverec2_one(out, bank, x.shape)
    return (y, s) if return_sigma else y
