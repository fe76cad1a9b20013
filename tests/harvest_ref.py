"""The numpy restatement of the harvester (emdenoise.harvest; include/emdenoise.h "Harvesting raw micrographs"): MATLAB's
``imresize(crop, [S, S], 'method', 'box')`` by its general ``contributions`` algorithm (the candidate matrix, the weights
``h(u - indices)``, row normalisation and the mirror fold of indices, applied as W X W^T), every statistic of ``img_params.m``, and
``estimate_noise.m``'s sum over the full convolution.  float64 unless a dtype is given.  MATLAB itself is not available: this is
written from the published algorithm, independently of the library's table function (which it checks)."""
from fractions import Fraction

import numpy as np

STAT_NAMES = ["min", "max", "nonzero", "negative", "mean", "std", "skewness", "kurtosis", "median", "rms", "coeff_variation", "noise",
              "sqrt_mean", "sqrt_std", "sqrt_skewness", "sqrt_kurtosis", "sqrt_mean_ratio"]


def box(x):
    return ((-0.5 <= x) & (x < 0.5)).astype(np.float64)


def contributions(n_in, n_out):
    """(weights [n_out, P], indices [n_out, P] 1-based after the mirror fold, indices before the fold) of imresize's box kernel with
    antialiasing, in IEEE double, one operation at a time."""
    scale = n_out / n_in
    if scale < 1:
        h = lambda x: scale * box(scale * x)
        kw = 1.0 / scale
    else:
        h = box
        kw = 1.0
    x = np.arange(1, n_out + 1, dtype=np.float64)
    u = x / scale + 0.5 * (1 - 1 / scale)
    left = np.floor(u - kw / 2)
    P = int(np.ceil(kw)) + 2
    unfolded = (left[:, None] + np.arange(P)[None, :]).astype(np.int64)
    weights = h(u[:, None] - unfolded)
    weights = weights / weights.sum(1, keepdims=True)
    aux = np.concatenate([np.arange(1, n_in + 1), np.arange(n_in, 0, -1)])
    return weights, aux[np.mod(unfolded - 1, aux.size)], unfolded


def runs(n_in, n_out):
    """int [n_out, 2]: (first member 0-based, count) of the non-zero weights of every output; asserts what the device kernel relies
    on: the members are one contiguous run inside the input, untouched by the mirror fold."""
    w, idx, unfolded = contributions(n_in, n_out)
    nz = w != 0
    count = nz.sum(1)
    first_slot = nz.argmax(1)
    rows = np.arange(n_out)
    first = unfolded[rows, first_slot]
    last_slot = nz.shape[1] - 1 - nz[:, ::-1].argmax(1)
    assert (count >= 1).all() and (last_slot - first_slot + 1 == count).all(), (n_in, n_out)
    assert (first >= 1).all() and (first + count - 1 <= n_in).all() and (idx[nz] == unfolded[nz]).all(), (n_in, n_out)
    return np.stack([first - 1, count], 1)


def exact_runs(n_in, n_out):
    """The same in exact rational arithmetic, over the common denominator: with d = n_in, S = n_out, u - i = (2xd + S - d - 2iS) / 2S
    and t = that times S/d when shrinking; member iff -1/2 <= t < 1/2.  (first 0-based, count) per output."""
    d, S = n_in, n_out
    x = np.arange(1, S + 1, dtype=np.int64)[:, None]
    i = np.arange(1, d + 1, dtype=np.int64)[None, :]
    num = 2 * x * d + S - d - 2 * i * S
    bound = d if S < d else S
    member = (-bound <= num) & (num < bound)
    return np.stack([member.argmax(1), member.sum(1)], 1)


def exact_member_fraction(n_in, n_out, x, i):
    """Membership of input i (1-based) in output x (1-based) with ``fractions.Fraction``, straight from the definition."""
    scale = Fraction(n_out, n_in)
    u = Fraction(x) / scale + Fraction(1, 2) * (1 - 1 / scale)
    t = scale * (u - i) if scale < 1 else u - i
    return Fraction(-1, 2) <= t < Fraction(1, 2)


def weight_matrix(n_in, n_out):
    w, idx, _ = contributions(n_in, n_out)
    m = np.zeros((n_out, n_in))
    np.add.at(m, (np.repeat(np.arange(n_out), w.shape[1]), idx.ravel() - 1), w.ravel())
    return m


def box_resize(x, size, dtype=np.float64):
    """[..., H, W] -> [..., size, size]: crop to the top-left d x d, d = min(H, W), then W X W^T in ``dtype``."""
    d = min(x.shape[-2:])
    m = weight_matrix(d, size).astype(dtype)
    return m @ x[..., :d, :d].astype(dtype) @ m.T


def noise_sum(x):
    """sum |conv2_full(x, [1 -2 1; -2 4 -2; 1 -2 1])| of one image, over the (H + 2) x (W + 2) zero-padded convolution."""
    k = np.array([[1.0, -2.0, 1.0], [-2.0, 4.0, -2.0], [1.0, -2.0, 1.0]])
    H, W = x.shape
    p = np.pad(x.astype(np.float64), 2)
    full = sum(k[a, b] * p[a:a + H + 2, b:b + W + 2] for a in range(3) for b in range(3))   # the kernel is symmetric
    return float(np.abs(full).sum())


def moments(v):
    """(mean, std with N - 1, skewness, kurtosis) of a float64 vector: two-pass central moments."""
    n = v.size
    mean = v.mean()
    dv = v - mean
    m2, m3, m4 = (dv ** 2).sum() / n, (dv ** 3).sum() / n, (dv ** 4).sum() / n
    return mean, np.sqrt((dv ** 2).sum() / (n - 1)), m3 / m2 ** 1.5, m4 / m2 ** 2


def image_stats(x):
    """[H, W] -> the seventeen, float64, in STAT_NAMES' order."""
    H, W = x.shape
    v = x.astype(np.float64).ravel()
    mean, std, skew, kurt = moments(v)
    smean, sstd, sskew, skurt = moments(np.sqrt(np.maximum(v, 0.0)))
    noise = noise_sum(x) * np.sqrt(0.5 * np.pi) / (6.0 * (W - 2) * (H - 2))
    return np.array([v.min(), v.max(), np.count_nonzero(v), np.count_nonzero(v < 0), mean, std, skew, kurt, np.median(v),
                     np.sqrt((v ** 2).mean()), 100.0 * std / mean, noise, smean, sstd, sskew, skurt, smean / mean])


def condition_numbers(x):
    """sum |t| / |sum t| of the sums that can cancel: the mean, the third central moments of x and of sqrt(max(x, 0))."""
    v = x.astype(np.float64).ravel()
    s = np.sqrt(np.maximum(v, 0.0))
    cond = lambda t: float(np.abs(t).sum() / abs(t.sum()))
    return {"mean": cond(v), "m3": cond((v - v.mean()) ** 3), "sqrt_m3": cond((s - s.mean()) ** 3)}


def scale01(x):
    """float32 (x - min) / (max - min); a constant image -> 0.5."""
    x = x.astype(np.float32)
    lo, hi = x.min(), x.max()
    if abs(float(hi) - float(lo)) < 1e-6:
        return np.full_like(x, 0.5)
    return (x - lo) / (hi - lo)
