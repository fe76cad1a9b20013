"""TEST INFRASTRUCTURE ONLY: the numpy restatement of csrc/dose.hip (include/emdenoise.h, "Dose series") -- the
weights, the CDF, the draws, the levels and the rescales, all in integers, so that the device is compared bit for bit.  The
reference (misc_py/lq_img_gen-backup.py) is not run: its arithmetic is restated here with the three departures the header lists."""
import functools

import numpy as np

from oracle.input_ops_ref import philox4x32_10

TAG_DOSE = 9
EMPTY, SANITIZED = 1, 2
M32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def weights(x):
    """float32 image -> (q uint64, flat, row-major; status)."""
    x = np.asarray(x, np.float32).ravel()
    finite = np.isfinite(x)
    good = finite & (x > 0)
    status = (0 if good.any() else EMPTY) | (SANITIZED if (~finite | (x < 0)).any() else 0)
    q = np.zeros(x.size, np.uint64)
    if good.any():
        m = np.float64(x[good].max())
        q[good] = np.rint(x[good].astype(np.float64) / m * 4294967296.0).astype(np.uint64)
    return q, status


def cdf(x):
    """-> (C int64 of x's shape: the inclusive row-major prefix sum of the weights; status)."""
    q, status = weights(x)
    return np.cumsum(q, dtype=np.uint64).astype(np.int64).reshape(np.shape(x)), status


def mulhi64(a, b):
    """The high 64 bits of the 128-bit product of uint64 arrays, from 32-bit halves (no intermediate exceeds 64 bits)."""
    a, b = np.asarray(a, np.uint64), np.asarray(b, np.uint64)
    a0, a1, b0, b1 = a & M32, a >> S32, b & M32, b >> S32
    p01, p10 = a0 * b1, a1 * b0
    mid = ((a0 * b0) >> S32) + (p01 & M32) + (p10 & M32)
    return a1 * b1 + (p01 >> S32) + (p10 >> S32) + (mid >> S32)


@functools.lru_cache(maxsize=64)
def draw_words(first, count, seed, image):
    """r of the draws first .. first + count - 1 of one image's stream (uint64): call j = d >> 1, even d the words x, y, odd d z, w."""
    d = np.arange(count, dtype=np.uint64) + np.uint64(first)
    j = d >> np.uint64(1)
    x, y, z, w = philox4x32_10([j & M32, j >> S32, np.full(count, image, np.uint64), np.full(count, TAG_DOSE, np.uint64)],
                               [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF])
    odd = (d & np.uint64(1)).astype(bool)
    r = (np.where(odd, z, x).astype(np.uint64) << S32) | np.where(odd, w, y).astype(np.uint64)
    r.setflags(write=False)
    return r


def pixels(C, first, count, seed, image):
    """The flat pixel of every draw: p = #{i : C[i] <= t}, t = (r T) >> 64."""
    C = np.asarray(C).ravel().astype(np.uint64)
    t = mulhi64(draw_words(int(first), int(count), int(seed), int(image)), C[-1])
    return np.searchsorted(C, t, side="right")


def sample_counts(x, draws, seed=0, first_draw=0, image=0):
    """int32 counts of the draws [first_draw, first_draw + draws) of one image."""
    C, status = cdf(x)
    n = C.size
    if status & EMPTY or draws == 0:
        return np.zeros(np.shape(x), np.int32)
    return np.bincount(pixels(C, first_draw, draws, seed, image), minlength=n).astype(np.int32).reshape(np.shape(x))


def series(x, bounds, seed=0, image=0):
    """int32 [L,H,W]: plane k counts every draw in [bounds[0], bounds[k+1])."""
    C, status = cdf(x)
    n, L = C.size, len(bounds) - 1
    out = np.zeros((L,) + tuple(np.shape(x)), np.int32)
    if status & EMPTY or bounds[-1] == bounds[0]:
        return out
    p = pixels(C, bounds[0], bounds[-1] - bounds[0], seed, image)
    for k in range(L):
        out[k] = np.bincount(p[: bounds[k + 1] - bounds[0]], minlength=n).reshape(np.shape(x))
    return out


def rescale(plane, mode):
    """record_lq (:30-35) of one plane of counts, as numpy forms it on float64 data; a flat plane -> zeros."""
    c = np.asarray(plane).astype(np.float64)
    lo, hi = c.min(), c.max()
    if hi == lo:
        return np.zeros(c.shape, np.int32 if mode == "uint16" else np.float32)
    if mode == "uint16":
        return (65535 * (c - lo) / (hi - lo)).astype(np.uint16).astype(np.int32)
    return ((c - lo) / (hi - lo)).astype(np.float32)


def lq_levels(avg_counts, chunkdepth, size):
    """The reference's chunk counting (:52-55, :72-83): chunks of chunkdepth * size electrons, level k after int(avg / chunkdepth)."""
    chunksize = size * chunkdepth
    return [int(avg / chunkdepth) * chunksize for avg in avg_counts]


def lq_img_gen(img, avg_counts=(2, 4, 8, 16, 32, 64), chunkdepth=2, seed=0):
    img = np.asarray(img, np.float32)
    s = series(img, [0] + lq_levels(avg_counts, chunkdepth, img.size), seed, 0)
    return [rescale(p, "uint16").astype(np.uint16) for p in s]
