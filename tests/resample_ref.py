"""cv2.resize for one-channel float32 restated in numpy from the rules of include/emdenoise.h (the section on csrc/resample.hip): the
reference of tests/test_resample.py and tests/test_resample_gpu.py.  OpenCV is not used.  Python floats and numpy float64 are IEEE
doubles and never fuse a multiply with an add; the float32 roundings the rules write out are ``np.float32`` casts.

``axis_taps`` states, for every destination sample of one axis, WHICH PIXEL gets WHICH WEIGHT, as the rules word it; it knows nothing
of how the library describes a sample.  ``resize`` applies two such tables as matrices: in float64 (the reference), or in float32 in
cv2's own order (float32 weights, a horizontal pass into float32 rows, a vertical pass in float32: the yardstick)."""
import collections

import numpy as np

NEAREST, LINEAR, CUBIC, AREA = 0, 1, 2, 3
MODES = {"nearest": NEAREST, "linear": LINEAR, "cubic": CUBIC, "area": AREA}
DBL_EPSILON = float(np.finfo(np.float64).eps)

Table = collections.namedtuple("Table", "index weight count block")   # index, weight: [n_out, K]; count: [n_out]; block: 0 or the side


def f32(a):
    """The rounding to float32 the rules write out, returned as float64."""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def scales(n_in, n_out):
    inv = float(n_out) / float(n_in)
    return inv, 1.0 / inv          # cv2's order: not n_in / n_out


def true_area(n_in, n_out, other_in, other_out):
    """The AREA rule looks at both axes: fractional coverage only where neither enlarges."""
    return scales(n_in, n_out)[1] >= 1.0 and scales(other_in, other_out)[1] >= 1.0


def whole_block(n_in, n_out):
    scale = scales(n_in, n_out)[1]
    i = int(scale)
    return i if abs(scale - i) < DBL_EPSILON else 0


def _linear_pair(s, f, n_in):
    """LINEAR's two clamps, then pixels s and min(s + 1, n_in - 1) with 1 - f and f."""
    low = s < 0
    s = np.where(low, 0, s)
    f = np.where(low, 0.0, f)
    high = s >= n_in - 1
    s = np.where(high, n_in - 1, s)
    f = np.where(high, 0.0, f)
    index = np.stack([s, np.minimum(s + 1, n_in - 1)], axis=1)
    weight = np.stack([1.0 - f, f], axis=1)
    return index, weight


def axis_taps(interpolation, n_in, n_out, other_in=None, other_out=None):
    """-> Table.  Sample d reads pixel ``index[d, k]`` with ``weight[d, k]`` for k < ``count[d]``; behind that the last index repeats
    with weight 0.  In the whole-ratio area form (``block`` != 0) the weights are 1 / block."""
    mode = MODES.get(interpolation, interpolation)
    other_in = n_in if other_in is None else other_in
    other_out = n_out if other_out is None else other_out
    inv, scale = scales(n_in, n_out)
    d = np.arange(n_out, dtype=np.float64)
    block = 0
    if mode == NEAREST:
        s = np.minimum(np.floor(d * scale), n_in - 1).astype(np.int64)
        index, weight = s[:, None], np.ones((n_out, 1))
    elif mode in (LINEAR, CUBIC):
        f = f32((d + 0.5) * scale - 0.5)          # rounded to float32 once, before the floor
        s = np.floor(f)
        f = f32(f - s)
        s = s.astype(np.int64)
        if mode == LINEAR:
            index, weight = _linear_pair(s, f, n_in)
        else:
            A = -0.75
            c0 = ((A * (f + 1.0) - 5.0 * A) * (f + 1.0) + 8.0 * A) * (f + 1.0) - 4.0 * A
            c1 = ((A + 2.0) * f - (A + 3.0)) * f * f + 1.0
            c2 = ((A + 2.0) * (1.0 - f) - (A + 3.0)) * (1.0 - f) * (1.0 - f) + 1.0
            c3 = 1.0 - c0 - c1 - c2
            index = np.clip(s[:, None] + np.arange(-1, 3)[None, :], 0, n_in - 1)     # border replicate
            weight = np.stack([c0, c1, c2, c3], axis=1)
    elif mode == AREA and not true_area(n_in, n_out, other_in, other_out):
        s = np.floor(d * scale)
        f = f32((d + 1.0) - (s + 1.0) * inv)
        f = np.where(f <= 0.0, 0.0, f32(f - np.floor(f)))
        index, weight = _linear_pair(s.astype(np.int64), f, n_in)
    elif mode == AREA:
        bx, by = whole_block(n_in, n_out), whole_block(other_in, other_out)
        if bx and by:
            block = bx
            index = (np.arange(n_out) * bx)[:, None] + np.arange(bx)[None, :]
            weight = np.full((n_out, bx), 1.0 / bx)
        else:
            f1 = d * scale
            f2 = f1 + scale
            cell = np.minimum(scale, n_in - f1)
            s1 = np.ceil(f1)
            s2 = np.minimum(np.floor(f2), n_in - 1)
            s1 = np.minimum(s1, s2)
            head, tail = s1 - f1 > 1e-3, f2 - s2 > 1e-3
            wh = f32((s1 - f1) / cell)
            wm = f32(1.0 / cell)
            wt = f32(np.minimum(np.minimum(f2 - s2, 1.0), cell) / cell)
            first = (s1 - head).astype(np.int64)
            count = (head + (s2 - s1) + tail).astype(np.int64)
            p = first[:, None] + np.arange(max(int(count.max()), 1))[None, :]             # candidate pixels
            c = lambda v: v[:, None]
            weight = np.where((p == c(s1) - 1) & c(head), c(wh),
                              np.where((p >= c(s1)) & (p < c(s2)), c(wm), np.where((p == c(s2)) & c(tail), c(wt), 0.0)))
            index = np.minimum(p, c(first + np.maximum(count - 1, 0)))
            weight = np.where(p < c(first + count), weight, 0.0)
            return Table(index.astype(np.int64), weight, count, 0)
    else:
        raise ValueError(interpolation)
    return Table(np.asarray(index, np.int64), np.asarray(weight, np.float64), np.full(n_out, index.shape[1], np.int64), block)


def matrix(table, n_in, dtype=np.float64):
    """[n_out, n_in]: the table as a matrix (weights of taps that read the same pixel add up)."""
    n_out, K = table.index.shape
    M = np.zeros((n_out, n_in), np.float64)
    np.add.at(M, (np.repeat(np.arange(n_out), K), table.index.ravel()), table.weight.ravel())
    return M.astype(dtype)


def resize(x, dsize, interpolation, dtype=np.float64):
    """``cv2.resize(x, dsize, interpolation=...)`` of ``[H,W]`` or ``[B,H,W]``; dsize = (w, h) or an int.  dtype float64: weights, sums and
    result in double (whole-ratio area: the block's sum divided by its pixel count).  dtype float32: cv2's order of operations."""
    x = np.asarray(x)
    w, h = (dsize, dsize) if isinstance(dsize, (int, np.integer)) else dsize
    H, W = x.shape[-2:]
    ty, tx = axis_taps(interpolation, H, h, W, w), axis_taps(interpolation, W, w, H, h)
    if dtype == np.float64 and tx.block:
        ones = lambda t: Table(t.index, np.ones_like(t.weight), t.count, t.block)
        s = matrix(ones(ty), H) @ x.astype(np.float64) @ matrix(ones(tx), W).T
        return s / float(ty.block * tx.block)
    My, Mx = matrix(ty, H, dtype), matrix(tx, W, dtype)
    rows = (x.astype(dtype) @ Mx.T).astype(dtype)
    return (My @ rows).astype(dtype)


def crop_resize(x, boxes, dsize, interpolation, dtype=np.float64):
    """Image b's rectangle (x0, y0, bw, bh) resized to dsize: the restatement applied to the numpy slice."""
    return np.stack([resize(im[y0:y0 + bh, x0:x0 + bw], dsize, interpolation, dtype) for im, (x0, y0, bw, bh) in zip(x, boxes)])
