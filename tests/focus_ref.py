"""The restatement of emdenoise.focus (include/emdenoise.h, "Autofocus") in numpy, for the tests: no GPU, no OpenCV.

Two forms.  The Laplacian is float32 in the header's fixed operation order (``laplacian``): the device must give the same bits.  The
statistics are float64 with the sums taken by ``math.fsum`` (exact, rounded once) -- or, with ``exact=False``, by numpy's pairwise
``sum``: the distance between the two is the yardstick of the GPU tests' bars.  scipy's ``kurtosis``, ``entropy`` and
``InterpolatedUnivariateSpline`` pin the statistics and the spline (tests/test_focus.py)."""
import math

import numpy as np

# the images of the hand-written border checks and their Laplacians (BORDER_REFLECT_101: index -1 -> 1, n -> n - 2)
HAND_2X2 = np.array([[1, 2], [4, 8]], np.float32)
HAND_2X2_K1 = np.array([[8, 10], [2, -20]], np.float32)
HAND_2X2_K3 = np.array([[56, 16], [-16, -56]], np.float32)
HAND_3X3 = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 10]], np.float32)
HAND_3X3_K1 = np.array([[8, 6, 4], [2, 0, -1], [-4, -5, -12]], np.float32)
HAND_3X3_K3 = np.array([[32, 24, 16], [8, 2, -8], [-16, -24, -40]], np.float32)


def laplacian(x, ksize):
    """float32 [..,H,W] -> float32, every operation a float32 operation of its own, in the header's order."""
    x = np.asarray(x, np.float32)
    assert ksize in (1, 3) and x.shape[-2] >= 2 and x.shape[-1] >= 2
    p = np.pad(x, [(0, 0)] * (x.ndim - 2) + [(1, 1), (1, 1)], mode="reflect")   # numpy's "reflect" is cv2's REFLECT_101
    c = p[..., 1:-1, 1:-1]
    if ksize == 1:
        u, d, l, r = p[..., :-2, 1:-1], p[..., 2:, 1:-1], p[..., 1:-1, :-2], p[..., 1:-1, 2:]
        y = ((u + d) + (l + r)) - np.float32(4) * c
    else:
        ul, ur, dl, dr = p[..., :-2, :-2], p[..., :-2, 2:], p[..., 2:, :-2], p[..., 2:, 2:]
        y = np.float32(2) * ((ul + ur) + (dl + dr)) - np.float32(8) * c
    assert y.dtype == np.float32
    return y


def _sum(a, exact):
    a = np.asarray(a, np.float64).ravel()
    return math.fsum(a.tolist()) if exact else float(np.sum(a))


def moments_of(L, rectify, exact=True):
    """The six columns of emd_laplacian_moments_f64 for one image's Laplacian (any shape), and the margin of the set's membership:
    the least |L - mean_L| over the image (inf without rectify)."""
    L = np.asarray(L, np.float64).ravel()
    mean_l = _sum(L, exact) / L.size
    S = L[L >= mean_l] if rectify else L
    margin = float(np.min(np.abs(L - mean_l))) if rectify else math.inf
    n = S.size
    with np.errstate(all="ignore"):
        mean_s = np.float64(_sum(S, exact)) / np.float64(n)
        d = S - mean_s
        d2 = d * d
        m2 = np.float64(_sum(d2, exact)) / np.float64(n)
        m4 = np.float64(_sum(d2 * d2, exact)) / np.float64(n)
        k = m4 / (m2 * m2) - 3.0
    return np.array([mean_l, n, mean_s, m2, m4, k], np.float64), margin


def laplacian_moments(x, ksize, rectify, exact=True):
    """[B,H,W] float32 -> ([B,6] float64, the smallest margin relative to max |L| over the batch)."""
    rows, rel = [], math.inf
    for img in np.asarray(x, np.float32):
        L = laplacian(img, ksize)
        row, margin = moments_of(L, rectify, exact)
        top = float(np.max(np.abs(L)))
        rel = min(rel, margin / top if top > 0 else math.inf)
        rows.append(row)
    return np.stack(rows), rel


def bin01(t, bins):
    """The rule: bin floor(t bins) for 0 <= t < 1, t == 1 in the last bin, -1 for everything else (NaN included)."""
    t = np.asarray(t)
    with np.errstate(invalid="ignore"):
        inside = (t >= 0) & (t < 1)
        k = np.where(inside, np.floor(np.where(inside, t, 0) * t.dtype.type(bins)), -1).astype(np.int64)
        return np.where(t == 1, bins - 1, k)


def histogram01(t, bins):
    """int64 [bins] of one image by the rule."""
    k = bin01(np.asarray(t).ravel(), bins)
    return np.bincount(k[k >= 0], minlength=bins).astype(np.int64)


def normalized(x, exact=True):
    """t = ((0.15 (x - mean)) / std) + 0.5 of one image in float64, mean and population std two-pass."""
    v = np.asarray(x, np.float32).astype(np.float64).ravel()
    mean = _sum(v, exact) / v.size
    d = v - mean
    std = math.sqrt(_sum(d * d, exact) / v.size)
    with np.errstate(all="ignore"):
        return ((0.15 * d) / np.float64(std)) + 0.5


def entropy(counts, eps):
    """-sum p log2 p, p = (c + eps) / sum (c + eps), with exact sums."""
    c = np.asarray(counts, np.float64) + eps
    p = c / math.fsum(c.tolist())
    with np.errstate(all="ignore"):
        terms = np.where(p > 0, -p * np.log(p), 0.0)
    return math.fsum(terms.tolist()) / math.log(2.0)


def notaknot_second_derivatives(z, y):
    """The second derivatives m [N] of the interpolating cubic spline with not-a-knot ends, from the full N x N system."""
    z, y = np.asarray(z, np.float64), np.asarray(y, np.float64)
    N = z.size
    assert N >= 4 and np.all(np.diff(z) > 0)
    h = np.diff(z)
    d = np.diff(y) / h
    A, rhs = np.zeros((N, N)), np.zeros(N)
    for i in range(1, N - 1):
        A[i, i - 1], A[i, i], A[i, i + 1] = h[i - 1], 2.0 * (h[i - 1] + h[i]), h[i]
        rhs[i] = 6.0 * (d[i] - d[i - 1])
    # the third derivative is continuous at z[1] and at z[N-2]
    A[0, 0], A[0, 1], A[0, 2] = h[1], -(h[0] + h[1]), h[0]
    A[N - 1, N - 3], A[N - 1, N - 2], A[N - 1, N - 1] = h[N - 2], -(h[N - 3] + h[N - 2]), h[N - 3]
    return np.linalg.solve(A, rhs)


def spline_eval(z, y, xs):
    z, y, xs = np.asarray(z, np.float64), np.asarray(y, np.float64), np.asarray(xs, np.float64)
    m = notaknot_second_derivatives(z, y)
    i = np.clip(np.searchsorted(z, xs, side="right") - 1, 0, z.size - 2)
    h, dx = z[i + 1] - z[i], xs - z[i]
    c1 = (y[i + 1] - y[i]) / h - h * (2.0 * m[i] + m[i + 1]) / 6.0
    c3 = (m[i + 1] - m[i]) / (6.0 * h)
    return y[i] + dx * (c1 + dx * (0.5 * m[i] + dx * c3))


def grid(z, interp_factor):
    z = np.asarray(z, np.float64)
    return np.linspace(z[0], z[-1], interp_factor * z.size)


def optimal_focus(z, scores, interp_factor, spline=None):
    """(zbest, curve, index) of one series; spline(z, scores) -> callable (default: this module's not-a-knot restatement)."""
    g = grid(z, interp_factor)
    curve = spline_eval(z, scores, g) if spline is None else spline(np.asarray(z, np.float64), np.asarray(scores, np.float64))(g)
    i = int(np.argmin(curve))
    return g[i], curve, i


def gaussian_blur(img, sigma):
    """A separable Gaussian blur (reflect borders, radius 4 sigma) in float64 -> float32: the synthetic through-focus series."""
    r = max(1, int(math.ceil(4 * sigma)))
    t = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    t /= t.sum()
    p = np.pad(np.asarray(img, np.float64), r, mode="reflect")
    p = sum(t[k] * p[k:k + img.shape[0], :] for k in range(2 * r + 1))
    p = sum(t[k] * p[:, k:k + img.shape[1]] for k in range(2 * r + 1))
    return p.astype(np.float32)


def focal_series(n=9, size=64, z0=0.3, seed=11):
    """(stack [n,size,size] float32, z [n] float64): one fixed random image blurred with a width that grows with |z - z0|."""
    rng = np.random.default_rng(seed)
    base = rng.poisson(30.0, (size, size)).astype(np.float32)
    z = np.linspace(-2.0, 2.0, n)
    return np.stack([gaussian_blur(base, 0.6 + 0.9 * abs(zi - z0)) for zi in z]), z
