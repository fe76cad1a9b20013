"""The float64 numpy restatement of the affine registration by mutual information and of the warp (emdenoise.affine;
include/emdenoise.h "Affine registration of a focal series"), written from the formulas of the header and independent of the library.
MATLAB is not available and is not run: the formulas are the specification.

Everything the device is compared with bit for bit uses only operations that IEEE 754 rounds correctly (+ - * / sqrt floor ceil rint),
one at a time, left to right as the header writes them: numpy's element-wise arithmetic does not fuse, and the 6 x 6 algebra runs on
Python floats.  The histogram is a sum of integers.  ``log``, ``sinpi`` and ``cospi`` are library functions on both sides: values that
go through them are compared within a bar."""
import math

import numpy as np

from oracle.input_ops_ref import philox4x32_10

PAD = 2
TAG_SAMPLES, TAG_NORMAL = 7, 8
CONVERGED, DEGENERATE, EXHAUSTED = 1, 2, 4
MASK = 0xFFFFFFFF


def geometry(H, W):
    return (W - 1) / 2, (H - 1) / 2, max(H, W) / 2


def identity():
    return np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])


def similarity(angle_deg, scale, shift_px, H, W):
    """The pull map that samples the moving image at scale R(angle) (point - c) + c + shift_px."""
    h = geometry(H, W)[2]
    a = np.deg2rad(angle_deg)
    return np.array([[scale * np.cos(a), -scale * np.sin(a), shift_px[0] / h], [scale * np.sin(a), scale * np.cos(a), shift_px[1] / h]])


def pull(T, H, W, x, y):
    """(x', y') of the pixels (x, y) (arrays) under the pull map T [2,3]."""
    T = np.asarray(T, np.float64).reshape(2, 3)
    cx, cy, h = geometry(H, W)
    with np.errstate(invalid="ignore", over="ignore"):
        u, v = (np.asarray(x, np.float64) - cx) / h, (np.asarray(y, np.float64) - cy) / h
        us = (T[0, 0] * u + T[0, 1] * v) + T[0, 2]
        vs = (T[1, 0] * u + T[1, 1] * v) + T[1, 2]
        return us * h + cx, vs * h + cy


def _taps(img, xs, ys, fill):
    """ix, iy, fx, fy, the four taps (fill outside) and the mask 'some tap inside' of float64 coordinates xs, ys."""
    H, W = img.shape
    with np.errstate(invalid="ignore"):
        flx, fly = np.floor(xs), np.floor(ys)
        fx, fy = xs - flx, ys - fly
        okx, oky = (flx > -1e9) & (flx < 1e9), (fly > -1e9) & (fly < 1e9)
    ix = np.where(okx, flx, -2e9).astype(np.int64)
    iy = np.where(oky, fly, -2e9).astype(np.int64)
    img64 = img.astype(np.float64)

    def tap(j, k):
        yy, xx = iy + j, ix + k
        inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        return np.where(inside, img64[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], fill), inside

    (p00, i00), (p01, i01), (p10, i10), (p11, i11) = tap(0, 0), tap(0, 1), tap(1, 0), tap(1, 1)
    return fx, fy, p00, p01, p10, p11, i00 | i01 | i10 | i11


def bilinear(fx, fy, p00, p01, p10, p11):
    with np.errstate(invalid="ignore"):
        return (1 - fy) * ((1 - fx) * p00 + fx * p01) + fy * ((1 - fx) * p10 + fx * p11)


def warp(images, T, fill=0.0):
    """[N,H,W] float32 through one T [2,3] for all, or [N,2,3]."""
    images = np.asarray(images, np.float32)
    N, H, W = images.shape
    T = np.asarray(T, np.float64)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.empty_like(images)
    f32 = np.float32(fill)
    for n in range(N):
        xs, ys = pull(T if T.ndim == 2 else T[n], H, W, xx, yy)
        fx, fy, p00, p01, p10, p11, some = _taps(images[n], xs, ys, np.float64(f32))
        v = bilinear(fx, fy, p00, p01, p10, p11)
        out[n] = np.where(some, v, np.float64(f32)).astype(np.float32)
    return out


def bspline3(u):
    a = np.abs(np.asarray(u, np.float64))
    a2 = a * a
    a3 = a2 * a
    inner = ((4.0 - 6.0 * a2) + 3.0 * a3) / 6.0
    t = 2.0 - a
    outer = ((t * t) * t) / 6.0
    return np.where(a < 1.0, inner, np.where(a < 2.0, outer, 0.0))


def draw_samples(n, H, W, seed=0):
    i = np.arange(n, dtype=np.uint64)
    j = i // np.uint64(4)
    z = np.zeros(n, np.uint64)
    r = philox4x32_10([j & np.uint64(MASK), z, z, np.full(n, TAG_SAMPLES, np.uint64)], [seed & MASK, (seed >> 32) & MASK])
    words = np.stack(r, axis=1)[np.arange(n), (i % np.uint64(4)).astype(np.int64)].astype(np.uint64)
    return ((words * np.uint64(H * W)) >> np.uint64(32)).astype(np.uint32)


def _parzen_index(v, lo, width, bins):
    t = (v - lo) / width + PAD
    return t, np.clip(np.floor(t), PAD, bins - PAD - 1).astype(np.int64)


def joint_histogram(fixed, moving, T, samples=None, bins=50):
    """int64 [bins,bins], or None where an image is constant."""
    fixed, moving = np.asarray(fixed, np.float32), np.asarray(moving, np.float32)
    H, W = fixed.shape
    fmin, fmax, mmin, mmax = (np.float64(v) for v in (fixed.min(), fixed.max(), moving.min(), moving.max()))
    if not (fmax > fmin and mmax > mmin):
        return None
    idx = np.arange(H * W, dtype=np.int64) if samples is None else np.asarray(samples).astype(np.int64)
    idx = idx[idx < H * W]
    y, x = idx // W, idx % W
    xs, ys = pull(T, H, W, x, y)
    with np.errstate(invalid="ignore"):
        valid = (xs >= 0) & (xs <= W - 1) & (ys >= 0) & (ys <= H - 1)
    idx, xs, ys = idx[valid], xs[valid], ys[valid]
    fx, fy, p00, p01, p10, p11, _ = _taps(moving, xs, ys, 0.0)
    m = bilinear(fx, fy, p00, p01, p10, p11)
    bf, bm = (fmax - fmin) / (bins - 2 * PAD), (mmax - mmin) / (bins - 2 * PAD)
    _, jf = _parzen_index(fixed.ravel()[idx].astype(np.float64), fmin, bf, bins)
    tm, jm = _parzen_index(m, mmin, bm, bins)
    hist = np.zeros(bins * bins, np.int64)
    for d in (-1, 0, 1, 2):
        w = bspline3((jm + d).astype(np.float64) - tm)
        np.add.at(hist, jf * bins + jm + d, np.rint(w * 4294967296.0).astype(np.int64))
    return hist.reshape(bins, bins)


def mi_terms(hist):
    """The bins' terms P log(P / (pf pm)), [bins,bins] (0 for an empty bin), and n."""
    n = int(hist.sum())
    if n == 0:
        return np.zeros(hist.shape), 0
    dn = np.float64(n)
    P = hist.astype(np.float64) / dn
    pf = hist.sum(1).astype(np.float64) / dn
    pm = hist.sum(0).astype(np.float64) / dn
    with np.errstate(divide="ignore", invalid="ignore"):
        t = P * np.log(P / (pf[:, None] * pm[None, :]))
    return np.where(hist > 0, t, 0.0), n


def mi_of_histogram(hist):
    """The header's order and form: one accumulator over the bins in row-major order."""
    if hist is None:
        return 0.0
    t, n = mi_terms(hist)
    return float(np.add.accumulate(t.ravel())[-1]) if n else 0.0


def mi_of_histogram_logs(hist):
    """Another float64 evaluation of the same histogram: P (log P - log pf - log pm) under numpy's pairwise sum."""
    if hist is None or hist.sum() == 0:
        return 0.0
    dn = np.float64(int(hist.sum()))
    P = hist.astype(np.float64) / dn
    with np.errstate(divide="ignore", invalid="ignore"):
        lf, lm = np.log(hist.sum(1).astype(np.float64) / dn), np.log(hist.sum(0).astype(np.float64) / dn)
        t = P * (np.log(P) - lf[:, None] - lm[None, :])
    return float(np.sum(np.where(hist > 0, t, 0.0)))


def mutual_information(fixed, moving, T, samples=None, bins=50):
    return mi_of_histogram(joint_histogram(fixed, moving, T, samples, bins))


def sincospi(t):
    """(sinpi(t), cospi(t)) of float64 t with few significant bits: the reduction to |r| <= 1/4 is exact."""
    t = np.asarray(t, np.float64)
    k = np.rint(2.0 * t)
    r = t - k / 2.0
    s, c = np.sin(np.pi * r), np.cos(np.pi * r)
    q = k.astype(np.int64) % 4
    return np.choose(q, [s, c, -s, -c]), np.choose(q, [c, -s, -c, s])


def normals(iterations, P, seed=0, first_iteration=0):
    """[iterations,P,6]: Box-Muller on the Philox words of counter (iteration, pair, draw, TAG_NORMAL)."""
    it, p, d = np.meshgrid(np.arange(iterations, dtype=np.uint64) + np.uint64(first_iteration), np.arange(P, dtype=np.uint64),
                           np.arange(3, dtype=np.uint64), indexing="ij")
    r = philox4x32_10([it & np.uint64(MASK), p, d, np.full(it.shape, TAG_NORMAL, np.uint64)], [seed & MASK, (seed >> 32) & MASK])
    u1 = (r[0].astype(np.float64) + 0.5) * 2.0 ** -32
    u2 = (r[1].astype(np.float64) + 0.5) * 2.0 ** -32
    rad = np.sqrt(-2.0 * np.log(u1))
    s, c = sincospi(2.0 * u2)
    return np.stack([rad * c, rad * s], axis=-1).reshape(iterations, P, 6)


def _matvec(A, n):
    out = []
    for i in range(6):
        v = A[i][0] * n[0]
        for j in range(1, 6):
            v += A[i][j] * n[j]
        out.append(v)
    return out


def register(fixed, moving, iterations, variates, samples=None, bins=50, initial_radius=6.25e-3, growth=1.05, epsilon=1.5e-6, T0=None,
             pair=0):
    """The (1+1) evolution strategy of one pair, ``iterations`` evaluations.  variates: [>= iterations, P, 6]; row t, pair ``pair`` makes
    the child of evaluation t + 1.  -> dict(x [6], T [2,3], A [6,6], f, iterations, accepted, status, margins: |MI - f| / f of every
    decision, values: the MI of every evaluation)."""
    x = [0.0] * 6 if T0 is None else [float(v) - (1.0 if j in (0, 4) else 0.0) for j, v in enumerate(np.asarray(T0, np.float64).ravel())]
    A = [[initial_radius if i == j else 0.0 for j in range(6)] for i in range(6)]
    shrink = math.sqrt(math.sqrt(1.0 / growth))
    child, n = list(x), [0.0] * 6
    f, accepted, status, done = 0.0, 0, 0, 0
    margins, values = [], []
    fixed, moving = np.asarray(fixed, np.float32), np.asarray(moving, np.float32)
    if not (fixed.max() > fixed.min() and moving.max() > moving.min()):
        return {"x": np.array(x), "A": np.array(A), "f": 0.0, "iterations": 0, "accepted": 0, "status": DEGENERATE, "margins": [], "values": []}
    for t in range(iterations):
        T = np.array([[1.0 + child[0], child[1], child[2]], [child[3], 1.0 + child[4], child[5]]])
        mi = mutual_information(fixed, moving, T, samples, bins)
        values.append(mi)
        done = t + 1
        if t == 0:
            f = mi
        else:
            margins.append(abs(mi - f) / f if f else np.inf)
            accept = mi > f
            if accept:
                x, f, accepted = list(child), mi, accepted + 1
            nn = 0.0
            for j in range(6):
                nn += n[j] * n[j]
            if nn > 0.0:
                c = ((growth if accept else shrink) - 1.0) / nn
                d = _matvec(A, n)
                A = [[A[i][j] + (c * d[i]) * n[j] for j in range(6)] for i in range(6)]
            fro = 0.0
            for i in range(6):
                for j in range(6):
                    fro += A[i][j] * A[i][j]
            if math.sqrt(fro) < epsilon:
                status = CONVERGED
                break
        if t >= len(variates):
            status = EXHAUSTED
            break
        n = [float(v) for v in variates[t][pair]]
        v = _matvec(A, n)
        child = [x[i] + v[i] for i in range(6)]
    xa = np.array(x)
    return {"x": xa, "T": (xa + np.array([1.0, 0, 0, 0, 1.0, 0])).reshape(2, 3), "A": np.array(A), "f": f, "iterations": done,
            "accepted": accepted, "status": status, "margins": margins, "values": values}


# ---- onto the middle image ---------------------------------------------------------------------------------------------------------

def _hom(t):
    t = [float(v) for v in np.asarray(t, np.float64).ravel()]
    return [t[0:3], t[3:6], [0.0, 0.0, 1.0]]


def _nan3():
    return [[math.nan] * 3, [math.nan] * 3, [0.0, 0.0, 1.0]]


def _mul3(a, b):
    return [[(a[i][0] * b[0][k] + a[i][1] * b[1][k]) + a[i][2] * b[2][k] for k in range(3)] for i in range(3)]


def _finite6(t):
    return all(math.isfinite(float(v)) for v in np.asarray(t, np.float64).ravel())


def _regular6(t):
    if not _finite6(t):
        return False
    a, b, _, d, e, _ = (float(v) for v in np.asarray(t, np.float64).ravel())
    det = a * e - b * d
    return math.isfinite(det) and det != 0.0


def _inv3(t):
    if not _regular6(t):
        return _nan3()
    a, b, c, d, e, f = (float(v) for v in np.asarray(t, np.float64).ravel())
    det = a * e - b * d
    return [[e / det, -b / det, (b * f - c * e) / det], [-d / det, a / det, (c * d - a * f) / det], [0.0, 0.0, 1.0]]


def inverse(T):
    return np.array(_inv3(T)[:2])


def chain_to_middle(T_pairs, middle=None):
    T_pairs = np.asarray(T_pairs, np.float64).reshape(-1, 2, 3)
    N = len(T_pairs) + 1
    middle = N // 2 if middle is None else middle
    C = np.empty((N, 2, 3))
    C[middle] = identity()
    cur = _hom(identity())
    with np.errstate(invalid="ignore"):
        for j in range(middle + 1, N):
            cur = _mul3(_hom(T_pairs[j - 1]), cur) if _regular6(T_pairs[j - 1]) else _nan3()
            C[j] = np.array(cur[:2])
        cur = _hom(identity())
        for j in range(middle - 1, -1, -1):
            cur = _mul3(_inv3(T_pairs[j]), cur)
            C[j] = np.array(cur[:2])
    return C


def common_limits(C, H, W):
    C = np.asarray(C, np.float64).reshape(-1, 2, 3)
    cx, cy, h = geometry(H, W)
    left, top, right, bottom = 0.0, 0.0, float(W - 1), float(H - 1)
    X, Y = [0.0, W - 1.0, W - 1.0, 0.0], [0.0, 0.0, H - 1.0, H - 1.0]
    for Cj in C:
        D = _inv3(Cj)
        xs = [(D[0][0] * (X[k] - cx) + D[0][1] * (Y[k] - cy)) + (D[0][2] * h + cx) for k in range(4)]
        ys = [(D[1][0] * (X[k] - cx) + D[1][1] * (Y[k] - cy)) + (D[1][2] * h + cy) for k in range(4)]
        if not all(math.isfinite(v) for v in xs + ys):
            return np.zeros(4, np.int32)
        left, right = max(left, math.ceil(max(xs[0], xs[3]))), min(right, math.floor(min(xs[1], xs[2])))
        top, bottom = max(top, math.ceil(max(ys[0], ys[1]))), min(bottom, math.floor(min(ys[2], ys[3])))
    w, hh = right - left + 1, bottom - top + 1
    return np.array([min(left, W - 1), min(top, H - 1), max(w, 0), max(hh, 0)], np.int32)


def warp_stack(stack, T_pairs, middle=None, fill=0.0):
    return warp(stack, chain_to_middle(T_pairs, middle), fill)


def corner_error(Ta, Tb, H, W):
    """The largest displacement, in pixels, of the four image corners between the pull maps Ta and Tb."""
    X, Y = np.array([0.0, W - 1, W - 1, 0]), np.array([0.0, 0, H - 1, H - 1])
    xa, ya = pull(Ta, H, W, X, Y)
    xb, yb = pull(Tb, H, W, X, Y)
    return float(np.hypot(xa - xb, ya - yb).max())


def pyramid_coordinates(W):
    """(the normalised coordinates of the coarse pixels of a factor-2 level, those of the fine points 2X + 1/2 they stand at)."""
    cf, hf = (W - 1) / 2, W / 2
    cc, hc = (W // 2 - 1) / 2, W / 4
    X = np.arange(W // 2, dtype=np.float64)
    return (X - cc) / hc, (2 * X + 0.5 - cf) / hf


# ---- inputs shared by tests/test_affine.py and tests/test_affine_gpu.py --------------------------------------------------------------

def sample_field(field, T, H, W, origin):
    """The [H,W] window of ``field`` whose top-left pixel is ``origin`` = (x, y), sampled bilinearly at the pull map T of the window."""
    yy, xx = np.mgrid[0:H, 0:W]
    xs, ys = pull(T, H, W, xx, yy)
    fx, fy, p00, p01, p10, p11, _ = _taps(np.asarray(field, np.float32), xs + origin[0], ys + origin[1], 0.0)
    return bilinear(fx, fy, p00, p01, p10, p11)


def invert_contrast(m, top):
    """(1 - m / top)^1.5: the contrast reversed, and not linearly."""
    return ((1.0 - np.asarray(m, np.float64) / top) ** 1.5).astype(np.float32)


_recovery = {}


def recovery_inputs():
    """(fixed, moving, T_true): the ``truth`` of synthetic_pair(1, 128, 128, seed=5); fixed is its central 64 x 64 window, moving the
    same field sampled through rotation 2 degrees, scale 1.02 and shift (1.5, -2) px, then mapped through (1 - m)^1.5 (m relative to the
    field's maximum, 0.898, so that the base is not negative).  The pull map that aligns moving with fixed is the INVERSE of the
    sampling transform.  The four corners move by up to 4.16 px between the identity and T_true."""
    if not _recovery:
        from tests.synth_inputs import synthetic_pair

        field = synthetic_pair(1, 128, 128, seed=5)[1][0, :, :, 0]
        sampling = similarity(2.0, 1.02, (1.5, -2.0), 64, 64)
        moving = invert_contrast(sample_field(field, sampling, 64, 64, (32, 32)), float(field.max()))
        _recovery["v"] = (field[32:96, 32:96].copy(), moving, inverse(sampling))
    return _recovery["v"]


def recovery_run(iterations=600, seed=0):
    """The restatement's run on recovery_inputs with the Philox normals of ``seed``.  Cached."""
    key = ("run", iterations, seed)
    if key not in _recovery:
        fixed, moving, _ = recovery_inputs()
        _recovery[key] = register(fixed, moving, iterations, normals(iterations, 1, seed))
    return _recovery[key]
