"""CPU restatements of the classical baseline filters for the tests (emdenoise.filters, csrc/filters.hip).

Gaussian, median and Wiener in float64 are thin wrappers over scipy (ndimage.gaussian_filter / median_filter with mode="mirror",
which is reflect-101, and signal.wiener); the bilateral filter and Chambolle's iteration are written here from their formulas.
Every function takes one image ``[H,W]`` or a batch ``[B,H,W]`` (each image on its own) and a ``dtype``: numpy.float64 is the
reference the device results are checked against; numpy.float32 is used only as a yardstick -- its own distance from the float64
result sets the tolerances.  scipy accumulates in double whatever the input's type, so the float32 yardsticks of the Gaussian
and of Wiener are the same formulas spelled out with every array in float32 (``*_restated``; tests/test_filters.py checks that
in float64 they are scipy's results)."""
import warnings

import numpy as np
import scipy.ndimage as ndi
import scipy.signal as sig

TAU = 0.25


def _each(fn, x, dtype):
    x = np.asarray(x)
    if x.ndim == 2:
        return fn(x.astype(dtype))
    return np.stack([fn(im.astype(dtype)) for im in x])


def gaussian_restated(x, sigma=1.5, ksize=3, dtype=np.float64):
    """taps exp(-i^2 / (2 sigma^2)) / sum, i = -r .. r, correlated along the rows, then along the columns, mirror border; all in dtype."""
    r = ksize // 2
    i = np.arange(-r, r + 1, dtype=np.float64)
    g = np.exp(-(i * i) / (2.0 * float(sigma) ** 2))
    g = (g / g.sum()).astype(dtype)

    def f(im):
        H, W = im.shape
        p = np.pad(im, ((0, 0), (r, r)), mode="reflect")
        h = np.zeros_like(im)
        for k in range(ksize):
            h += g[k] * p[:, k:k + W]
        p = np.pad(h, ((r, r), (0, 0)), mode="reflect")
        v = np.zeros_like(im)
        for k in range(ksize):
            v += g[k] * p[k:k + H, :]
        return v

    return _each(f, x, dtype)


def gaussian(x, sigma=1.5, ksize=3, dtype=np.float64):
    if dtype != np.float64:
        return gaussian_restated(x, sigma, ksize, dtype)
    return _each(lambda im: ndi.gaussian_filter(im, sigma, mode="mirror", radius=ksize // 2), x, dtype)


def median(x, ksize=3):
    """Exact in any dtype: the result is one of the inputs."""
    x = np.asarray(x)
    f = lambda im: ndi.median_filter(im, size=ksize, mode="mirror")
    return f(x) if x.ndim == 2 else np.stack([f(im) for im in x])


def _local_moments(im, ksize):
    """(mean, variance) over the ksize x ksize window of the zero-padded image, as scipy.signal.wiener forms them, in im's dtype."""
    dtype = im.dtype.type
    r, (H, W) = ksize // 2, im.shape

    def box(a):
        p = np.pad(a, r)
        s = np.zeros_like(a)
        for dy in range(ksize):
            for dx in range(ksize):
                s += p[dy:dy + H, dx:dx + W]
        return s / dtype(ksize * ksize)

    m = box(im)
    return m, box(im * im) - m * m


def wiener_restated(x, ksize=5, noise=None, dtype=np.float64, return_noise=False):
    """scipy.signal.wiener's formulas with every array in dtype: res = (x - m) (1 - n / v) + m; where(v < n, m, res); noise=None:
    n = mean(v)."""
    used = []

    def f(im):
        m, v = _local_moments(im, ksize)
        n = v.mean(dtype=dtype) if noise is None else dtype(noise)
        used.append(n)
        with np.errstate(divide="ignore", invalid="ignore"):
            res = (im - m) * (dtype(1.0) - n / v) + m
        return np.where(v < n, m, res)

    y = _each(f, x, dtype)
    return (y, np.array(used)) if return_noise else y


def wiener(x, ksize=5, noise=None, dtype=np.float64, return_noise=False):
    """float64: scipy.signal.wiener itself (return_noise: the n it used, restated -- scipy does not return it)."""
    if dtype != np.float64:
        return wiener_restated(x, ksize, noise, dtype, return_noise)

    def f(im):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)     # 0 / 0 where the local variance is 0
            return sig.wiener(im, mysize=ksize, noise=noise)

    y = _each(f, x, dtype)
    return (y, wiener_restated(x, ksize, noise, dtype, True)[1]) if return_noise else y


def disc_offsets(d):
    """(dy, dx) of the taps inside cv2's circular support: dx^2 + dy^2 <= (d // 2)^2."""
    r = d // 2
    return [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dx * dx + dy * dy <= r * r]


def bilateral(x, d=5, sigma_color=0.1, sigma_space=1.5, dtype=np.float64):
    """out[p] = sum_q w x[q] / sum_q w, w = exp(-(dx^2 + dy^2) / (2 sigma_space^2)) exp(-(x[q] - x[p])^2 / (2 sigma_color^2)) over
    the disc, mirror border; all arithmetic in `dtype`."""
    r = d // 2
    two_ss, two_sc = dtype(2.0 * sigma_space * sigma_space), dtype(2.0) * dtype(sigma_color) * dtype(sigma_color)

    def f(im):
        H, W = im.shape
        p = np.pad(im, r, mode="reflect")
        num, den = np.zeros_like(im), np.zeros_like(im)
        for dy, dx in disc_offsets(d):
            q = p[r + dy:r + dy + H, r + dx:r + dx + W]
            df = q - im
            w = np.exp(-dtype(dx * dx + dy * dy) / two_ss).astype(dtype) * np.exp(-(df * df) / two_sc)
            num += w * q
            den += w
        return num / den

    return _each(f, x, dtype)


def disc_gaussian(x, d=5, sigma_space=1.5, dtype=np.float64):
    """The bilateral filter without its range term: the normalised correlation with the disc-masked Gaussian, mirror border."""
    r = d // 2
    k = np.zeros((d, d), dtype)
    for dy, dx in disc_offsets(d):
        k[dy + r, dx + r] = np.exp(-dtype(dx * dx + dy * dy) / dtype(2.0 * sigma_space * sigma_space))
    k /= k.sum()
    return _each(lambda im: ndi.correlate(im, k, mode="mirror"), x, dtype)


def _tv_u(im, p1, p2):
    d = -p1 - p2
    d[1:, :] += p1[:-1, :]
    d[:, 1:] += p2[:, :-1]
    return im + d


def tv_chambolle(x, weight=0.1, n_iter=50, dtype=np.float64):
    """p = 0; n_iter times: u = x + div p; g = forward differences of u (0 past the last row / column); p <- (p - tau g) / (1 +
    (tau / weight) |g|), tau = 0.25.  The result is the last u (n_iter = 1: x); the last iteration's p update is not needed."""
    tau, tw = dtype(TAU), dtype(TAU) / dtype(weight)

    def f(im):
        p1, p2 = np.zeros_like(im), np.zeros_like(im)
        for it in range(n_iter):
            u = _tv_u(im, p1, p2)
            if it == n_iter - 1:
                return u
            g1, g2 = np.zeros_like(im), np.zeros_like(im)
            g1[:-1, :] = u[1:, :] - u[:-1, :]
            g2[:, :-1] = u[:, 1:] - u[:, :-1]
            den = dtype(1.0) + tw * np.sqrt(g1 * g1 + g2 * g2)
            p1 = (p1 - tau * g1) / den
            p2 = (p2 - tau * g2) / den

    return _each(f, x, dtype)


def total_variation(u):
    """sum |grad u| with the forward differences of the iteration."""
    u = np.asarray(u, np.float64)
    g1, g2 = np.zeros_like(u), np.zeros_like(u)
    g1[..., :-1, :] = u[..., 1:, :] - u[..., :-1, :]
    g2[..., :, :-1] = u[..., :, 1:] - u[..., :, :-1]
    return float(np.sqrt(g1 * g1 + g2 * g2).sum())
