"""Classical baseline filters on the device (csrc/filters.hip) and the denoiser comparison table: the methods the
reference's evaluation compares its networks with (misc_py/err_hist_maker.py:26-45) and its ground-truth blur
(misc_py/blur_images.py:13, ``gaussian(x, 1.5, 3)``).

Images are float32 ``[B,H,W,1]`` (or ``[B,H,W]`` / ``[H,W]``); every image of a batch is filtered on its own.  numpy in -> numpy
out; torch CUDA tensor in -> device tensor of the same shape out, on the current stream, with no host synchronisation (the
conventions of ``emdenoise.metrics``).  Python here only shapes buffers: every number comes from a HIP kernel.  "Mirror" border
= reflect-101 (cv2's default), which needs the window radius < min(H, W).

``wavedec2`` / ``waverec2`` / ``denoise_wavelet`` (csrc/wavelet.hip) are the 2-D orthogonal wavelet transform with
the half-sample symmetric border and the reference table's "Wavelet" method, built as ``skimage.restoration.denoise_wavelet``'s
arithmetic at its defaults from the formulas in include/emdenoise.h (neither skimage nor pywt is used)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, metrics
from .metrics import _dims, _images, _p, _ws, gaussian_taps

LABELS = ["Unfiltered", "Gaussian", "Bilateral", "Median", "Wiener", "Chambolle"]   # err_hist_maker.py:27 without "Wavelet"
REFERENCE_LABELS = ["Unfiltered", "Gaussian", "Bilateral", "Median", "Wiener", "Wavelet", "Chambolle"]   # err_hist_maker.py:27
WAVELET_METHODS = {"BayesShrink": 0, "VisuShrink": 1}                               # EMD_WAVELET_BAYES, EMD_WAVELET_VISU


def _shaped(y, like, as_np):
    """The filtered [B,H,W] tensor in the shape (and kind) of the argument."""
    y = y.reshape(tuple(like.shape))
    return y.cpu().numpy() if as_np else y


def _mirror_ok(name, radius, x):
    """Checked on the argument's shape, before anything is moved to the device."""
    _, H, W = _dims(x)
    if min(H, W) <= radius:
        raise ValueError(f"{name}: the mirror border needs radius < min(H, W) (radius {radius}, image {H} x {W})")


def gaussian(x, sigma=1.5, ksize=3):
    """Separable Gaussian blur, taps exp(-i^2 / (2 sigma^2)) / sum for i = -ksize//2 .. ksize//2 (ksize odd, 3..15), mirror border.
    The defaults are ``cv2.GaussianBlur(img, (3,3), 1.5)`` (blur_images.py:13)."""
    import torch

    taps = gaussian_taps(ksize, sigma)
    _mirror_ok("gaussian", int(ksize) // 2, x)
    xd, as_np = _images(x)
    B, H, W = xd.shape
    out = torch.empty_like(xd)
    _lib.check(_lib.load().emd_filter_gaussian_f32(_p(xd), _p(out), B, H, W, taps.ctypes.data_as(C.c_void_p), int(ksize),
                                                   _lib.stream_ptr()), "emd_filter_gaussian_f32")
    return _shaped(out, x, as_np)


def median(x, ksize=3):
    """Median of the ksize x ksize window (3 or 5), mirror border; every output is one of the input values, bit for bit."""
    import torch

    ksize = int(ksize)
    if ksize not in (3, 5):
        raise ValueError(f"median: ksize must be 3 or 5 (got {ksize})")
    _mirror_ok("median", ksize // 2, x)
    xd, as_np = _images(x)
    B, H, W = xd.shape
    out = torch.empty_like(xd)
    _lib.check(_lib.load().emd_filter_median_f32(_p(xd), _p(out), B, H, W, ksize, _lib.stream_ptr()), "emd_filter_median_f32")
    return _shaped(out, x, as_np)


def bilateral(x, d=5, sigma_color=0.1, sigma_space=1.5):
    """``cv2.bilateralFilter``'s arithmetic: the taps within the disc dx^2 + dy^2 <= (d//2)^2, weight exp(-(dx^2 + dy^2) / (2
    sigma_space^2)) exp(-(x[q] - x[p])^2 / (2 sigma_color^2)), normalised; d odd, 3..9; mirror border."""
    import torch

    d = int(d)
    if d < 3 or d > 9 or d % 2 == 0:
        raise ValueError(f"bilateral: d must be odd, 3..9 (got {d})")
    if not (sigma_color > 0 and sigma_space > 0):
        raise ValueError("bilateral: the sigmas must be positive")
    _mirror_ok("bilateral", d // 2, x)
    xd, as_np = _images(x)
    B, H, W = xd.shape
    out = torch.empty_like(xd)
    _lib.check(_lib.load().emd_filter_bilateral_f32(_p(xd), _p(out), B, H, W, d, C.c_float(sigma_color), C.c_float(sigma_space),
                                                    _lib.stream_ptr()), "emd_filter_bilateral_f32")
    return _shaped(out, x, as_np)


def wiener(x, ksize=5, noise=None, return_noise=False):
    """``scipy.signal.wiener(x, ksize, noise)``: local mean m and variance v over the ksize x ksize window of the zero-padded image
    (ksize odd, 3..9); m + (x - m) (1 - n / v) where v >= n, else m.  noise=None: n of each image is the mean of its own v.  Where
    scipy divides 0 by 0 (v = n = 0, a constant image) the result here is m.  return_noise=True: the pair (filtered, n ``[B]``)."""
    import torch

    ksize = int(ksize)
    if ksize < 3 or ksize > 9 or ksize % 2 == 0:
        raise ValueError(f"wiener: ksize must be odd, 3..9 (got {ksize})")
    if noise is not None and not noise >= 0:
        raise ValueError("wiener: noise must be None (estimate it) or >= 0")
    xd, as_np = _images(x)
    B, H, W = xd.shape
    lib = _lib.load()
    out = torch.empty_like(xd)
    used = torch.empty(B, dtype=torch.float32, device=xd.device)
    nbytes, ws = 0, None
    if noise is None:
        nbytes = lib.emd_filter_wiener_workspace_bytes(B, H, W)
        ws = _ws(nbytes, xd.device)
    _lib.check(lib.emd_filter_wiener_f32(_p(xd), _p(out), B, H, W, ksize, C.c_float(-1.0 if noise is None else noise), _p(used), _p(ws),
                                         nbytes, _lib.stream_ptr()), "emd_filter_wiener_f32")
    y = _shaped(out, x, as_np)
    return (y, used.cpu().numpy() if as_np else used) if return_noise else y


def tv_chambolle(x, weight=0.1, n_iter=50):
    """Total-variation denoising by Chambolle's dual projection with a fixed number of iterations (tau = 0.25; no stopping rule, so
    the call can be captured): the arithmetic is spelled out at ``emd_filter_tv_f32`` in include/emdenoise.h.  A larger weight
    smooths more; n_iter=1 returns x."""
    import torch

    n_iter = int(n_iter)
    if n_iter < 1:
        raise ValueError("tv_chambolle: n_iter must be >= 1")
    if not weight > 0:
        raise ValueError("tv_chambolle: weight must be positive")
    xd, as_np = _images(x)
    B, H, W = xd.shape
    lib = _lib.load()
    out = torch.empty_like(xd)
    nbytes = lib.emd_filter_tv_workspace_bytes(B, H, W)
    ws = _ws(nbytes, xd.device)
    _lib.check(lib.emd_filter_tv_f32(_p(xd), _p(out), B, H, W, C.c_float(weight), n_iter, _p(ws), nbytes, _lib.stream_ptr()),
               "emd_filter_tv_f32")
    return _shaped(out, x, as_np)


# ---- wavelets (csrc/wavelet.hip) ---------------------------------------------------------------------------------------------

def wavelet_taps(wavelet):
    """Reconstruction low-pass taps rec_lo (float64, even count, 2..8) of a named wavelet ("haar" = "db1", "db2") or of an array
    holding the taps of any other orthogonal filter; the other three filters follow from them (include/emdenoise.h)."""
    if isinstance(wavelet, str):
        if wavelet in ("haar", "db1"):
            return np.array([1.0, 1.0]) / np.sqrt(2.0)
        if wavelet == "db2":
            s3 = np.sqrt(3.0)
            return np.array([1.0 + s3, 3.0 + s3, 3.0 - s3, 1.0 - s3]) / (4.0 * np.sqrt(2.0))
        raise ValueError(f"wavelet: unknown name {wavelet!r} (\"haar\", \"db1\", \"db2\", or an array of reconstruction low-pass taps)")
    taps = np.ascontiguousarray(wavelet, dtype=np.float64)
    if taps.ndim != 1 or taps.size < 2 or taps.size > 8 or taps.size % 2:
        raise ValueError(f"wavelet: the tap count must be even, 2..8 (got shape {taps.shape})")
    if not np.isfinite(taps).all():
        raise ValueError("wavelet: the taps must be finite")
    return taps


def wavelet_max_levels(H, W, ntaps):
    """floor(log2(min(H, W) / (ntaps - 1))): the deepest decomposition allowed (< 1: the image is too small for the filter)."""
    k = -1
    while (ntaps - 1) * 2 ** (k + 1) <= min(H, W):
        k += 1
    return k


def _wavelet_args(name, wavelet, levels, H, W):
    """(taps, levels) checked on the shape alone, before anything is moved to the device; levels=None is skimage's rule."""
    taps = wavelet_taps(wavelet)
    top = wavelet_max_levels(H, W, taps.size)
    if top < 1 or max(H, W) > 32768:
        raise ValueError(f"{name}: an image of {H} x {W} allows no level of a {taps.size}-tap wavelet (needs min(H, W) >= "
                         f"{2 * (taps.size - 1)}, H, W <= 32768)")
    if levels is None:
        return taps, max(top - 3, 1)
    if int(levels) != levels or not 1 <= levels <= top:
        raise ValueError(f"{name}: levels must be 1..{top} for an image of {H} x {W} and {taps.size} taps (got {levels})")
    return taps, int(levels)


def _layout(H, W, ntaps, levels):
    """(floats per image, [(offset, rows, cols)] of cA_n, ad_n, da_n, dd_n, ..., dd_1) from the library."""
    bands = (C.c_long * (3 * (1 + 3 * levels)))()
    total = _lib.load().emd_wavelet_pyramid_floats(H, W, ntaps, levels, bands)
    if not total:
        raise ValueError(f"wavelet: no pyramid for an image of {H} x {W}, {ntaps} taps, {levels} levels")
    return int(total), [tuple(bands[3 * i:3 * i + 3]) for i in range(1 + 3 * levels)]


def _taps_p(taps):
    return taps.ctypes.data_as(C.c_void_p)


def wavedec2(x, wavelet="db1", levels=None):
    """2-D wavelet decomposition with the half-sample symmetric border (pywt's default mode) -> ``[cA_n, {"ad","da","dd"}_n, ...,
    {...}_1]``, coarsest first: ``ad`` is low along H and high along W, ``da`` high along H and low along W, ``dd`` high along both;
    a band of an axis of length N has (N + L - 1) // 2 samples.  ``wavelet``: "haar" = "db1", "db2", or the reconstruction low-pass
    taps of any orthogonal filter of up to 8 taps.  ``levels``: 1..floor(log2(min(H,W) / (L-1))); None is skimage's rule, that
    bound minus 3 (at least 1).  Bands are ``[B,h,w]`` (``[h,w]`` for an ``[H,W]`` image, ``[B,h,w,1]`` for ``[B,H,W,1]``); for a
    tensor they are views of one packed buffer."""
    import torch

    B, H, W = _dims(x)
    taps, levels = _wavelet_args("wavedec2", wavelet, levels, H, W)
    xd, as_np = _images(x)
    lib = _lib.load()
    total, bands = _layout(H, W, taps.size, levels)
    pyr = torch.empty((B, total), dtype=torch.float32, device=xd.device)
    nbytes = lib.emd_wavelet_workspace_bytes(B, H, W, taps.size, levels)
    ws = _ws(nbytes, xd.device)
    _lib.check(lib.emd_wavelet_forward_f32(_p(xd), _p(pyr), B, H, W, _taps_p(taps), taps.size, levels, _p(ws), nbytes, _lib.stream_ptr()),
               "emd_wavelet_forward_f32")
    nd = len(np.shape(x))

    def band(i):
        off, h, w = bands[i]
        v = pyr[:, off:off + h * w].reshape((h, w) if nd == 2 else (B, h, w, 1) if nd == 4 else (B, h, w))
        return v.cpu().numpy() if as_np else v

    return [band(0)] + [{k: band(1 + 3 * i + j) for j, k in enumerate(("ad", "da", "dd"))} for i in range(levels)]


def waverec2(coeffs, wavelet, shape):
    """The inverse of ``wavedec2``: ``coeffs`` as it returns them, ``shape`` the image's (``[H,W]``, ``[B,H,W]`` or ``[B,H,W,1]``: the
    result has that shape).  Synthesis along W, then along H; a level's result is cropped to the shape of the level below."""
    import torch

    shape = tuple(int(v) for v in shape)
    B, H, W = _dims(np.empty(shape, np.bool_))
    levels = len(coeffs) - 1
    taps, levels = _wavelet_args("waverec2", wavelet, levels, H, W)
    total, bands = _layout(H, W, taps.size, levels)
    flat = [coeffs[0]] + [c[k] for c in coeffs[1:] for k in ("ad", "da", "dd")]
    for v, (_, h, w) in zip(flat, bands):
        want = (h, w) if len(shape) == 2 else (B, h, w, 1) if len(shape) == 4 else (B, h, w)
        if tuple(np.shape(v)) != want:
            raise ValueError(f"waverec2: a band of shape {tuple(np.shape(v))} where the image {shape} has {want}")
    as_np = not isinstance(flat[0], torch.Tensor)
    device = torch.device("cuda", torch.cuda.current_device()) if as_np else flat[0].device
    pyr = torch.empty((B, total), dtype=torch.float32, device=device)
    for v, (off, h, w) in zip(flat, bands):
        t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)) if as_np else v
        pyr[:, off:off + h * w].copy_(t.reshape(B, h * w))
    lib = _lib.load()
    out = torch.empty((B, H, W), dtype=torch.float32, device=device)
    nbytes = lib.emd_wavelet_workspace_bytes(B, H, W, taps.size, levels)
    ws = _ws(nbytes, device)
    _lib.check(lib.emd_wavelet_inverse_f32(_p(pyr), _p(out), B, H, W, _taps_p(taps), taps.size, levels, _p(ws), nbytes, _lib.stream_ptr()),
               "emd_wavelet_inverse_f32")
    out = out.reshape(shape)
    return out.cpu().numpy() if as_np else out


def denoise_wavelet(x, wavelet="db1", levels=None, method="BayesShrink", sigma=None, return_sigma=False):
    """Wavelet shrinkage, ``skimage.restoration.denoise_wavelet``'s arithmetic at its defaults: ``wavedec2``, a soft threshold
    sign(d) max(|d| - t, 0) on every detail band of every level (never on cA), ``waverec2``.  method "BayesShrink": t = var /
    sqrt(max(mean(d^2) - var, float32's epsilon)) per band, var = sigma^2; "VisuShrink": t = sigma sqrt(2 ln(H W)) for all.
    sigma=None: per image, median(|dd_1| over its non-zero coefficients) / 0.6745 with dd_1 the finest diagonal band, an exact
    median found on the device with no host synchronisation (an image without a non-zero coefficient: 0, and it comes back through
    the transform unthresholded).  ``wavelet`` and ``levels`` as in ``wavedec2``.  return_sigma=True: the pair (denoised, sigma
    ``[B]``).  Hard thresholding is not built (it is discontinuous: its parity cannot be stated as a norm), and skimage's final clip
    to [0, 1] is not applied (``baseline_table(clip=True)`` clips).  Launches only, on the current stream: capturable."""
    import torch

    B, H, W = _dims(x)
    taps, levels = _wavelet_args("denoise_wavelet", wavelet, levels, H, W)
    if method not in WAVELET_METHODS:
        raise ValueError(f"denoise_wavelet: method must be one of {sorted(WAVELET_METHODS)} (got {method!r})")
    if sigma is not None and not (sigma >= 0 and np.isfinite(sigma)):
        raise ValueError("denoise_wavelet: sigma must be None (estimate it) or finite and >= 0")
    xd, as_np = _images(x)
    lib = _lib.load()
    out = torch.empty_like(xd)
    used = torch.empty(B, dtype=torch.float32, device=xd.device)
    nbytes = lib.emd_filter_wavelet_workspace_bytes(B, H, W, taps.size, levels)
    ws = _ws(nbytes, xd.device)
    _lib.check(lib.emd_filter_wavelet_f32(_p(xd), _p(out), B, H, W, _taps_p(taps), taps.size, levels, WAVELET_METHODS[method],
                                          C.c_float(-1.0 if sigma is None else sigma), _p(used), _p(ws), nbytes, _lib.stream_ptr()),
               "emd_filter_wavelet_f32")
    y = _shaped(out, x, as_np)
    return (y, used.cpu().numpy() if as_np else used) if return_sigma else y


def _clip01(y):
    """min(max(y, 0), 1) on the device, into a new tensor (y may be a buffer its maker keeps)."""
    import torch

    yd, as_np = _images(y)
    out = torch.empty_like(yd)
    _lib.check(_lib.load().emd_filter_clip01_f32(_p(yd), _p(out), C.c_long(yd.numel()), _lib.stream_ptr()), "emd_filter_clip01_f32")
    return _shaped(out, y, as_np)


def _upload(a, device=None):
    """-> (float32 CUDA tensor in a's own shape, was_numpy): the table moves its inputs to the device once."""
    t, is_np = _images(a, device)
    return t.reshape(tuple(np.shape(a))), is_np


def _mse_ssim(pred, truth):
    """Per-image (mse ``[N]``, ssim ``[N]``) of pred against truth, both from the fixed-order device reductions of the metrics."""
    _, mse = metrics.psnr(pred, truth, per_image=True, return_mse=True)
    return mse, metrics.ssim(pred, truth, per_image=True)


def baseline_table(lq, truth, extra=None, clip=False, reference_columns=False, **filter_args):
    """The reference's comparison array (misc_py/err_hist_maker.py:26-45) -> ``(data, labels)``: ``data`` float32 ``[N, M, 2]`` with
    ``data[n, m, 0]`` the MSE of method m's output for image n against ``truth`` and ``data[n, m, 1]`` its SSIM (``emdenoise.ssim(...,
    per_image=True)``); ``labels`` = ["Unfiltered", "Gaussian", "Bilateral", "Median", "Wiener", "Chambolle"], the reference's order,
    then the keys of ``extra``.  reference_columns=True: the reference's seven, ``REFERENCE_LABELS``, with "Wavelet"
    (``denoise_wavelet``) between "Wiener" and "Chambolle"; only then is the filter-argument key ``denoise_wavelet={...}`` accepted.

    ``extra``: ``{label: callable(lq) -> denoised}`` appended as further rows, e.g. ``{"D": den.denoise_batch}``: one call then gives
    the paper's comparison.  ``filter_args``: keyword arguments per filter, keyed by its function name, e.g. ``gaussian={"sigma": 1.0},
    tv_chambolle={"weight": 0.2}``.  clip=True clips every method's output to [0, 1] before it is scored (default: scored as it is).
    Every number is computed on the device: numpy inputs are moved there once, every method and both metrics run on the device
    tensors, and only ``data`` comes back; numpy in -> numpy out, CUDA tensors in -> a device tensor."""
    import torch

    unknown = set(filter_args) - {"gaussian", "bilateral", "median", "wiener", "tv_chambolle"} - ({"denoise_wavelet"} if reference_columns else set())
    if unknown:
        raise TypeError(f"baseline_table: unknown filter(s) {sorted(unknown)}")
    arg = lambda name: dict(filter_args.get(name) or {})
    methods = [("Unfiltered", lambda a: a),
               ("Gaussian", lambda a: gaussian(a, **arg("gaussian"))),
               ("Bilateral", lambda a: bilateral(a, **arg("bilateral"))),
               ("Median", lambda a: median(a, **arg("median"))),
               ("Wiener", lambda a: wiener(a, **arg("wiener"))),
               ("Chambolle", lambda a: tv_chambolle(a, **arg("tv_chambolle")))]
    assert [m[0] for m in methods] == LABELS
    if reference_columns:
        methods.insert(5, ("Wavelet", lambda a: denoise_wavelet(a, **arg("denoise_wavelet"))))
        assert [m[0] for m in methods] == REFERENCE_LABELS
    for label, fn in (extra or {}).items():
        if label in [m[0] for m in methods]:
            raise ValueError(f"baseline_table: the label {label!r} is taken")
        methods.append((str(label), fn))
    lq, np_lq = _upload(lq)
    truth, np_truth = _upload(truth, getattr(lq, "device", None))
    cols = []
    for label, fn in methods:
        y = fn(lq)
        if tuple(np.shape(y)) != tuple(np.shape(lq)):
            raise ValueError(f"baseline_table: {label} returned shape {tuple(np.shape(y))} for input {tuple(np.shape(lq))}")
        if clip and label != "Unfiltered":
            y = _clip01(y)
        mse, s = _mse_ssim(y, truth)
        stack = torch.stack if isinstance(mse, torch.Tensor) else np.stack
        cols.append(stack([mse, s], -1))                # [N, 2]
    stack = torch.stack if isinstance(cols[0], torch.Tensor) else np.stack
    data = stack(cols, 1)                               # [N, M, 2]
    if np_lq and np_truth and isinstance(data, torch.Tensor):
        data = data.cpu().numpy()
    return data, [m[0] for m in methods]
