"""Classical baseline filters on the device (csrc/filters.hip) and the denoiser comparison table: the methods the
reference's evaluation compares its networks with (misc_py/err_hist_maker.py:26-45) and its ground-truth blur
(misc_py/blur_images.py:13, ``gaussian(x, 1.5, 3)``).

Images are float32 ``[B,H,W,1]`` (or ``[B,H,W]`` / ``[H,W]``); every image of a batch is filtered on its own.  numpy in -> numpy
out; torch CUDA tensor in -> device tensor of the same shape out, on the current stream, with no host synchronisation (the
conventions of ``emdenoise.metrics``).  Python here only shapes buffers: every number comes from a HIP kernel.  "Mirror" border
= reflect-101 (cv2's default), which needs the window radius < min(H, W)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, metrics
from .metrics import _dims, _images, _p, _ws, gaussian_taps

LABELS = ["Unfiltered", "Gaussian", "Bilateral", "Median", "Wiener", "Chambolle"]   # err_hist_maker.py:27 without "Wavelet"


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


def baseline_table(lq, truth, extra=None, clip=False, **filter_args):
    """The reference's comparison array (misc_py/err_hist_maker.py:26-45) -> ``(data, labels)``: ``data`` float32 ``[N, M, 2]`` with
    ``data[n, m, 0]`` the MSE of method m's output for image n against ``truth`` and ``data[n, m, 1]`` its SSIM (``emdenoise.ssim(...,
    per_image=True)``); ``labels`` = ["Unfiltered", "Gaussian", "Bilateral", "Median", "Wiener", "Chambolle"], the reference's order,
    then the keys of ``extra``.  The reference's "Wavelet" column is not built: it needs a wavelet-transform pipeline of its own.

    ``extra``: ``{label: callable(lq) -> denoised}`` appended as further rows, e.g. ``{"D": den.denoise_batch}``: one call then gives
    the paper's comparison.  ``filter_args``: keyword arguments per filter, keyed by its function name, e.g. ``gaussian={"sigma": 1.0},
    tv_chambolle={"weight": 0.2}``.  clip=True clips every method's output to [0, 1] before it is scored (default: scored as it is).
    Every number is computed on the device: numpy inputs are moved there once, every method and both metrics run on the device
    tensors, and only ``data`` comes back; numpy in -> numpy out, CUDA tensors in -> a device tensor."""
    import torch

    unknown = set(filter_args) - {"gaussian", "bilateral", "median", "wiener", "tv_chambolle"}
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
