"""Image-quality metrics on the device (csrc/ssim.hip): SSIM, MS-SSIM and PSNR, and the SSIM loss term with its
gradient -- the reference's ``_tf_fspecial_gauss`` / ``tf_ssim`` / ``tf_ms_ssim`` (misc_py/denoiser-multi-gpu.py:124-192) and the
term ``tower_loss += 1.0 - tf_ssim(out, truth)`` of its tower (:775).

Images are float32 ``[B,H,W,1]`` (or ``[B,H,W]`` / ``[H,W]``).  numpy in -> numpy / float out; torch CUDA tensor in -> device
tensor out, with no host synchronisation (the convention of ``denoise_images``).  Python here only shapes buffers: every number
comes from a HIP kernel."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)   # :171
MAX_SIZE = 15


def gaussian_taps(size=11, sigma=1.5):
    """The 1-D window g whose outer product g x g is ``_tf_fspecial_gauss(size, sigma)`` (:124-139): exp(-i^2 / (2 sigma^2)) for
    i = -size//2 + 1 .. size//2, divided by its sum (the 2-D window divided by its sum is the outer product of that)."""
    size = int(size)
    if size < 3 or size > MAX_SIZE or size % 2 == 0:
        raise ValueError(f"window size must be odd, 3..{MAX_SIZE} (got {size})")
    if not sigma > 0:
        raise ValueError("sigma must be positive")
    i = np.arange(-(size // 2), size // 2 + 1, dtype=np.float64)
    g = np.exp(-(i * i) / (2.0 * float(sigma) ** 2))
    return np.ascontiguousarray(g / g.sum(), dtype=np.float32)


def _taps_arg(taps):
    return taps.ctypes.data_as(C.c_void_p)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _images(a, device=None):
    """-> (float32 contiguous CUDA tensor [B,H,W], was_numpy).  A numpy array goes to ``device`` (default: the current one)."""
    import torch

    is_np = not isinstance(a, torch.Tensor)
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)) if is_np else a
    if t.dim() == 4:
        if t.shape[3] != 1:
            raise ValueError("single-channel images: [B,H,W,1]")
        t = t.reshape(t.shape[0], t.shape[1], t.shape[2])
    elif t.dim() == 2:
        t = t.reshape(1, t.shape[0], t.shape[1])
    elif t.dim() != 3:
        raise ValueError("images are [B,H,W,1], [B,H,W] or [H,W]")
    if not t.is_cuda:
        t = t.to(device if device is not None else torch.device("cuda", torch.cuda.current_device()))
    return t.to(dtype=torch.float32).contiguous(), is_np


def _dims(a):
    """(B, H, W) of an image argument, before anything is moved to the device."""
    shp = tuple(a.shape) if hasattr(a, "shape") else np.shape(a)
    if len(shp) == 4 and shp[3] == 1:
        return shp[:3]
    if len(shp) == 3:
        return shp
    if len(shp) == 2:
        return (1,) + shp
    raise ValueError("images are [B,H,W,1], [B,H,W] or [H,W]")


def _pair(a, b):
    import torch

    dev = b.device if isinstance(b, torch.Tensor) and b.is_cuda else None
    ta, np_a = _images(a, dev)
    tb, np_b = _images(b, ta.device)
    if ta.shape != tb.shape:
        raise ValueError(f"shapes differ: {tuple(ta.shape)} and {tuple(tb.shape)}")
    return ta, tb, np_a and np_b


def _ws(nbytes, device):
    import torch

    return torch.empty(max(int(nbytes), 16) // 8 + 1, dtype=torch.float64, device=device)


def _out(t, as_np, scalar=False):
    if not as_np:
        return t
    v = t.cpu().numpy()
    return float(v) if scalar else v


def ssim(a, b, cs_map=False, mean_metric=True, size=11, sigma=1.5, per_image=False):
    """``tf_ssim`` (:142-167).  mean_metric=True: the mean of ssim_map over the whole batch (or, with cs_map, the pair (mean
    ssim_map, mean cs_map)); per_image=True (not in the reference): each image's own mean(s), ``[B]``.  mean_metric=False: the
    map(s) ``[B, H-size+1, W-size+1, 1]``."""
    import torch

    taps = gaussian_taps(size, sigma)
    B, H, W = _dims(a)
    if H < size or W < size:
        raise ValueError(f"image {H} x {W} is smaller than the {size} x {size} window")
    x, y, as_np = _pair(a, b)
    lib = _lib.load()
    means = torch.empty((B + 1, 2), dtype=torch.float32, device=x.device)
    smap = cmap = None
    if not mean_metric:
        smap = torch.empty((B, H - size + 1, W - size + 1, 1), dtype=torch.float32, device=x.device)
        cmap = torch.empty_like(smap) if cs_map else None
    nbytes = lib.emd_ssim_workspace_bytes(B, H, W, size)
    ws = _ws(nbytes, x.device)
    _lib.check(lib.emd_ssim_f32(_p(x), _p(y), B, H, W, _taps_arg(taps), size, _p(means), _p(smap), _p(cmap), _p(ws), nbytes,
                                _lib.stream_ptr()), "emd_ssim_f32")
    if not mean_metric:
        return (_out(smap, as_np), _out(cmap, as_np)) if cs_map else _out(smap, as_np)
    sel = means[:B] if per_image else means[B]
    if cs_map:
        return _out(sel[..., 0], as_np, not per_image), _out(sel[..., 1], as_np, not per_image)
    return _out(sel[..., 0], as_np, not per_image)


def ms_ssim(a, b, mean_metric=True, level=5, per_image=False, return_levels=False):
    """``tf_ms_ssim`` (:170-192): prod(mcs[0:level-1] ** w[0:level-1]) * mssim[level-1] ** w[level-1] with the batch means of every
    level (mean_metric only takes the mean of that scalar, as in the reference); per_image=True: the same formula on each image's
    own means, ``[B]``.  A negative mean cs gives NaN, as the reference's fractional power does (nothing is clamped).  Needs
    min(H, W) >= 11 * 2**(level-1).  return_levels=True: also the level means ``[level, B+1, 2]`` (row B the batch)."""
    import torch

    del mean_metric   # the value is a scalar already (:190-191)
    B, H, W = _dims(a)
    level = int(level)
    size = 11
    if level < 1 or level > len(MS_SSIM_WEIGHTS):
        raise ValueError("level must be 1..5")
    if min(H, W) < size * 2 ** (level - 1):
        raise ValueError(f"ms_ssim with {level} levels needs images of at least {size * 2 ** (level - 1)} pixels per side "
                         f"(got {H} x {W})")
    taps = gaussian_taps(size, 1.5)
    x, y, as_np = _pair(a, b)
    lib = _lib.load()
    value = torch.empty(B + 1, dtype=torch.float32, device=x.device)
    lm = torch.empty((level, B + 1, 2), dtype=torch.float32, device=x.device)
    nbytes = lib.emd_ms_ssim_workspace_bytes(B, H, W, level, size)
    ws = _ws(nbytes, x.device)
    _lib.check(lib.emd_ms_ssim_f32(_p(x), _p(y), B, H, W, level, _taps_arg(taps), size, _p(value), _p(lm), _p(ws), nbytes,
                                   _lib.stream_ptr()), "emd_ms_ssim_f32")
    v = _out(value[:B], as_np) if per_image else _out(value[B], as_np, True)
    return (v, _out(lm, as_np)) if return_levels else v


def psnr(a, b, data_range=1.0, per_image=False, return_mse=False):
    """10 log10(data_range^2 / mse): of the batch mse, or (per_image=True) of each image's, ``[B]``; mse == 0 gives inf.
    return_mse=True: the pair (psnr, mse)."""
    import torch

    x, y, as_np = _pair(a, b)
    B, H, W = x.shape
    lib = _lib.load()
    out = torch.empty((B + 1, 2), dtype=torch.float32, device=x.device)
    nbytes = lib.emd_psnr_workspace_bytes(B, H * W)
    ws = _ws(nbytes, x.device)
    _lib.check(lib.emd_psnr_f32(_p(x), _p(y), B, C.c_long(H * W), C.c_float(data_range), _p(out), _p(ws), nbytes, _lib.stream_ptr()),
               "emd_psnr_f32")
    sel = out[:B] if per_image else out[B]
    p, m = _out(sel[..., 1], as_np, not per_image), _out(sel[..., 0], as_np, not per_image)
    return (p, m) if return_mse else p


def ssim_loss(x, y, dout=None, scale=1.0, per_image=False, size=11, sigma=1.5, loss_acc=None, acc_stride=1, acc_weight=0.0,
              return_ssim=False):
    """L = 1 - ssim(x, y) (:775) and, when ``dout`` (a CUDA tensor shaped like x) is given, ``dout += scale * dL/dx`` -- the gradient
    is ADDED so that it composes with ``train_ops.denoise_loss``'s dout; there is no gradient for y.  per_image=False: L is the
    loss of the batch mean, a device scalar; per_image=True: every image its own loss, ``[B]``.  ``scale``: a number, or a CUDA
    tensor of B floats (one factor per image).  loss_acc (CUDA tensor): ``loss_acc[b * acc_stride] += acc_weight * L_b``
    (per_image) or ``loss_acc[0] += acc_weight * L``.  return_ssim=True: the pair (L, mean ssim)."""
    import torch

    taps = gaussian_taps(size, sigma)
    B, H, W = _dims(x)
    if H < size or W < size:
        raise ValueError(f"image {H} x {W} is smaller than the {size} x {size} window")
    xd, yd, as_np = _pair(x, y)
    if dout is not None:
        if not (isinstance(dout, torch.Tensor) and dout.is_cuda and dout.dtype == torch.float32 and dout.is_contiguous()
                and dout.numel() == xd.numel()):
            raise ValueError("dout must be a contiguous float32 CUDA tensor shaped like x")
    scale_dev = None
    if isinstance(scale, torch.Tensor):
        if not (scale.is_cuda and scale.dtype == torch.float32 and scale.is_contiguous() and scale.numel() == B):
            raise ValueError("a per-image scale is a contiguous float32 CUDA tensor of B elements")
        scale_dev, scale = scale, 1.0
    lib = _lib.load()
    res = torch.empty((B + 1, 2), dtype=torch.float32, device=xd.device)
    nbytes = lib.emd_ssim_loss_workspace_bytes(B, H, W, size)
    ws = _ws(nbytes, xd.device)
    _lib.check(lib.emd_ssim_loss_f32(_p(xd), _p(yd), B, H, W, _taps_arg(taps), size, 1 if per_image else 0, C.c_float(scale),
                                     _p(scale_dev), _p(dout), _p(res), _p(loss_acc), int(acc_stride), C.c_float(acc_weight), _p(ws),
                                     nbytes, _lib.stream_ptr()), "emd_ssim_loss_f32")
    sel = res[:B] if per_image else res[B]
    loss, val = _out(sel[..., 1], as_np, not per_image), _out(sel[..., 0], as_np, not per_image)
    return (loss, val) if return_ssim else loss


def avg_pool2x2_same(a):
    """``tf.nn.avg_pool(a, [1,2,2,1], [1,2,2,1], 'SAME')`` on single-channel images (:178-179) -> ``[B, ceil(H/2), ceil(W/2), 1]``."""
    import torch

    x, as_np = _images(a)
    B, H, W = x.shape
    y = torch.empty((B, (H + 1) // 2, (W + 1) // 2, 1), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().emd_avgpool2x2_same_c1_f32(_p(x), _p(y), B, H, W, _lib.stream_ptr()), "emd_avgpool2x2_same_c1_f32")
    return _out(y, as_np)


def score(pred, truth):
    """{"mse", "psnr", "ssim"} of a batch of predictions against ``truth`` (batch values; data range 1), computed on the device."""
    p, m = psnr(pred, truth, return_mse=True)
    return {"mse": m, "psnr": p, "ssim": ssim(pred, truth)}


def tf_ssim(img1, img2, cs_map=False, mean_metric=True, size=11, sigma=1.5):
    """The reference's name and argument list (:142)."""
    return ssim(img1, img2, cs_map=cs_map, mean_metric=mean_metric, size=size, sigma=sigma)


def tf_ms_ssim(img1, img2, mean_metric=True, level=5):
    """The reference's name and argument list (:170)."""
    return ms_ssim(img1, img2, mean_metric=mean_metric, level=level)
