"""Dose series on the device (csrc/dose.hip): low-dose images made by throwing a fixed number of electrons at a
micrograph taken as an unnormalised probability density -- the reference's second low-quality generator,
misc_py/lq_img_gen-backup.py:6-91 (``lq_chunks_gen``, ``record_lq``, ``lq_img_gen``).  The result is a multinomial sample with an
exact total, and a series of levels is nested: every level contains the electrons of the level below.

All-integer arithmetic (include/emdenoise.h states it; tests/dose_ref.py restates it in numpy), so every output is exact:
weights ``q = rint(x / max * 2**32)`` (a pixel that is not finite or <= 0 weighs 0), their inclusive row-major prefix sum as int64,
one Philox4x32-10 stream per image, draw ``d`` -> target ``t = (r * T) >> 64`` -> the pixel ``searchsorted(cdf, t, "right")``.

Departures from the reference: its walk along the sorted uniforms advances at most one pixel per draw (:21-26), so a draw that skips
a whole low-weight pixel is booked to the wrong pixel -- here the lookup is the inverse CDF the walk stands for; it normalises the
cumulative sum in floating point -- here the comparison is scaled by the total in integers; it reseeds numpy from numpy per chunk --
here the draws ``[0, D)`` of an image are the same electrons however they are split into calls or levels.  The reference is not run.

The conventions of ``emdenoise.focus``: images are float32 ``[H,W]`` or ``[B,H,W]``; numpy in -> numpy out; torch CUDA tensor in ->
device tensor out, on the current stream, with no host synchronisation (capturable); arguments are checked on the shape before
anything moves to the device, and an error names the function.  A ``[H,W]`` input gives outputs without the batch axis."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .focus import _is_tensor
from .metrics import _p, _ws

TILE, COARSE, MAX_LEVELS = 2048, 2048, 32        # EMD_DOSE_TILE, EMD_DOSE_COARSE, EMD_DOSE_MAX_LEVELS
SCAN_STEP = 256                                  # tiles that the scan of the tiles' sums covers in one step
EMPTY, SANITIZED = 1, 2                          # EMD_DOSE_EMPTY, EMD_DOSE_SANITIZED
MODES = {"unit": 0, "uint16": 1}                 # EMD_DOSE_UNIT, EMD_DOSE_UINT16
MAX_EXTENT, MAX_PIXELS, MAX_DRAWS = 32768, 1 << 30, (1 << 31) - 1


def _dims(name, x):
    """(B, H, W) of a float32 [H,W] or [B,H,W] argument, checked before anything moves."""
    if not _is_tensor(x) and not isinstance(x, np.ndarray):
        raise ValueError(f"{name}: images are a numpy array or a torch tensor (got {type(x).__name__})")
    shp = tuple(int(s) for s in x.shape)
    if len(shp) not in (2, 3):
        raise ValueError(f"{name}: images are [H,W] or [B,H,W] (got shape {shp})")
    if "float32" not in str(x.dtype):
        raise ValueError(f"{name}: images are float32 (got {x.dtype})")
    B, H, W = (1,) + shp if len(shp) == 2 else shp
    if min(H, W) < 2 or max(H, W) > MAX_EXTENT or H * W > MAX_PIXELS:
        raise ValueError(f"{name}: 2 <= H, W <= {MAX_EXTENT} and H W <= 2^30 (got {H} x {W})")
    if B > 65535:
        raise ValueError(f"{name}: at most 65535 images (got {B})")
    return B, H, W


def _device_images(x):
    import torch

    as_np = not _is_tensor(x)
    if as_np:
        a = np.ascontiguousarray(x)
        t = torch.from_numpy(a if a.flags.writeable else a.copy())     # torch warns about a read-only array
    else:
        t = x
    if t.dim() == 2:
        t = t.reshape(1, *t.shape)
    if not t.is_cuda:
        t = t.to(torch.device("cuda", torch.cuda.current_device()))
    return t.contiguous(), as_np


def _integer(name, what, v, least, most):
    if isinstance(v, bool) or int(v) != v or not least <= int(v) <= most:
        raise ValueError(f"{name}: {what} must be an integer, {least} <= {what} <= {most} (got {v!r})")
    return int(v)


def _seed_and_image(name, seed, first_image, B):
    return _integer(name, "seed", seed, 0, (1 << 64) - 1), _integer(name, "first_image", first_image, 0, (1 << 32) - B)


def _check_bounds(name, bounds):
    """Draw indices of the levels' ends -> a list of L + 1 ints, refused unless 0 <= bounds[0] <= ... and bounds[L] - bounds[0] < 2^31."""
    b = [int(v) for v in bounds]
    if not 2 <= len(b) <= MAX_LEVELS + 1:
        raise ValueError(f"{name}: 1 to {MAX_LEVELS} levels (got {len(b) - 1})")
    if b[0] < 0 or any(b[k] > b[k + 1] for k in range(len(b) - 1)):
        raise ValueError(f"{name}: the levels' draw counts must not descend (got {b})")
    if b[-1] - b[0] > MAX_DRAWS:
        raise ValueError(f"{name}: at most 2^31 - 1 draws an image in one call, counts are int32 (got {b[-1] - b[0]})")
    return b


def _check_mode(name, mode, none_ok=False):
    if mode is None and none_ok:
        return None
    if mode not in MODES:
        raise ValueError(f"{name}: rescale mode must be 'unit' or 'uint16'{' or None' if none_ok else ''} (got {mode!r})")
    return MODES[mode]


def _cdf_device(xd):
    import torch

    B, H, W = (int(s) for s in xd.shape)
    lib = _lib.load()
    cdf = torch.empty((B, H, W), dtype=torch.int64, device=xd.device)
    status = torch.empty((B,), dtype=torch.int32, device=xd.device)
    nbytes = lib.emd_dose_workspace_bytes(B, H, W)
    ws = _ws(nbytes, xd.device)
    _lib.check(lib.emd_dose_cdf_i64(_p(xd), B, H, W, _p(cdf), _p(status), _p(ws), nbytes, _lib.stream_ptr()), "emd_dose_cdf_i64")
    return cdf, status


def _draw_device(cdf, seed, first_image, bounds, planes):
    B, H, W = (int(s) for s in cdf.shape)
    L = len(bounds) - 1
    arr = (C.c_int64 * (L + 1))(*bounds)
    _lib.check(_lib.load().emd_dose_draw_i32(_p(cdf), B, H, W, seed, first_image, arr, L, _p(planes), _lib.stream_ptr()),
               "emd_dose_draw_i32")


def _cumulate_device(planes, B, L, H, W):
    import torch

    minmax = torch.empty((B, L, 2), dtype=torch.int32, device=planes.device)
    _lib.check(_lib.load().emd_dose_cumulate_i32(_p(planes), B, L, H, W, _p(minmax), _lib.stream_ptr()), "emd_dose_cumulate_i32")
    return minmax


def _rescale_device(planes, minmax, B, L, H, W, mode):
    import torch

    out = torch.empty((B, L, H, W), dtype=torch.int32 if mode == MODES["uint16"] else torch.float32, device=planes.device)
    _lib.check(_lib.load().emd_dose_rescale(_p(planes), _p(minmax), B, L, H, W, mode, _p(out), _lib.stream_ptr()), "emd_dose_rescale")
    return out


def cdf(x, return_status=False):
    """The integer cumulative distribution of every image -> int64, the shape of x: ``cumsum(q)`` in row-major order, inclusive, with
    ``q = rint(double(x) / double(max) * 2**32)`` and a pixel that is not finite or <= 0 weighing 0.  Exact, whatever the order of the
    additions on the device.  With return_status ``(cdf, status)``: status int32 ``[B]`` with bit ``EMPTY`` (no positive pixel: the cdf
    is all 0) and bit ``SANITIZED`` (a negative, infinite or NaN pixel was zeroed)."""
    _dims("cdf", x)
    xd, as_np = _device_images(x)
    c, status = _cdf_device(xd)
    c = c.reshape(tuple(x.shape))
    if as_np:
        c, status = c.cpu().numpy(), status.cpu().numpy()
    return (c, status) if return_status else c


def sample_counts(x, draws, seed=0, first_draw=0, first_image=0, out=None):
    """Electron counts of the draws ``[first_draw, first_draw + draws)`` of every image -> int32, the shape of x: a multinomial sample
    of exactly ``draws`` electrons an image with the probabilities ``q / sum(q)`` of ``cdf``.  Image b of the batch draws from the
    Philox stream ``(seed, first_image + b)``, so an image's counts do not depend on the batch it is in, and the draws ``[0, D)``
    are the same electrons however they are split into calls.  ``out=`` (a device int32 tensor of x's shape) is ADDED to and returned:
    a later call with ``first_draw`` where the last one stopped extends it.  An image with no positive pixel gets no electrons."""
    import torch

    B, H, W = _dims("sample_counts", x)
    draws = _integer("sample_counts", "draws", draws, 0, MAX_DRAWS)
    first_draw = _integer("sample_counts", "first_draw", first_draw, 0, (1 << 62))
    seed, first_image = _seed_and_image("sample_counts", seed, first_image, B)
    if out is not None:
        if not _is_tensor(out) or not out.is_cuda or out.dtype != torch.int32 or tuple(out.shape) != tuple(x.shape) or not out.is_contiguous():
            raise ValueError(f"sample_counts: out is a contiguous int32 CUDA tensor of shape {tuple(x.shape)}")
    xd, as_np = _device_images(x)
    c, _ = _cdf_device(xd)
    planes = out if out is not None else torch.zeros((B, H, W), dtype=torch.int32, device=xd.device)
    _draw_device(c, seed, first_image, [first_draw, first_draw + draws], planes)
    if out is not None:
        return out
    planes = planes.reshape(tuple(x.shape))
    return planes.cpu().numpy() if as_np else planes


def _series_device(xd, bounds, seed, first_image, mode):
    import torch

    B, H, W = (int(s) for s in xd.shape)
    L = len(bounds) - 1
    c, status = _cdf_device(xd)
    planes = torch.zeros((B, L, H, W), dtype=torch.int32, device=xd.device)
    _draw_device(c, seed, first_image, bounds, planes)
    minmax = _cumulate_device(planes, B, L, H, W)
    return (planes if mode is None else _rescale_device(planes, minmax, B, L, H, W, mode)), status


def dose_series(x, avg_counts=(2, 4, 8, 16, 32, 64), seed=0, first_image=0, rescale=None, return_status=False):
    """A nested dose series of every image -> ``[B,L,H,W]`` (``[L,H,W]`` for an ``[H,W]`` image): level k holds the first
    ``round(avg_counts[k] * H * W)`` electrons of the image's stream, so it contains every electron of the level below and sums to
    that number exactly.  avg_counts must be positive and ascending.

    rescale None: the counts, int32.  ``"uint16"``: ``record_lq``'s 16-bit image (:30-35), ``int(65535.0 * (c - min) / (max - min))``
    with the plane's own min and max, the operations in double as numpy does them, stored as int32.  ``"unit"``:
    ``(c - min) / (max - min)`` in double, rounded once to float32.  Where max == min the reference divides by zero; here the plane is
    all 0.  With return_status ``(series, status)``, status as ``cdf`` gives it."""
    B, H, W = _dims("dose_series", x)
    avg = [float(a) for a in avg_counts]
    if not avg or not all(np.isfinite(a) and a > 0 for a in avg) or any(avg[k] >= avg[k + 1] for k in range(len(avg) - 1)):
        raise ValueError(f"dose_series: avg_counts must be positive and ascending (got {list(avg_counts)})")
    bounds = _check_bounds("dose_series", [0] + [int(round(a * H * W)) for a in avg])
    mode = _check_mode("dose_series", rescale, none_ok=True)
    seed, first_image = _seed_and_image("dose_series", seed, first_image, B)
    xd, as_np = _device_images(x)
    out, status = _series_device(xd, bounds, seed, first_image, mode)
    if len(x.shape) == 2:
        out = out[0]
    if as_np:
        out, status = out.cpu().numpy(), status.cpu().numpy()
    return (out, status) if return_status else out


def rescale_counts(counts, mode):
    """``record_lq``'s min-max rescale (:30-35) of every plane of int32 counts ``[H,W]``, ``[B,H,W]`` or ``[B,L,H,W]`` (not negative) ->
    the same shape: mode ``"uint16"`` int32 ``int(65535.0 * (c - min) / (max - min))``, mode ``"unit"`` float32
    ``(c - min) / (max - min)``, as ``dose_series`` describes them.  A flat plane gives zeros."""
    import torch

    if not _is_tensor(counts) and not isinstance(counts, np.ndarray):
        raise ValueError(f"rescale_counts: counts are a numpy array or a torch tensor (got {type(counts).__name__})")
    shp = tuple(int(s) for s in counts.shape)
    if len(shp) not in (2, 3, 4):
        raise ValueError(f"rescale_counts: counts are [H,W], [B,H,W] or [B,L,H,W] (got shape {shp})")
    if "int32" not in str(counts.dtype):
        raise ValueError(f"rescale_counts: counts are int32 (got {counts.dtype})")
    H, W = shp[-2:]
    planes = int(np.prod(shp[:-2], dtype=np.int64))
    if min(H, W) < 2 or max(H, W) > MAX_EXTENT or H * W > MAX_PIXELS or planes > 65535:
        raise ValueError(f"rescale_counts: 2 <= H, W <= {MAX_EXTENT}, H W <= 2^30, at most 65535 planes (got shape {shp})")
    m = _check_mode("rescale_counts", mode)
    as_np = not _is_tensor(counts)
    t = torch.from_numpy(np.ascontiguousarray(counts)) if as_np else counts
    if not t.is_cuda:
        t = t.to(torch.device("cuda", torch.cuda.current_device()))
    t = t.contiguous()
    if planes == 0:
        out = torch.empty(shp, dtype=torch.int32 if m else torch.float32, device=t.device)
    else:
        minmax = _cumulate_device(t, planes, 1, H, W)           # one level: the planes stay as they are
        out = _rescale_device(t, minmax, planes, 1, H, W, m).reshape(shp)
    return out.cpu().numpy() if as_np else out


def lq_levels(avg_counts, chunkdepth, size):
    """The draws of every level of ``lq_img_gen``: the reference sums chunks of ``chunkdepth * size`` electrons and saves after
    ``int(avg / chunkdepth)`` of them (:52-55, :72-83)."""
    return [int(avg / chunkdepth) * chunkdepth * size for avg in avg_counts]


def lq_img_gen(img, avg_counts=[2, 4, 8, 16, 32, 64], chunkdepth=2, seed=0):
    """``lq_img_gen`` (lq_img_gen-backup.py:46-91), the reference's name and argument order without ``saveLoc`` and ``num_parallel``:
    img ``[H,W]`` (anything numpy converts to float32) -> the list of uint16 numpy images, one per entry of avg_counts, that the
    reference writes to ``avgcounts_<n>.tif``.  Level k holds ``int(avg_counts[k] / chunkdepth) * chunkdepth * img.size`` electrons, as
    the reference's chunk counting gives, each level containing the one below, min-max rescaled to 16 bits (a flat level: zeros)."""
    img = np.ascontiguousarray(np.asarray(img.detach().cpu().numpy() if _is_tensor(img) else img), dtype=np.float32)
    if img.ndim != 2:
        raise ValueError(f"lq_img_gen: img is one image [H,W] (got shape {img.shape})")
    _dims("lq_img_gen", img)
    if isinstance(chunkdepth, bool) or int(chunkdepth) != chunkdepth or chunkdepth < 1:
        raise ValueError(f"lq_img_gen: chunkdepth must be a positive integer (got {chunkdepth!r})")
    if len(avg_counts) < 1 or any(not a > 0 for a in avg_counts):
        raise ValueError(f"lq_img_gen: avg_counts must be positive (got {list(avg_counts)})")
    bounds = _check_bounds("lq_img_gen", [0] + lq_levels(avg_counts, int(chunkdepth), img.size))
    seed, _ = _seed_and_image("lq_img_gen", seed, 0, 1)
    xd, _ = _device_images(img)
    out, _ = _series_device(xd, bounds, seed, 0, MODES["uint16"])
    return [p.astype(np.uint16) for p in out[0].cpu().numpy()]
