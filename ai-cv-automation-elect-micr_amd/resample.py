"""``cv2.resize`` on the device for one-channel float32 images (csrc/resample.hip, csrc/resize_taps.hpp): what the
reference does to every image before anything else touches it -- ``load_image(addr, resizeSize)`` with ``INTER_AREA`` or ``INTER_CUBIC``,
a crop of random size resized to the network's side (modified_Xception.py:976-982), ``EWREC.resize_stack`` with the default
``INTER_LINEAR`` (ewrec_class.py:236-238) and ``INTER_NEAREST`` (misc_py/downsample.py:24).  OpenCV is not used: the arithmetic is
restated from the rules in include/emdenoise.h, float32 roundings of the coordinates included, sums in double.

The conventions of ``emdenoise.harvest``: images are float32 ``[H,W]`` or ``[B,H,W]``; numpy in -> numpy out; torch CUDA tensor in ->
device tensor out, on the current stream, with no host synchronisation; arguments are checked before anything moves to the device.
Python here only shapes buffers: every pixel comes from one HIP kernel, and ``taps`` from the library's host function, the same code
the kernel calls.  1 <= H, W <= 32768; 1 <= h, w <= 8192.  Non-finite values are the caller's problem."""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np

from . import _lib
from .metrics import _p

NEAREST, LINEAR, CUBIC, AREA = 0, 1, 2, 3   # cv2.INTER_*
INTERPOLATIONS = {"nearest": NEAREST, "linear": LINEAR, "cubic": CUBIC, "area": AREA}
MAX_EXTENT, MAX_SIZE, MAX_BATCH = 32768, 8192, 65535

Taps = collections.namedtuple("Taps", "first count index weight block")


def _mode(name, interpolation):
    if isinstance(interpolation, str):
        if interpolation in INTERPOLATIONS:
            return INTERPOLATIONS[interpolation]
    elif isinstance(interpolation, (int, np.integer)) and not isinstance(interpolation, bool) and int(interpolation) in INTERPOLATIONS.values():
        return int(interpolation)
    raise ValueError(f"{name}: interpolation must be one of {sorted(INTERPOLATIONS)} or cv2's 0..3 (got {interpolation!r})")


def _int_in(name, what, v, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= hi:
        raise ValueError(f"{name}: {what} must be an integer, 1..{hi} (got {v!r})")
    return int(v)


def _dsize(name, dsize):
    """(w, h), cv2's order, or one int for a square -> (h, w)."""
    if isinstance(dsize, (int, np.integer)):
        dsize = (dsize, dsize)
    if not isinstance(dsize, (tuple, list)) or len(dsize) != 2:
        raise ValueError(f"{name}: dsize is (w, h) or an integer (got {dsize!r})")
    w, h = (_int_in(name, "dsize", v, MAX_SIZE) for v in dsize)
    return h, w


def _check_images(name, x):
    """-> (the argument as a tensor, was_numpy, rank, B, H, W), before anything moves to the device."""
    import torch

    is_np = not isinstance(x, torch.Tensor)
    if is_np:
        x = np.asarray(x)
    if x.dtype != (np.float32 if is_np else torch.float32):
        raise ValueError(f"{name}: images are float32 (got {x.dtype})")
    rank = len(x.shape)
    if rank not in (2, 3):
        raise ValueError(f"{name}: images are [H,W] or [B,H,W] (got shape {tuple(x.shape)})")
    B, H, W = (1,) + tuple(x.shape) if rank == 2 else tuple(x.shape)
    if not (0 <= B <= MAX_BATCH and 1 <= H <= MAX_EXTENT and 1 <= W <= MAX_EXTENT):
        raise ValueError(f"{name}: at most {MAX_BATCH} images, 1 <= H, W <= {MAX_EXTENT} (got shape {tuple(x.shape)})")
    return (torch.from_numpy(np.ascontiguousarray(x)) if is_np else x), is_np, rank, B, H, W


def _check_boxes(name, boxes, B, H, W):
    """-> the boxes as they go to the library: an int32 CUDA tensor as it is, anything else a checked int32 numpy array."""
    import torch

    if isinstance(boxes, torch.Tensor) and boxes.is_cuda:
        # a device-side sampler's boxes stay where they are: the kernel clamps them into the image
        if boxes.dtype != torch.int32 or tuple(boxes.shape) != (B, 4) or not boxes.is_contiguous():
            raise ValueError(f"{name}: device boxes are a contiguous int32 tensor [B,4] = [{B},4] (got {boxes.dtype}, {tuple(boxes.shape)})")
        return boxes
    bh = np.asarray(boxes)
    if bh.shape != (B, 4):
        raise ValueError(f"{name}: boxes are [B,4] = [{B},4], (x0, y0, bw, bh) (got shape {bh.shape})")
    if not np.issubdtype(bh.dtype, np.integer):
        raise ValueError(f"{name}: boxes are integers (got {bh.dtype})")
    bh = bh.astype(np.int64)
    bad = (bh[:, 0] < 0) | (bh[:, 1] < 0) | (bh[:, 2] < 1) | (bh[:, 3] < 1) | (bh[:, 0] + bh[:, 2] > W) | (bh[:, 1] + bh[:, 3] > H)
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise ValueError(f"{name}: box {k} = {tuple(int(v) for v in bh[k])} does not lie inside the {H} x {W} image with sizes >= 1")
    return bh.astype(np.int32)


def _resize(name, x, boxes, dsize, interpolation):
    import torch

    mode = _mode(name, interpolation)
    h, w = _dsize(name, dsize)
    t, as_np, rank, B, H, W = _check_images(name, x)
    if boxes is not None:
        boxes = _check_boxes(name, boxes, B, H, W)
    if not t.is_cuda:
        t = t.to(torch.device("cuda", torch.cuda.current_device()))
    xd = t.reshape(B, H, W).contiguous()
    if isinstance(boxes, np.ndarray):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{name}: the boxes are not on the device; pass an int32 CUDA tensor when capturing")
        boxes = torch.from_numpy(boxes).to(xd.device)
    out = torch.empty((B, h, w), dtype=torch.float32, device=xd.device)
    _lib.check(_lib.load().emd_resize_f32(_p(xd), C.c_long(H * W), W, B, H, W, _p(boxes), _p(out), h, w, mode, _lib.stream_ptr()),
               "emd_resize_f32")
    if rank == 2:
        out = out.reshape(h, w)
    return out.cpu().numpy() if as_np else out


def resize(x, dsize, interpolation="linear"):
    """``cv2.resize(x, dsize, interpolation=...)`` of every image of x, ``[H,W]`` or ``[B,H,W]`` float32 -> ``[h,w]`` or ``[B,h,w]``.
    dsize is ``(w, h)``, as cv2 orders it, or an int for a square; interpolation a name (``"nearest"``, ``"linear"``, ``"cubic"``,
    ``"area"``) or cv2's integer.  ``"area"`` is true area (fractional coverage; the block mean at whole ratios) where neither axis
    enlarges, and cv2's emulated area otherwise.  Equal sizes return the images bit for bit."""
    return _resize("resize", x, None, dsize, interpolation)


def crop_resize(x, boxes, dsize, interpolation="area"):
    """Image b's rectangle ``boxes[b] = (x0, y0, bw, bh)`` resized to dsize: ``cv2.resize(x[b, y0:y0+bh, x0:x0+bw], dsize, ...)`` in one
    launch for the whole batch, the sizes and the area rule taken per image -- a crop of random size resized to the network's side
    (the intent of modified_Xception.py:976-982).  ``boxes`` is ``[B,4]`` integers.  A host array is checked (inside the image, sizes
    >= 1) and uploaded.  An int32 CUDA tensor is used where it is: the boxes never visit the host and the call can be captured in a
    ``torch.cuda.graph``; the kernel clamps such a box into the image whatever it holds."""
    if boxes is None:
        raise ValueError("crop_resize: boxes are [B,4], (x0, y0, bw, bh) (got None)")
    return _resize("crop_resize", x, boxes, dsize, interpolation)


def taps(n_in, n_out, interpolation, other_in=None, other_out=None):
    """The taps of every destination sample of ``n_in -> n_out`` along one axis, from the library's host function
    (``emd_resize_taps``: the code the kernel calls).  ``other_in -> other_out`` are the sizes of the other axis, which the area rule
    looks at too (default: the same pair).  -> ``Taps(first, count, index, weight, block)``: ``first`` and ``count`` int32 ``[n_out]``;
    ``index`` int32 and ``weight`` float64 ``[n_out, max(count)]``, tap k of sample d reading ``index[d, k]`` (clamped into the axis:
    the border replicates) with ``weight[d, k]``, zero-weight padding behind ``count[d]`` repeating the last index; ``block`` 0, or
    the block's side where area takes its whole-ratio form (the weights are then 1 / block)."""
    mode = _mode("taps", interpolation)
    n_in = _int_in("taps", "n_in", n_in, MAX_EXTENT)
    n_out = _int_in("taps", "n_out", n_out, MAX_SIZE)
    other_in = n_in if other_in is None else _int_in("taps", "other_in", other_in, MAX_EXTENT)
    other_out = n_out if other_out is None else _int_in("taps", "other_out", other_out, MAX_SIZE)
    first, count = np.empty(n_out, np.int32), np.empty(n_out, np.int32)
    w4 = np.empty((n_out, 4), np.float64)
    block = C.c_int(0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    _lib.check(_lib.load().emd_resize_taps(mode, n_in, n_out, other_in, other_out, vp(first), vp(count), vp(w4),
                                           C.cast(C.byref(block), C.c_void_p)), "emd_resize_taps")
    K = max(int(count.max()), 1)
    k = np.arange(K)[None, :]
    cnt = count[:, None]
    index = np.clip(first[:, None] + np.minimum(k, np.maximum(cnt - 1, 0)), 0, n_in - 1).astype(np.int32)
    weight = np.where(k == 0, w4[:, 0:1], np.where(k == cnt - 1, w4[:, 3:4], np.where(k == 1, w4[:, 1:2], w4[:, 2:3])))
    weight = np.where(k < cnt, weight, 0.0)
    if block.value:
        weight = weight / float(block.value)
    return Taps(first, count, index, weight, int(block.value))
