"""Dataset diversity on the device (csrc/diversity.hip): how different the micrographs of a harvested dataset are
from each other -- the arithmetic of the reference's misc_py/img_stats.py (plotted by misc_py/gram_hist.py): for every image the
matrix of squared Euclidean distances between its rows (the script's ``gram``), and for pairs of images the mean squared difference
of their two matrices.  The directory walk, the shuffle, the histogram and the plot are host work on P numbers and are not here.

The conventions of ``emdenoise.harvest``: images are float32 ``[H,W]`` or ``[B,H,W]``; numpy in -> numpy out; torch CUDA tensor in ->
device tensor out, on the current stream, with no host synchronisation; arguments are checked on the shape before anything moves to
the device, and an error names the function.  Python here only shapes buffers: every number comes from a HIP kernel (the float32
matrix-core product of include/emdenoise.h; no matrix is written for the pair statistic)."""
from __future__ import annotations

import numpy as np

from . import _lib
from .metrics import _p, _ws

TILE, TILE_K, CHAIN = 128, 32, 256             # EMD_DIVERSITY_TILE, _TILE_K, _CHAIN
OK, NONFINITE, BAD_INDEX = 0, 1, 2             # EMD_DIVERSITY_OK, _NONFINITE, _BAD_INDEX
MAX_W, MAX_H_PAIR, MAX_H_DISTANCES, MAX_PAIRS = 32768, 8192, 4096, 1 << 20


def _is_tensor(a):
    import torch

    return isinstance(a, torch.Tensor)


def _image_dims(name, x, max_h):
    """(B, H, W) of a float32 [H,W] or [B,H,W] argument, checked before anything moves."""
    if not _is_tensor(x) and not isinstance(x, np.ndarray):
        raise ValueError(f"{name}: images are a numpy array or a torch tensor (got {type(x).__name__})")
    shp = tuple(x.shape)
    if len(shp) not in (2, 3):
        raise ValueError(f"{name}: images are [H,W] or [B,H,W] (got shape {shp})")
    if "float32" not in str(x.dtype):
        raise ValueError(f"{name}: images are float32 (got {x.dtype})")
    B, H, W = (1,) + shp if len(shp) == 2 else shp
    if not 1 <= H <= max_h or not 1 <= W <= MAX_W:
        raise ValueError(f"{name}: 1 <= H <= {max_h}, 1 <= W <= {MAX_W} (got {H} x {W})")
    if B > 65535:
        raise ValueError(f"{name}: at most 65535 images (got {B})")
    return int(B), int(H), int(W)


def _device_images(x):
    """-> (contiguous float32 CUDA tensor [B,H,W], was_numpy)."""
    import torch

    as_np = not _is_tensor(x)
    t = torch.from_numpy(np.ascontiguousarray(x)) if as_np else x
    if t.dim() == 2:
        t = t.reshape(1, *t.shape)
    if not t.is_cuda:
        t = t.to(torch.device("cuda", torch.cuda.current_device()))
    return t.contiguous(), as_np


def _check_pairs(name, pairs):
    if not _is_tensor(pairs) and not isinstance(pairs, np.ndarray):
        raise ValueError(f"{name}: pairs are a numpy array or a torch tensor (got {type(pairs).__name__})")
    shp = tuple(pairs.shape)
    if len(shp) != 2 or shp[1] != 2 or "int32" not in str(pairs.dtype):
        raise ValueError(f"{name}: pairs are int32 [P,2] (got {pairs.dtype} {shp})")
    if shp[0] > MAX_PAIRS:
        raise ValueError(f"{name}: at most {MAX_PAIRS} pairs a call (got {shp[0]})")
    return int(shp[0])


def row_sq_norms(x, return_nonfinite=False):
    """``(x ** 2).sum(axis=-1)`` of every image in double, in the fixed order of include/emdenoise.h -> ``[B,H]`` float64; with
    return_nonfinite also the number of NaN or infinite pixels of every image, ``[B]`` int32."""
    import torch

    B, H, W = _image_dims("row_sq_norms", x, MAX_H_PAIR)
    xd, as_np = _device_images(x)
    norms = torch.empty((B, H), dtype=torch.float64, device=xd.device)
    bad = torch.empty((B,), dtype=torch.int32, device=xd.device)
    if B:
        _lib.check(_lib.load().emd_row_sq_norms_f64(_p(xd), B, H, W, _p(norms), _p(bad), _lib.stream_ptr()), "emd_row_sq_norms_f64")
    if as_np:
        norms, bad = norms.cpu().numpy(), bad.cpu().numpy()
    return (norms, bad) if return_nonfinite else norms


def row_distances(x):
    """The script's ``gram``: ``D[i,j] = n_i + n_j - 2 x_i . x_j``, the squared Euclidean distance between the rows i and j of every
    image -> float32 ``[B,H,H]``, equal to its transpose as bits.  The product is the float32 matrix-core chain of
    include/emdenoise.h, norms and the combination are in double, rounded once.  H <= 4096."""
    import torch

    B, H, W = _image_dims("row_distances", x, MAX_H_DISTANCES)
    xd, as_np = _device_images(x)
    D = torch.empty((B, H, H), dtype=torch.float32, device=xd.device)
    if B:
        lib = _lib.load()
        nbytes = lib.emd_row_distances_workspace_bytes(B, H, W)
        ws = _ws(nbytes, xd.device)
        _lib.check(lib.emd_row_distances_f32(_p(xd), B, H, W, _p(D), _p(ws), nbytes, _lib.stream_ptr()), "emd_row_distances_f32")
    return D.cpu().numpy() if as_np else D


def _pairs_device(xd, pd):
    """stack [B,H,W] and pairs [P,2] on the device -> (ssd [P] float64, status [P] int32)."""
    import torch

    B, H, W = (int(s) for s in xd.shape)
    P = int(pd.shape[0])
    ssd = torch.empty((P,), dtype=torch.float64, device=xd.device)
    status = torch.empty((P,), dtype=torch.int32, device=xd.device)
    if P:
        lib = _lib.load()
        nbytes = lib.emd_gram_ssd_workspace_bytes(B, H, W, P)
        ws = _ws(nbytes, xd.device)
        _lib.check(lib.emd_gram_ssd_f64(_p(xd), B, H, W, _p(pd), P, _p(ssd), _p(status), _p(ws), nbytes, _lib.stream_ptr()),
                   "emd_gram_ssd_f64")
    return ssd, status


def gram_ssd_pairs(stack, pairs):
    """``mean((D(stack[i]) - D(stack[j])) ** 2)`` for every row (i, j) of ``pairs`` (int32 ``[P,2]``, numpy or device), D the matrix
    of ``row_distances`` -- which is never formed: the two images' products run side by side and only the H x H sum leaves the
    kernel.  -> ``(ssd [P] float64, status [P] int32)``: status ``OK``; ``NONFINITE`` where a named image has a NaN or infinite
    pixel (the reference skips such an image); ``BAD_INDEX`` where an index is outside ``[0, B)``; the value is NaN where the status
    is not ``OK``.  ``ssd(x, x)`` is exactly 0, ``(i, j)`` and ``(j, i)`` give the same bits, and a pair's value depends on nothing
    but its two images.  H <= 8192."""
    import torch

    B, H, W = _image_dims("gram_ssd_pairs", stack, MAX_H_PAIR)
    _check_pairs("gram_ssd_pairs", pairs)
    xd, as_np = _device_images(stack)
    pd = pairs if _is_tensor(pairs) else torch.from_numpy(np.ascontiguousarray(pairs))
    ssd, status = _pairs_device(xd, pd.to(xd.device).contiguous())
    return (ssd.cpu().numpy(), status.cpu().numpy()) if as_np else (ssd, status)


def gram_ssd(a, b):
    """``mean((D(a[k]) - D(b[k])) ** 2)`` for two stacks of equal shape -> ``[P]`` float64, P the number of images in each: the
    pairs (k, P + k) of ``gram_ssd_pairs`` on the concatenated stack.  NaN where either image has a non-finite pixel."""
    import torch

    B, H, W = _image_dims("gram_ssd", a, MAX_H_PAIR)
    if (B, H, W) != _image_dims("gram_ssd", b, MAX_H_PAIR) or len(a.shape) != len(b.shape):
        raise ValueError(f"gram_ssd: the two stacks have one shape (got {tuple(a.shape)} and {tuple(b.shape)})")
    if 2 * B > 65535:
        raise ValueError(f"gram_ssd: at most 32767 pairs a call (got {B})")
    ad, as_np = _device_images(a)
    bd, _ = _device_images(b)
    k = torch.arange(B, dtype=torch.int32, device=ad.device)
    ssd, _ = _pairs_device(torch.cat([ad, bd.to(ad.device)]), torch.stack([k, k + B], dim=1).contiguous())
    return ssd.cpu().numpy() if as_np else ssd


def pair_schedule(n, limit=None, first_offset=1):
    """The script's walk over a list of n images, host-side -> int32 ``[P,2]``: ``(i, i + first_offset + loop)`` for i = 0, 1, ..
    with loop = 0, then loop = 1, ...  Each pass stops where its second index reaches the end of the list (there the script itself
    indexes past the list and dies), and the walk ends when a pass has no pair left, so that without a limit every pair at least
    ``first_offset`` apart comes up once; it is cut after ``limit`` pairs.  No index is ever >= n."""
    if int(n) != n or n < 0:
        raise ValueError(f"pair_schedule: n is a number of images (got {n!r})")
    if limit is not None and (int(limit) != limit or limit < 0):
        raise ValueError(f"pair_schedule: limit is a number of pairs or None (got {limit!r})")
    if int(first_offset) != first_offset or first_offset < 1:
        raise ValueError(f"pair_schedule: first_offset must be an integer >= 1 (got {first_offset!r})")
    n, off = int(n), int(first_offset)
    total = sum(n - d for d in range(off, n))
    P = total if limit is None else min(total, int(limit))
    out = np.empty((P, 2), np.int32)
    done = 0
    for d in range(off, n):
        take = min(n - d, P - done)
        if take <= 0:
            break
        out[done:done + take, 0] = np.arange(take)
        out[done:done + take, 1] = np.arange(take) + d
        done += take
    return out


def dataset_diversity(stack, limit=None):
    """``gram_ssd_pairs`` over ``pair_schedule(len(stack), limit)`` -> ``(values, skipped)``: the float64 values of the pairs whose
    status is ``OK``, in the schedule's order, and the number of pairs left out (the script's ``skips``).  The selection needs the
    statuses on the host, so this call synchronises."""
    B, H, W = _image_dims("dataset_diversity", stack, MAX_H_PAIR)
    if len(stack.shape) != 3:
        raise ValueError(f"dataset_diversity: the stack is [N,H,W] (got shape {tuple(stack.shape)})")
    pairs = pair_schedule(B, limit)
    if pairs.shape[0] > MAX_PAIRS:
        raise ValueError(f"dataset_diversity: at most {MAX_PAIRS} pairs a call (got {pairs.shape[0]}): set limit")
    ssd, status = gram_ssd_pairs(stack, pairs)
    keep = status == OK
    return ssd[keep], int(pairs.shape[0] - int(keep.sum()))
