"""Whole-micrograph denoising on the device: tile plans on the host, everything else in csrc/tile_ops.hip.

``denoise_images`` of the three apply classes (denoiser.Denoiser, autoencoder.Micrograph_Autoencoder, the graph-K
kernel_denoiser.Micrograph_Autoencoder) lands here.  An image or a stack of images is uploaded once (or used where it is, if it is
already a CUDA tensor), prepared per image, cut into the crops of the class's plan, run through the engine in batches of
``max_batch`` pooled over all images of the call, and blended once; one result comes back.  Per image the semantics are those of
the class's ``denoise`` with the same arguments; the result is float32.

The plan (tile start rows / columns and, per output row / column, the range of tiles covering it) is computed here and only
here, so that Python's ``round`` (half to even) in graph D's plan is the one the host path uses.  Kernels read it; they never
recompute it.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

PREP_S, PREP_K, PREP_D = 0, 1, 2  # include/emdenoise.h EMD_TILE_PREP_*
_MAX_TILES_PER_LAUNCH = 65535   # emd_tile_gather_f32: count <= 65535


# ---- plans ------------------------------------------------------------------------------------------------------------------
def d_starts(n: int, cs: int, overlap: int):
    """Denoiser.denoise: tiles evenly spaced over an axis of n >= cs pixels, starts rounded half to even."""
    num = (n - cs + (cs - overlap) - 1) // (cs - overlap) + 1 if n > cs else 1
    return [int(round(i * (n - cs) / max(num - 1, 1))) for i in range(num)]


def s_starts(n: int, cs: int, overlap: int):
    """autoencoder.Micrograph_Autoencoder.denoise: stride cs - 2*overlap over the padded axis of n pixels, the last tile
    aligned with its end."""
    step = cs - 2 * overlap
    s = list(range(0, max(n - cs, 0) + 1, step))
    if s[-1] != n - cs:
        s.append(n - cs)
    return s


def cover_ranges(starts, n: int, pad: int, cs: int, m: int) -> np.ndarray:
    """[n, 2] int32: for each un-padded position y, the tiles [first, last) whose kept window [s + m, s + cs - m) holds y + pad."""
    s = np.asarray(starts, np.int64)
    p = np.arange(n, dtype=np.int64) + pad
    first = np.searchsorted(s, p - cs + m, side="right")
    last = np.searchsorted(s, p - m, side="right")
    return np.stack([first, np.maximum(last, first)], axis=1).astype(np.int32)


class TilePlan:
    """Tiles of side cs over an [H,W] image reflect-padded by ``pad``, each keeping [start + m, start + cs - m) per axis."""

    def __init__(self, H: int, W: int, cs: int, pad: int, m: int, ys, xs):
        self.H, self.W, self.cs, self.pad, self.m = int(H), int(W), int(cs), int(pad), int(m)
        self.ys, self.xs = [int(v) for v in ys], [int(v) for v in xs]
        self.row_range = cover_ranges(self.ys, self.H, self.pad, self.cs, self.m)
        self.col_range = cover_ranges(self.xs, self.W, self.pad, self.cs, self.m)

    @property
    def tiles_per_image(self) -> int:
        return len(self.ys) * len(self.xs)

    def device_arrays(self, device):
        """One upload: (ys, xs, row_range, col_range) as device addresses into a single int32 tensor (returned to keep it alive)."""
        import torch

        flat = np.concatenate([np.asarray(self.ys, np.int32), np.asarray(self.xs, np.int32), self.row_range.ravel(),
                               self.col_range.ravel()])
        t = torch.from_numpy(flat).to(device)
        base = t.data_ptr()
        offs = np.cumsum([0, len(self.ys), len(self.xs), self.row_range.size])
        return t, [C.c_void_p(base + 4 * int(o)) for o in offs]


def d_plan(H: int, W: int, cs: int, overlap: int) -> TilePlan:
    return TilePlan(H, W, cs, 0, 0, d_starts(H, cs, overlap), d_starts(W, cs, overlap))


def s_plan(H: int, W: int, cs: int, overlap: int, used_overlap: int) -> TilePlan:
    """overlap here is already max(overlap, used_overlap), as Micrograph_Autoencoder.denoise makes it."""
    return TilePlan(H, W, cs, overlap, overlap - used_overlap, s_starts(H + 2 * overlap, cs, overlap),
                    s_starts(W + 2 * overlap, cs, overlap))


# ---- device steps -----------------------------------------------------------------------------------------------------------
def prepare(x, mode: int, param: int = 0):
    """x [N,H,W] float32 CUDA -> (prepared images, K's per-image (off, scale, flat) float64 [N,3] or None)."""
    import torch

    N, H, W = x.shape
    lib = _lib.load()
    out = torch.empty((N, param, param) if mode == PREP_D else (N, H, W), dtype=torch.float32, device=x.device)
    stats = torch.empty((N, 3), dtype=torch.float64, device=x.device) if mode == PREP_K else None
    nb = lib.emd_tile_prep_workspace_bytes(N, H, W, mode, param)
    ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
    rc = lib.emd_tile_prep_f32(_lib.ptr(x), _lib.ptr(out), N, H, W, mode, param, None if stats is None else _lib.ptr(stats),
                               _lib.ptr(ws), nb, _lib.stream_ptr())
    _lib.check(rc, "emd_tile_prep_f32")
    return out, stats


def gather(src, plan: TilePlan, dev_plan, t0: int, count: int, out, crop_stats=None):
    """Crops t0 .. t0+count-1 of the plan into out [count,cs,cs] (contiguous); crop_stats [count,2] selects the S rescale."""
    N, H, W = src.shape
    ys, xs = dev_plan[0], dev_plan[1]
    rc = _lib.load().emd_tile_gather_f32(_lib.ptr(src), N, H, W, plan.pad, plan.cs, ys, len(plan.ys), xs, len(plan.xs), t0, count,
                                         _lib.ptr(out), None if crop_stats is None else _lib.ptr(crop_stats), _lib.stream_ptr())
    _lib.check(rc, "emd_tile_gather_f32")
    return out


def blend(preds, plan: TilePlan, dev_plan, N: int, crop_stats=None, clip: bool = False, out=None):
    """preds [N*tiles,cs,cs] -> out [N,H,W] float32."""
    import torch

    if out is None:
        out = torch.empty((N, plan.H, plan.W), dtype=torch.float32, device=preds.device)
    ys, xs, rr, cr = dev_plan
    rc = _lib.load().emd_tile_blend_f32(_lib.ptr(preds), None if crop_stats is None else _lib.ptr(crop_stats), N, plan.H, plan.W,
                                        plan.pad, plan.cs, plan.m, ys, len(plan.ys), xs, len(plan.xs), rr, cr, int(bool(clip)),
                                        _lib.ptr(out), _lib.stream_ptr())
    _lib.check(rc, "emd_tile_blend_f32")
    return out


def affine(x, stats, out=None):
    """K's inverse rescale per image, x [N,H,W]; out may be x."""
    out = x if out is None else out
    N = x.shape[0]
    rc = _lib.load().emd_tile_affine_f32(_lib.ptr(x), _lib.ptr(out), N, x[0].numel(), _lib.ptr(stats), _lib.stream_ptr())
    _lib.check(rc, "emd_tile_affine_f32")
    return out


def run_tiles(src, plan: TilePlan, forward, max_batch: int, rescale: bool = False, clip: bool = False):
    """The tiles of every image of src [N,H,W], gathered in one launch (per 65535 tiles), through ``forward`` ([B,cs,cs,1] CUDA ->
    [B,cs,cs,1]) in batches of at most max_batch, every prediction kept on the device, then one blend -> [N,H,W] float32."""
    import torch

    if max_batch < 1:
        raise ValueError("max_batch must be >= 1")
    N = src.shape[0]
    cs, dev = plan.cs, src.device
    T = N * plan.tiles_per_image
    keep, dev_plan = plan.device_arrays(dev)
    crops = torch.empty((T, cs, cs, 1), dtype=torch.float32, device=dev)
    cstats = torch.empty((T, 2), dtype=torch.float32, device=dev) if rescale else None
    for g0 in range(0, T, _MAX_TILES_PER_LAUNCH):
        n = min(_MAX_TILES_PER_LAUNCH, T - g0)
        gather(src, plan, dev_plan, g0, n, crops[g0:g0 + n], None if cstats is None else cstats[g0:g0 + n])
    # the engines allocate their outputs: each batch's predictions are copied into one buffer for the blend
    preds = torch.empty((T, cs, cs), dtype=torch.float32, device=dev)
    for t0 in range(0, T, max_batch):
        n = min(max_batch, T - t0)
        preds[t0:t0 + n] = forward(crops[t0:t0 + n])[..., 0]
    out = blend(preds, plan, dev_plan, N, cstats, clip)
    del keep  # the plan's device arrays stay allocated until the blend is enqueued
    return out


# ---- containers -------------------------------------------------------------------------------------------------------------
def as_stack(imgs, device):
    """One [H,W] image or an [N,H,W] stack (float32 numpy, or a torch tensor) -> ([N,H,W] float32 contiguous on device, wrap),
    wrap(out) returning out in the caller's container with the caller's leading shape.  A CUDA tensor that already is float32 and
    contiguous on the device is used in place (never written)."""
    import torch

    if isinstance(imgs, torch.Tensor):
        t, kind = imgs, ("cuda" if imgs.is_cuda else "cpu")
    else:
        t, kind = torch.from_numpy(np.ascontiguousarray(np.asarray(imgs, dtype=np.float32))), "numpy"
    if t.dim() not in (2, 3):
        raise ValueError("denoise_images expects an [H,W] image or an [N,H,W] stack")
    single = t.dim() == 2
    x = t.to(device=device, dtype=torch.float32).contiguous()
    if single:
        x = x[None]

    def wrap(y):
        y = y[0] if single else y
        if kind == "numpy":
            return y.cpu().numpy()
        return y.cpu() if kind == "cpu" else y

    return x, wrap


# ---- the three apply classes ------------------------------------------------------------------------------------------------
def denoise_images_d(engine, device, imgs, preprocess=True, postprocess=True, overlap=80, max_batch=32, cropsize=512):
    """Denoiser.denoise per image: optional preprocess to cropsize^2, evenly spaced tiles, mean of the overlapping predictions,
    optional clip to [0,1]."""
    x, wrap = as_stack(imgs, device)
    if preprocess:
        x, _ = prepare(x, PREP_D, cropsize)
    N, H, W = x.shape
    if H < cropsize or W < cropsize:
        raise ValueError("denoise(preprocess=False) needs an image of at least 512x512")
    plan = d_plan(H, W, cropsize, overlap)
    return wrap(run_tiles(x, plan, engine.forward, max_batch, rescale=False, clip=postprocess))


def denoise_images_s(engine, device, imgs, preprocess=True, overlap=25, used_overlap=1, max_batch=64, cropsize=160):
    """autoencoder.Micrograph_Autoencoder.denoise per image: reflect padding by overlap, crops at stride cropsize - 2*overlap,
    each rescaled to minimum 0 / mean 1 and mapped back, centres averaged."""
    x, wrap = as_stack(imgs, device)
    N, H, W = x.shape
    if min(H, W) + 2 * overlap < cropsize:
        raise ValueError("denoise expects a 2-D image of at least cropsize - 2*overlap pixels per side")
    overlap = max(overlap, used_overlap)
    if cropsize - 2 * overlap <= 0:
        raise ValueError("overlap must be less than cropsize / 2")
    if preprocess:
        x, _ = prepare(x, PREP_S)
    plan = s_plan(H, W, cropsize, overlap, used_overlap)
    return wrap(run_tiles(x, plan, engine.forward, max_batch, rescale=True, clip=False))


def denoise_images_k(model, imgs, preprocess=True, postprocess=True):
    """kernel_denoiser.Micrograph_Autoencoder.denoise per image: rescale by the reflect-padded image's statistics, one filter
    launch over the whole stack, inverse rescale."""
    x, wrap = as_stack(imgs, model.device)
    N, H, W = x.shape
    p = model.width // 2   # min(H, W) <= p is refused by the library (EmdError), as the host denoise's filter launch refuses it
    stats = None
    if preprocess:
        x, stats = prepare(x, PREP_K, p)
    den = model._run(x)
    if preprocess and postprocess:
        affine(den, stats)
    return wrap(den)
