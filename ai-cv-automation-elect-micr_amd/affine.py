"""Affine registration of a focal series by mutual information, and warping, on the device (csrc/affine.hip): the
reference's ``misc_py/evolutionary_align.m`` (``imregtform`` with ``imregconfig('multimodal')``: Mattes mutual information on random
samples under a (1+1) evolutionary optimizer) and ``misc_py/warp_stack.m`` (the pair transforms chained onto the middle image,
``imwarp``, the rectangle common to all warped images).  MATLAB is not run: the formulas of include/emdenoise.h are the specification.
A through-focus series drifts, rotates, changes magnification and reverses its contrast; ``exitwave.align`` finds translations only.

Conventions.  Images are float32 ``[N,H,W]``, H and W 8..4096 each.  Pixel coordinates are zero-based (x, y); with
``c = ((W-1)/2, (H-1)/2)`` and ``h = max(H, W)/2`` the normalised coordinates are ``u = (x - cx)/h``, ``v = (y - cy)/h``.  A transform T is
``[2,3]`` float64 in normalised coordinates and a pull map: it takes a point of the fixed (output) frame to the point of the moving
(input) frame that is sampled there.  The optimizer's six parameters are ``p = T - [I | 0]``.  ``to_pixel_matrix`` gives the 3 x 3
matrix in pixel coordinates; MATLAB's ``tform.T`` is the transpose of its inverse.

The parameters carry from one level of a factor-2 pyramid to the next unchanged.  ``harvest.box_resize`` averages 2 x 2 blocks: coarse
pixel X stands at the fine coordinate 2X + 1/2.  For an even W the coarse centre is ``(W/2 - 1)/2`` and the coarse h is ``h/2``, so the
coarse pixel's normalised coordinate is ``(X - (W/2 - 1)/2)/(h/2) = (2X + 1/2 - (W - 1)/2)/h``: that of the point it stands at, exactly.
The same holds for y; a T that aligns the fine images aligns the coarse ones.  It is why H and W must be divisible by 2^(levels-1).

numpy in -> numpy out; torch CUDA tensor in -> device tensor out, on the current stream, with no host synchronisation.  Arguments are
checked before anything moves to the device.  A float64 CUDA tensor of transforms (and int32 samples, float64 variates) is used where
it is: such calls can be captured in a ``torch.cuda.graph``; anything else is uploaded before the call, which a capture does not allow.
Two runs give the same bits.

Deviations from the reference: the pull-map convention and the normalised parameters (MATLAB's optimizer scales are internal to it);
the histogram is 64-bit fixed point, so that it is a sum of integers; ``warp_stack.m`` as committed does not run (its loop
``(mid-2):1`` is empty, the right-hand images use ``left_trans``, ``crop_limits`` reads an undefined image) and ``int32(L/2)+1`` is not
the middle for odd L (here ``N // 2``); the corner box of ``common_limits`` is the reference's heuristic, not the exact inscribed
rectangle; ``imregtform``'s moment-based initialisation and its pyramid smoothing are not restated."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .metrics import _p, _ws

MIN_SIDE, MAX_SIDE, MAX_PAIRS, MAX_IMAGES = 8, 4096, 64, 65535
MIN_BINS, MAX_BINS = 8, 64
STATE_DOUBLES = 64                          # EMD_AFFINE_STATE_DOUBLES
MI_CONSTANT, MI_EMPTY = 1, 2                # EMD_MI_*
CONVERGED, DEGENERATE, EXHAUSTED = 1, 2, 4  # EMD_AFFINE_* status words
RESET, NEXT_LEVEL = 1, 2                    # EMD_AFFINE_* flags
MAX_ITERATIONS = 1 << 20
# the slots of a pair's state (include/emdenoise.h)
_X, _A, _N, _CHILD, _F, _MI, _ITER, _ACCEPTED, _STATUS, _WEIGHT = 0, 6, 42, 48, 54, 55, 56, 57, 58, 59


def geometry(H, W):
    """(cx, cy, h)."""
    return (W - 1) / 2, (H - 1) / 2, max(H, W) / 2


def to_pixel_matrix(T, H, W):
    """The 3 x 3 matrix, on column vectors (x, y, 1) of zero-based pixel coordinates, of the pull map T ``[2,3]`` (normalised).  On the
    host.  MATLAB's ``tform.T`` is the transpose of its inverse (one-based coordinates aside)."""
    T = np.asarray(T.detach().cpu() if hasattr(T, "detach") else T, np.float64).reshape(2, 3)
    _hw("to_pixel_matrix", H, W)
    cx, cy, h = geometry(H, W)
    M = np.eye(3)
    M[:2, :2] = T[:, :2]
    M[0, 2] = T[0, 2] * h + cx - T[0, 0] * cx - T[0, 1] * cy
    M[1, 2] = T[1, 2] * h + cy - T[1, 0] * cx - T[1, 1] * cy
    return M


def from_similarity(angle_deg, scale, shift_px, H, W):
    """The pull map that samples the moving image at ``scale R(angle) (point - c) + c + shift_px``: ``[2,3]`` float64, on the host."""
    _, _, h = geometry(H, W)
    a = np.deg2rad(angle_deg)
    return np.array([[scale * np.cos(a), -scale * np.sin(a), shift_px[0] / h], [scale * np.sin(a), scale * np.cos(a), shift_px[1] / h]])


# ---- argument checks, before anything moves ----------------------------------------------------------------------------------------

def _hw(name, H, W):
    if int(H) != H or int(W) != W or not (MIN_SIDE <= H <= MAX_SIDE and MIN_SIDE <= W <= MAX_SIDE):
        raise ValueError(f"{name}: H and W must be integers, {MIN_SIDE}..{MAX_SIDE} (got {H!r} x {W!r})")


def _images(name, a, max_images=MAX_IMAGES, min_images=1):
    """(N, H, W, ndim) of an [N,H,W] or [H,W] argument."""
    import torch

    shp = tuple(a.shape) if hasattr(a, "shape") else np.shape(a)
    ndim = len(shp)
    if ndim == 2:
        shp = (1,) + shp
    if len(shp) != 3:
        raise ValueError(f"{name}: images are [N,H,W] or [H,W] (got a shape of {ndim} dimensions)")
    _hw(name, shp[1], shp[2])
    if not min_images <= shp[0] <= max_images:
        raise ValueError(f"{name}: {min_images}..{max_images} images (got {shp[0]})")
    if isinstance(a, torch.Tensor) and a.is_complex() or not isinstance(a, torch.Tensor) and np.iscomplexobj(a):
        raise ValueError(f"{name}: the images are real (float32)")
    return int(shp[0]), int(shp[1]), int(shp[2]), ndim


def _device(a):
    import torch

    return a.device if isinstance(a, torch.Tensor) and a.is_cuda else torch.device("cuda", torch.cuda.current_device())


def _real(a, device, N, H, W):
    """-> (contiguous float32 CUDA tensor [N,H,W], was_numpy)."""
    import torch

    is_np = not isinstance(a, torch.Tensor)
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)) if is_np else a
    return t.to(device=device, dtype=torch.float32).reshape(N, H, W).contiguous(), is_np


def _on_device(name, what, a, dtype, shape, device):
    """A contiguous CUDA tensor of ``dtype`` and ``shape`` is used where it is; anything else is uploaded (not while capturing)."""
    import torch

    if isinstance(a, torch.Tensor) and a.is_cuda:
        if a.dtype != dtype or tuple(a.shape) != tuple(shape) or not a.is_contiguous():
            raise ValueError(f"{name}: device {what} must be a contiguous {dtype} tensor of shape {tuple(shape)} (got {a.dtype}, "
                             f"{tuple(a.shape)})")
        return a
    arr = np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a)
    if arr.shape != tuple(shape):
        raise ValueError(f"{name}: {what} has the shape {tuple(shape)} (got {arr.shape})")
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f"{name}: {what} is not on the device; pass a CUDA tensor when capturing")
    return torch.from_numpy(np.ascontiguousarray(arr)).to(device=device, dtype=dtype).contiguous()


def _transform_shape(name, T, count, shared_ok=False):
    """-> count of transforms (1 when shared) of a [count,2,3], [count,6], [2,3] or [6] argument."""
    shp = tuple(T.shape) if hasattr(T, "shape") else np.shape(T)
    if shp in ((2, 3), (6,)) and (shared_ok or count == 1):
        return 1
    if shp in ((count, 2, 3), (count, 6)):
        return count
    raise ValueError(f"{name}: transforms are [{count},2,3]" + (" or one [2,3] for all" if shared_ok else "") + f" (got {shp})")


def _transforms(name, T, k, device):
    import torch

    shp = tuple(T.shape) if hasattr(T, "shape") else np.shape(T)
    t = _on_device(name, "the transforms", T, torch.float64, shp, device)
    return t.reshape(k, 6)


def _bins(name, bins):
    if int(bins) != bins or not MIN_BINS <= bins <= MAX_BINS:
        raise ValueError(f"{name}: bins must be an integer, {MIN_BINS}..{MAX_BINS} (got {bins!r})")
    return int(bins)


def _seed(name, seed):
    if int(seed) != seed or not 0 <= seed < 1 << 64:
        raise ValueError(f"{name}: seed must be an integer, 0..2^64-1 (got {seed!r})")
    return int(seed)


# ---- the warp ----------------------------------------------------------------------------------------------------------------------

def _warp(x, t, shared, fill):
    import torch

    N, H, W = x.shape
    out = torch.empty_like(x)
    _lib.check(_lib.load().emd_warp_affine_f32(_p(x), N, H, W, _p(t), int(shared), float(fill), _p(out), _lib.stream_ptr()),
               "emd_warp_affine_f32")
    return out


def warp(images, T, fill=0.0):
    """``imwarp(img, T, 'OutputView', imref2d(size(img)))`` with linear interpolation: every output pixel goes through its image's pull
    map T and takes the bilinear value there; a tap outside the image reads ``fill``.  ``T``: ``[N,2,3]``, or one ``[2,3]`` shared by all
    images.  float32, the shape of ``images``."""
    N, H, W, ndim = _images("warp", images)
    k = _transform_shape("warp", T, N, shared_ok=True)
    if not np.isfinite(fill):
        raise ValueError(f"warp: fill must be finite (got {fill!r})")
    device = _device(images)
    t = _transforms("warp", T, k, device)
    x, as_np = _real(images, device, N, H, W)
    out = _warp(x, t, k == 1, fill)
    out = out.reshape(H, W) if ndim == 2 else out
    return out.cpu().numpy() if as_np else out


# ---- the metric --------------------------------------------------------------------------------------------------------------------

def draw_samples(n, H, W, seed=0):
    """n pixel indices ``y W + x`` drawn with replacement: ``mulhi32(r_i, H W)`` with r_i the i-th word of the Philox stream of ``seed``
    (counter (i / 4, 0, 0, 7)).  A device int32 tensor ``[n]`` (the indices are below 2^24)."""
    import torch

    _hw("draw_samples", H, W)
    if int(n) != n or not 1 <= n <= 4 * H * W:
        raise ValueError(f"draw_samples: n must be an integer, 1..4 H W (got {n!r})")
    seed = _seed("draw_samples", seed)
    out = torch.empty((int(n),), dtype=torch.int32, device=torch.device("cuda", torch.cuda.current_device()))
    _lib.check(_lib.load().emd_mi_samples_u32(int(n), int(H), int(W), seed, _p(out), _lib.stream_ptr()), "emd_mi_samples_u32")
    return out


def _check_samples(name, samples, H, W):
    """n of a [n] argument of pixel indices (0 for None), checked before anything moves."""
    import torch

    if samples is None:
        return 0
    shp = tuple(samples.shape) if hasattr(samples, "shape") else np.shape(samples)
    if len(shp) != 1 or not 1 <= shp[0] <= 4 * H * W:
        raise ValueError(f"{name}: samples are [n] pixel indices, 1 <= n <= 4 H W (got a shape of {shp})")
    if isinstance(samples, torch.Tensor) and samples.is_cuda:
        if samples.dtype != torch.int32 or not samples.is_contiguous():
            raise ValueError(f"{name}: device samples must be a contiguous int32 tensor")
    else:
        arr = np.asarray(samples.cpu() if isinstance(samples, torch.Tensor) else samples)
        if arr.dtype.kind not in "iu" or arr.min() < 0 or arr.max() >= H * W:
            raise ValueError(f"{name}: samples are integers inside the image, 0..H W - 1")
    return int(shp[0])


def _samples(name, samples, n, device):
    """-> int32 CUDA tensor [n], or None."""
    import torch

    if samples is None or isinstance(samples, torch.Tensor) and samples.is_cuda:
        return samples
    arr = np.asarray(samples.cpu() if isinstance(samples, torch.Tensor) else samples).astype(np.int32)
    return _on_device(name, "samples", arr, torch.int32, (n,), device)


def mutual_information(fixed, moving, T, samples=None, bins=50, return_histogram=False, return_status=False):
    """Mattes mutual information of every pair ``(fixed[p], moving[p])`` (``[P,H,W]``, 1 <= P <= 64; or ``[H,W]``: one pair) under the
    candidate pull map ``T[p]``: float64 ``[P]`` (a 0-d result for one ``[H,W]`` pair).  ``samples``: None for every fixed pixel, or pixel
    indices ``[n]`` (``draw_samples``), shared by the pairs.  The joint histogram has ``bins`` x ``bins`` cells (8..64), the moving
    image enters through a cubic B-spline Parzen window, and the counts are 64-bit fixed point (2^32 per unit weight), so the
    histogram is exact.  ``return_histogram`` adds it (int64 ``[P,bins,bins]``), ``return_status`` the status words (int32 ``[P]``:
    ``MI_EMPTY`` no sample inside, ``MI_CONSTANT`` a constant image; MI is 0 in both cases)."""
    import torch

    P, H, W, ndim = _images("mutual_information", fixed, MAX_PAIRS)
    if _images("mutual_information", moving, MAX_PAIRS)[:3] != (P, H, W):
        raise ValueError("mutual_information: fixed and moving must have the same shape")
    _transform_shape("mutual_information", T, P)
    bins = _bins("mutual_information", bins)
    n = _check_samples("mutual_information", samples, H, W)
    device = _device(fixed)
    smp = _samples("mutual_information", samples, n, device)
    t = _transforms("mutual_information", T, P, device)
    f, as_np = _real(fixed, device, P, H, W)
    m, _ = _real(moving, device, P, H, W)
    lib = _lib.load()
    mi = torch.empty((P,), dtype=torch.float64, device=device)
    status = torch.empty((P,), dtype=torch.int32, device=device)
    hist = torch.empty((P, bins, bins), dtype=torch.int64, device=device) if return_histogram else None
    nbytes = lib.emd_mattes_mi_workspace_bytes(P, H, W, n, bins)
    ws = _ws(nbytes, device)
    _lib.check(lib.emd_mattes_mi_f64(_p(f), _p(m), P, H, W, _p(t), _p(smp), n, bins, _p(mi), _p(status), _p(hist), _p(ws), nbytes,
                                     _lib.stream_ptr()), "emd_mattes_mi_f64")
    outs = [mi[0] if ndim == 2 else mi] + ([hist[0] if ndim == 2 else hist] if return_histogram else [])
    outs += [status[0] if ndim == 2 else status] if return_status else []
    outs = [o.cpu().numpy() if as_np else o for o in outs]
    return outs[0] if len(outs) == 1 else tuple(outs)


# ---- the optimizer -----------------------------------------------------------------------------------------------------------------

def normals(iterations, P, seed=0, first_iteration=0):
    """The optimizer's normal variates, float64 ``[iterations,P,6]`` on the device: Box-Muller on the Philox stream of ``seed``, the
    bits that ``register`` draws (counter (iteration, pair, draw, 8), three draws of two normals each)."""
    import torch

    if int(iterations) != iterations or not 1 <= iterations <= MAX_ITERATIONS or int(P) != P or not 1 <= P <= MAX_PAIRS:
        raise ValueError(f"normals: 1..{MAX_ITERATIONS} iterations and 1..{MAX_PAIRS} pairs (got {iterations!r}, {P!r})")
    if int(first_iteration) != first_iteration or first_iteration < 0:
        raise ValueError(f"normals: first_iteration must be a non-negative integer (got {first_iteration!r})")
    seed = _seed("normals", seed)
    out = torch.empty((int(iterations), int(P), 6), dtype=torch.float64, device=torch.device("cuda", torch.cuda.current_device()))
    _lib.check(_lib.load().emd_affine_normals_f64(int(iterations), int(P), int(first_iteration), seed, _p(out), _lib.stream_ptr()),
               "emd_affine_normals_f64")
    return out


def _optimizer_args(name, iterations, bins, initial_radius, growth, epsilon, seed):
    if int(iterations) != iterations or not 0 <= iterations <= MAX_ITERATIONS:
        raise ValueError(f"{name}: iterations must be an integer, 0..{MAX_ITERATIONS} (got {iterations!r})")
    if not (np.isfinite(initial_radius) and initial_radius > 0):
        raise ValueError(f"{name}: initial_radius must be positive and finite (got {initial_radius!r})")
    if not (np.isfinite(growth) and growth > 1):
        raise ValueError(f"{name}: growth must be finite and above 1 (got {growth!r})")
    if not (np.isfinite(epsilon) and epsilon >= 0):
        raise ValueError(f"{name}: epsilon must be finite and not negative (got {epsilon!r})")
    return int(iterations), _bins(name, bins), _seed(name, seed)


def iterate(fixed, moving, state=None, iterations=1, samples=None, bins=50, initial_radius=6.25e-3, growth=1.05, epsilon=1.5e-6, seed=0,
            variates=None, reset=False, next_level=False, T0=None, first_iteration=0, workspace=None):
    """``iterations`` evaluations of the (1+1) evolution strategy on the device state ``[P,64]`` float64 (``state_fields`` names its
    slots), two launches each for all pairs, after two launches for the images' extrema: one C call, nothing read back.  ``fixed`` and
    ``moving`` are float32 CUDA tensors ``[P,H,W]``.  ``reset`` starts from ``T0`` (a float64 CUDA tensor ``[P,2,3]``, or None: the
    identity) with the evaluation counter at ``first_iteration``; ``next_level`` keeps the parameters and the counters and resets the
    matrix and the status; neither continues where the state stands, which is what a captured block does on replay.  ``state=None``
    allocates one (and needs ``reset``).  ``variates`` (float64 CUDA ``[rows,P,6]``) replaces the Philox normals: evaluation t uses row t.
    Returns the state."""
    import torch

    name = "iterate"
    P, H, W, _ = _images(name, fixed, MAX_PAIRS)
    if _images(name, moving, MAX_PAIRS)[:3] != (P, H, W):
        raise ValueError(f"{name}: fixed and moving must have the same shape")
    iterations, bins, seed = _optimizer_args(name, iterations, bins, initial_radius, growth, epsilon, seed)
    for what, t in (("fixed", fixed), ("moving", moving)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError(f"{name}: {what} must be a contiguous float32 CUDA tensor")
    if reset and next_level:
        raise ValueError(f"{name}: reset or next_level, not both")
    if state is None and not reset:
        raise ValueError(f"{name}: a new state needs reset=True")
    if T0 is not None and not reset:
        raise ValueError(f"{name}: T0 is read by a reset only")
    if int(first_iteration) != first_iteration or first_iteration < 0:
        raise ValueError(f"{name}: first_iteration must be a non-negative integer (got {first_iteration!r})")
    n = _check_samples(name, samples, H, W)
    device = fixed.device
    rows = 0
    if variates is not None:
        shp = tuple(variates.shape)
        if len(shp) != 3 or shp[1:] != (P, 6) or shp[0] < 1:
            raise ValueError(f"{name}: variates are [rows,{P},6] (got {shp})")
        rows = int(shp[0])
    if T0 is not None:
        _transform_shape(name, T0, P)
    if state is not None and not (isinstance(state, torch.Tensor) and state.is_cuda and state.dtype == torch.float64
                                  and state.is_contiguous() and tuple(state.shape) == (P, STATE_DOUBLES)):
        raise ValueError(f"{name}: state must be a contiguous float64 CUDA tensor [{P},{STATE_DOUBLES}]")
    smp = _samples(name, samples, n, device)
    if variates is not None:
        variates = _on_device(name, "variates", variates, torch.float64, shp, device)
    if T0 is not None:
        T0 = _transforms(name, T0, P, device)
    if state is None:
        state = torch.zeros((P, STATE_DOUBLES), dtype=torch.float64, device=device)
    lib = _lib.load()
    nbytes = lib.emd_mattes_mi_workspace_bytes(P, H, W, n, bins)
    ws = workspace if workspace is not None else _ws(nbytes, device)
    if ws.numel() * ws.element_size() < nbytes:
        raise ValueError(f"{name}: the workspace holds {ws.numel() * ws.element_size()} bytes, {nbytes} are needed")
    flags = RESET if reset else NEXT_LEVEL if next_level else 0
    _lib.check(lib.emd_affine_register_f64(_p(fixed), _p(moving), P, H, W, _p(smp), n, bins, float(initial_radius), float(growth),
                                           float(epsilon), seed, _p(variates), rows, flags, _p(T0), int(first_iteration), iterations,
                                           _p(state), _p(ws), nbytes, _lib.stream_ptr()), "emd_affine_register_f64")
    return state


def state_fields(state):
    """The named slots of an optimizer state ``[P,64]``: x ``[P,6]``, T ``[P,2,3]`` (= [I | 0] + x), A ``[P,6,6]``, f, mi (the last
    value), and int64 iterations (evaluations done), accepted, status (0, ``CONVERGED``, ``DEGENERATE``, ``EXHAUSTED``), weight (the
    histogram's sum at the last evaluation).  Views and small device tensors; nothing is read back."""
    import torch

    ints = state.view(torch.int64)
    x = state[:, _X:_X + 6]
    eye = torch.tensor([1.0, 0, 0, 0, 1.0, 0], dtype=torch.float64, device=state.device)
    return {"x": x, "T": (x + eye).reshape(-1, 2, 3), "A": state[:, _A:_A + 36].reshape(-1, 6, 6), "n": state[:, _N:_N + 6],
            "child": state[:, _CHILD:_CHILD + 6], "f": state[:, _F], "mi": state[:, _MI], "iterations": ints[:, _ITER],
            "accepted": ints[:, _ACCEPTED], "status": ints[:, _STATUS], "weight": ints[:, _WEIGHT]}


def register(fixed, moving, iterations=1000, samples=250000, bins=50, initial_radius=6.25e-3, growth=1.05, epsilon=1.5e-6, seed=0, levels=3,
             T0=None, variates=None, return_state=False):
    """``imregtform(moving, fixed, 'affine', optimizer, metric)`` with ``imregconfig('multimodal')``'s optimizer and metric, for every
    pair ``(fixed[p], moving[p])`` (``[P,H,W]``, 1 <= P <= 64; or ``[H,W]``) at once: the pull maps ``[P,2,3]`` float64 that maximise
    the mutual information.  The defaults are MATLAB's and the reference's (evolutionary_align.m:52-57).

    ``samples``: the number of random samples (drawn with ``seed``; every pixel where that is not more), None for every pixel, or
    (``levels=1`` only) pixel indices.  ``levels``: a factor-2 pyramid by ``harvest.box_resize``, coarsest first; the normalised
    parameters carry over unchanged (see the module's docstring), the matrix A is reset and the iterations are split evenly (the
    remainder goes to the finest level); H and W must be divisible by 2^(levels-1) and stay >= 8.  ``T0``: the starting transforms.
    ``variates`` ``[iterations,P,6]`` replaces the Philox normals.  Nothing is read back before the call returns; with
    ``return_state`` the device state ``[P,64]`` (``state_fields``) is returned as well."""
    import torch

    from . import harvest

    name = "register"
    P, H, W, ndim = _images(name, fixed, MAX_PAIRS)
    if _images(name, moving, MAX_PAIRS)[:3] != (P, H, W):
        raise ValueError(f"{name}: fixed and moving must have the same shape")
    iterations, bins, seed = _optimizer_args(name, iterations, bins, initial_radius, growth, epsilon, seed)
    if int(levels) != levels or levels < 1:
        raise ValueError(f"{name}: levels must be a positive integer (got {levels!r})")
    levels = int(levels)
    f = 1 << (levels - 1)
    if H % f or W % f or H // f < MIN_SIDE or W // f < MIN_SIDE:
        raise ValueError(f"{name}: H and W must be divisible by 2^(levels-1) = {f} and stay >= {MIN_SIDE} there (got {H} x {W})")
    if levels > 1 and H != W:
        raise ValueError(f"{name}: the pyramid (harvest.box_resize) is for square images; use levels=1 for {H} x {W}")
    if iterations < levels:
        raise ValueError(f"{name}: at least one iteration per level (got {iterations} for {levels} levels)")
    count = None
    if samples is not None and np.ndim(samples) == 0 and not hasattr(samples, "shape"):
        if int(samples) != samples or samples < 1:
            raise ValueError(f"{name}: samples must be a positive integer, None or an array of indices (got {samples!r})")
        count, samples = int(samples), None
    elif samples is not None and levels > 1:
        raise ValueError(f"{name}: sample indices belong to one image size; use levels=1 or a count")
    elif samples is not None:
        _check_samples(name, samples, H, W)
    if T0 is not None:
        _transform_shape(name, T0, P)
    if variates is not None and tuple(variates.shape) != (iterations, P, 6):
        raise ValueError(f"{name}: variates are [iterations,P,6] = [{iterations},{P},6] (got {tuple(variates.shape)})")
    device = _device(fixed)
    fx, as_np = _real(fixed, device, P, H, W)
    mv, _ = _real(moving, device, P, H, W)
    if variates is not None:
        variates = _on_device(name, "variates", variates, torch.float64, (iterations, P, 6), device)
    if T0 is not None:
        T0 = _transforms(name, T0, P, device)
    pyramid = [(fx, mv)]
    for _ in range(levels - 1):
        a, b = pyramid[0]
        pyramid.insert(0, (harvest.box_resize(a, a.shape[-1] // 2), harvest.box_resize(b, b.shape[-1] // 2)))
    per, state, done = iterations // levels, None, 0
    for lv, (a, b) in enumerate(pyramid):
        k = per if lv < levels - 1 else iterations - done
        h, w = int(a.shape[1]), int(a.shape[2])
        smp = samples if count is None else (draw_samples(count, h, w, seed) if count < h * w else None)
        state = iterate(a, b, state, k, smp, bins, initial_radius, growth, epsilon, seed, variates, reset=lv == 0, next_level=lv > 0,
                        T0=T0 if lv == 0 else None)
        done += k
    T = state_fields(state)["T"]
    T = T[0] if ndim == 2 else T
    T = T.cpu().numpy() if as_np else T
    return (T, state) if return_state else T


def register_series(stack, **kw):
    """``evolutionary_align.m:43-66``: image k+1 (moving) is registered onto image k (fixed) for k = 0..N-2, all pairs in the same
    launches.  ``stack`` ``[N,H,W]``, 2 <= N <= 65; keywords as ``register`` has them.  ``[N-1,2,3]``."""
    N, H, W, _ = _images("register_series", stack, MAX_PAIRS + 1, 2)
    x, as_np = _real(stack, _device(stack), N, H, W)
    out = register(x[:-1], x[1:], **kw)
    if not as_np:
        return out
    return (out[0].cpu().numpy(), out[1]) if isinstance(out, tuple) else out.cpu().numpy()


# ---- onto the middle image ---------------------------------------------------------------------------------------------------------

def _middle(name, middle, N):
    middle = N // 2 if middle is None else middle
    if int(middle) != middle or not 0 <= middle < N:
        raise ValueError(f"{name}: middle must be an integer, 0..{N - 1} (got {middle!r})")
    return int(middle)


def _pairs(name, T_pairs):
    shp = tuple(T_pairs.shape) if hasattr(T_pairs, "shape") else np.shape(T_pairs)
    if len(shp) not in (2, 3) or shp[1:] not in ((2, 3), (6,)) or not 1 <= shp[0] <= MAX_PAIRS:
        raise ValueError(f"{name}: pair transforms are [N-1,2,3], 1..{MAX_PAIRS} of them (got {shp})")
    return int(shp[0]) + 1


def _chain(t, N, middle):
    import torch

    Cm = torch.empty((N, 2, 3), dtype=torch.float64, device=t.device)
    _lib.check(_lib.load().emd_affine_chain_f64(_p(t), N, middle, _p(Cm), _lib.stream_ptr()), "emd_affine_chain_f64")
    return Cm


def chain_to_middle(T_pairs, middle=None):
    """The pull maps ``[N,2,3]`` of every image onto the frame of image ``middle`` (default N // 2) from the pair transforms
    ``[N-1,2,3]`` (pair k: fixed k, moving k + 1): ``C_middle = I``, ``C_j = M_{j-1} C_{j-1}`` above it and ``C_j = inv(M_j) C_{j+1}`` below.
    A singular or non-finite pair transform gives NaNs from there outwards."""
    import torch

    N = _pairs("chain_to_middle", T_pairs)
    middle = _middle("chain_to_middle", middle, N)
    as_np = not isinstance(T_pairs, torch.Tensor)
    t = _transforms("chain_to_middle", T_pairs, N - 1, _device(T_pairs))
    Cm = _chain(t, N, middle)
    return Cm.cpu().numpy() if as_np else Cm


def _limits(c, N, H, W):
    import torch

    out = torch.empty((4,), dtype=torch.int32, device=c.device)
    _lib.check(_lib.load().emd_affine_limits_i32(_p(c), N, H, W, _p(out), _lib.stream_ptr()), "emd_affine_limits_i32")
    return out


def common_limits(C_maps, H, W):
    """The rectangle common to all images warped with ``C_maps`` ``[N,2,3]`` (warp_stack.m:112-150 applied to every image and
    intersected): int32 ``[x0, y0, w, h]``; w or h is 0 where there is none, and all four are 0 for a singular or non-finite map."""
    import torch

    _hw("common_limits", H, W)
    shp = tuple(C_maps.shape) if hasattr(C_maps, "shape") else np.shape(C_maps)
    if len(shp) not in (2, 3) or shp[1:] not in ((2, 3), (6,)) or not 1 <= shp[0] <= MAX_PAIRS + 1:
        raise ValueError(f"common_limits: the maps are [N,2,3], 1..{MAX_PAIRS + 1} of them (got {shp})")
    as_np = not isinstance(C_maps, torch.Tensor)
    c = _transforms("common_limits", C_maps, shp[0], _device(C_maps))
    out = _limits(c, int(shp[0]), int(H), int(W))
    return out.cpu().numpy() if as_np else out


def warp_stack(stack, T_pairs, middle=None, crop=False, fill=0.0):
    """``warp_stack.m``: every image of ``stack`` ``[N,H,W]`` warped onto the frame of image ``middle`` with ``chain_to_middle(T_pairs)``.
    ``crop``: cut to ``common_limits``, which reads the four integers back once (refused inside a capture)."""
    import torch

    N, H, W, _ = _images("warp_stack", stack, MAX_PAIRS + 1, 2)
    if _pairs("warp_stack", T_pairs) != N:
        raise ValueError(f"warp_stack: {N} images need [{N - 1},2,3] pair transforms")
    middle = _middle("warp_stack", middle, N)
    if not np.isfinite(fill):
        raise ValueError(f"warp_stack: fill must be finite (got {fill!r})")
    if crop and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("warp_stack: crop=True reads the limits back, which a capture does not allow")
    device = _device(stack)
    t = _transforms("warp_stack", T_pairs, N - 1, device)
    x, as_np = _real(stack, device, N, H, W)
    Cm = _chain(t, N, middle)
    out = _warp(x, Cm.reshape(N, 6), False, fill)
    if crop:
        x0, y0, w, h = (int(v) for v in _limits(Cm.reshape(N, 6), N, H, W).cpu())
        out = out[:, y0:y0 + h, x0:x0 + w].contiguous()
    return out.cpu().numpy() if as_np else out


def align(stack, middle=None, crop=False, fill=0.0, **register_kw):
    """``register_series`` followed by ``warp_stack``: ``(aligned [N,H,W] float32, T_pairs [N-1,2,3] float64)``.  With a CUDA stack and
    ``crop=False`` nothing is read back: the result feeds ``exitwave.crop_stack`` and ``exitwave.reconstruct`` on the device."""
    pairs = register_series(stack, **register_kw)
    return warp_stack(stack, pairs, middle, crop, fill), pairs
