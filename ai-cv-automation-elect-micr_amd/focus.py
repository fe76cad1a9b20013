"""Autofocus on the device (csrc/focus.hip): "which image of a through-focus series is in focus" -- the arithmetic
inside the reference's microscope-automation package, em_env/fresnel_env.py:163-208 (``fresnel_quantifier``, ``get_optimal_z``), and
its other per-image quality number, misc_py/entropy.py:36-53 (``image_entropy``).  The text-file mailboxes, the gym and DQN code and
``_get_reward`` of em_env/ need a microscope and are not here.  OpenCV is not used: the Laplacian is restated from its rules
(include/emdenoise.h), not run against OpenCV.

The conventions of ``emdenoise.harvest``: images are float32 ``[H,W]`` or ``[B,H,W]``; numpy in -> numpy out; torch CUDA tensor in ->
device tensor out, on the current stream, with no host synchronisation; arguments are checked on the shape before anything moves to
the device, and an error names the function.  Python here only shapes buffers: every number comes from a HIP kernel."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .metrics import _p, _ws

NMOMENTS = 6   # EMD_NFOCUS
MOMENT_NAMES = ["mean_laplacian", "n", "mean", "m2", "m4", "kurtosis"]
MAX_EXTENT, MAX_BINS = 32768, 4096
MIN_KNOTS, MAX_KNOTS, MAX_FACTOR = 4, 256, 4096


def _is_tensor(a):
    import torch

    return isinstance(a, torch.Tensor)


def _image_dims(name, x, least=2):
    """(B, H, W) of a float32 [H,W] or [B,H,W] argument, checked before anything moves."""
    if not _is_tensor(x) and not isinstance(x, np.ndarray):
        raise ValueError(f"{name}: images are a numpy array or a torch tensor (got {type(x).__name__})")
    shp = tuple(x.shape)
    if len(shp) not in (2, 3):
        raise ValueError(f"{name}: images are [H,W] or [B,H,W] (got shape {shp})")
    if "float32" not in str(x.dtype):
        raise ValueError(f"{name}: images are float32 (got {x.dtype})")
    B, H, W = (1,) + shp if len(shp) == 2 else shp
    if min(H, W) < least or max(H, W) > MAX_EXTENT:
        raise ValueError(f"{name}: {least} <= H, W <= {MAX_EXTENT} (got {H} x {W})")
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


def _check_ksize(name, ksize):
    if ksize not in (1, 3):
        raise ValueError(f"{name}: ksize must be 1 or 3 (got {ksize!r})")
    return int(ksize)


def _check_bins(name, bins):
    if int(bins) != bins or not 2 <= bins <= MAX_BINS or int(bins) & (int(bins) - 1):
        raise ValueError(f"{name}: bins must be a power of two, 2..{MAX_BINS} (got {bins!r})")
    return int(bins)


def laplacian(x, ksize=1):
    """``cv2.Laplacian(x, cv2.CV_32F, ksize=ksize)`` with its default border (BORDER_REFLECT_101), ksize 1 (``[0 1 0; 1 -4 1; 0 1 0]``)
    or 3 (``[2 0 2; 0 -8 0; 2 0 2]``), in float32 in the operation order of include/emdenoise.h -> the shape of x."""
    import torch

    B, H, W = _image_dims("laplacian", x)
    ksize = _check_ksize("laplacian", ksize)
    xd, as_np = _device_images(x)
    y = torch.empty_like(xd)
    _lib.check(_lib.load().emd_laplacian_f32(_p(xd), B, H, W, ksize, _p(y), _lib.stream_ptr()), "emd_laplacian_f32")
    y = y.reshape(tuple(x.shape))
    return y.cpu().numpy() if as_np else y


def _moments_device(xd, ksize, rectify):
    import torch

    B, H, W = (int(s) for s in xd.shape)
    lib = _lib.load()
    out = torch.empty((B, NMOMENTS), dtype=torch.float64, device=xd.device)
    nbytes = lib.emd_laplacian_moments_workspace_bytes(B, H, W)
    ws = _ws(nbytes, xd.device)
    _lib.check(lib.emd_laplacian_moments_f64(_p(xd), B, H, W, ksize, int(bool(rectify)), _p(out), _p(ws), nbytes, _lib.stream_ptr()),
               "emd_laplacian_moments_f64")
    return out


def laplacian_moments(x, ksize=3, rectify=True):
    """``[B, 6]`` float64, the columns named by ``MOMENT_NAMES``, of the Laplacian L of every image (never written to memory): the mean
    of L; the size n of the set S (rectify: the values with ``double(L) >= mean``; else all of them); the mean of S; its population
    central moments m2 and m4 about that mean; ``m4 / m2**2 - 3``.  Two-pass in double in a fixed order: bitwise reproducible, and an
    image's row does not depend on the batch it is in.  A constant image gives m2 = m4 = 0 and NaN in the last column."""
    _image_dims("laplacian_moments", x)
    ksize = _check_ksize("laplacian_moments", ksize)
    xd, as_np = _device_images(x)
    out = _moments_device(xd, ksize, rectify)
    return out.cpu().numpy() if as_np else out


def fresnel_quantifier(x, rectify=True, ksize=3):
    """``fresnel_quantifier`` (fresnel_env.py:163-179): the excess kurtosis (``scipy.stats.kurtosis``: Fisher, biased) of the image's
    Laplacian, by default of the values at or above the Laplacian's mean -> ``[B]`` float64.  Low values indicate the absence of
    Fresnel fringes.  The threshold is the double mean (the reference: numpy's float32 mean)."""
    _image_dims("fresnel_quantifier", x)
    ksize = _check_ksize("fresnel_quantifier", ksize)
    xd, as_np = _device_images(x)
    k = _moments_device(xd, ksize, rectify)[:, NMOMENTS - 1].contiguous()
    return k.cpu().numpy() if as_np else k


def _hist_device(xd, bins, normalize):
    import torch

    B, H, W = (int(s) for s in xd.shape)
    lib = _lib.load()
    counts = torch.empty((B, bins), dtype=torch.int64, device=xd.device)
    nbytes = lib.emd_histogram01_workspace_bytes(B, H, W, int(bool(normalize)))
    ws = _ws(nbytes, xd.device)
    _lib.check(lib.emd_histogram01_i64(_p(xd), B, H, W, bins, int(bool(normalize)), _p(counts), _p(ws), nbytes, _lib.stream_ptr()),
               "emd_histogram01_i64")
    return counts


def histogram01(x, bins=256, normalize=False):
    """``np.histogram(x, bins, range=(0, 1))[0]`` of every image -> int64 ``[B, bins]``; bins a power of two, 2..4096 (every edge is then
    exact).  Values outside [0, 1] and NaN are dropped; 1 goes to the last bin.  normalize=True bins
    ``0.15 * (x - mean) / std + 0.5`` instead (entropy.py:48-49), with the image's own mean and population std, in double."""
    _image_dims("histogram01", x, least=1)
    bins = _check_bins("histogram01", bins)
    xd, as_np = _device_images(x)
    counts = _hist_device(xd, bins, normalize)
    return counts.cpu().numpy() if as_np else counts


def image_entropy(x, num_bins=256, eps=1e-6, normalize=False):
    """``image_entropy`` (entropy.py:36-42): the Shannon entropy in bits of the histogram over [0, 1],
    ``scipy.stats.entropy(hist + eps, base=2)`` -> ``[B]`` float64.  The reference ignores its ``num_bins`` and always uses 256; here
    ``num_bins`` is honoured (a power of two, 2..4096).  normalize=True applies the reference's ``0.15 (x - mean) / std + 0.5``
    (:48-49) first."""
    import torch

    B, _, _ = _image_dims("image_entropy", x, least=1)
    bins = _check_bins("image_entropy", num_bins)
    if not eps >= 0:
        raise ValueError(f"image_entropy: eps must be >= 0 (got {eps!r})")
    xd, as_np = _device_images(x)
    counts = _hist_device(xd, bins, normalize)
    out = torch.empty((B,), dtype=torch.float64, device=xd.device)
    _lib.check(_lib.load().emd_hist_entropy_f64(_p(counts), B, bins, float(eps), _p(out), _lib.stream_ptr()), "emd_hist_entropy_f64")
    return out.cpu().numpy() if as_np else out


def _spline_args(name, z, scores, interp_factor):
    """-> (z host-or-device, scores, N, series shape): shapes and dtypes checked; z increasing only when it is host data."""
    for what, a in (("z", z), ("scores", scores)):
        if _is_tensor(a) and "float64" not in str(a.dtype):
            raise ValueError(f"{name}: {what} is float64 (got {a.dtype})")
    if not _is_tensor(z):
        z = np.ascontiguousarray(z, dtype=np.float64)
    if not _is_tensor(scores):
        scores = np.ascontiguousarray(scores, dtype=np.float64)
    if len(z.shape) != 1:
        raise ValueError(f"{name}: z is [N] (got shape {tuple(z.shape)})")
    N = int(z.shape[0])
    if len(scores.shape) not in (1, 2) or int(scores.shape[-1]) != N:
        raise ValueError(f"{name}: scores are [N] or [B,N] with N = len(z) = {N} (got shape {tuple(scores.shape)})")
    if not MIN_KNOTS <= N <= MAX_KNOTS:
        raise ValueError(f"{name}: the cubic spline needs {MIN_KNOTS} <= N <= {MAX_KNOTS} samples (got {N})")
    if int(interp_factor) != interp_factor or not 1 <= interp_factor <= MAX_FACTOR:
        raise ValueError(f"{name}: interp_factor must be an integer, 1..{MAX_FACTOR} (got {interp_factor!r})")
    if isinstance(z, np.ndarray) and not bool(np.all(np.diff(z) > 0)):
        raise ValueError(f"{name}: z must be strictly increasing")
    return z, scores, N


def _to_device_f64(a, device=None):
    import torch

    t = a if _is_tensor(a) else torch.from_numpy(a)
    if not t.is_cuda:
        t = t.to(device if device is not None else torch.device("cuda", torch.cuda.current_device()))
    return t.contiguous()


def _spline_device(zd, sd, interp_factor, want_curve):
    """z [N], scores [B,N] device float64 -> (zbest [B], curve [B,G] or None, index [B] int64)."""
    import torch

    B, N = (int(s) for s in sd.shape)
    zbest = torch.empty((B,), dtype=torch.float64, device=sd.device)
    index = torch.empty((B,), dtype=torch.int64, device=sd.device)
    curve = torch.empty((B, interp_factor * N), dtype=torch.float64, device=sd.device) if want_curve else None
    _lib.check(_lib.load().emd_spline_argmin_f64(_p(zd), _p(sd), B, N, int(interp_factor), _p(zbest), _p(curve), _p(index),
                                                 _lib.stream_ptr()), "emd_spline_argmin_f64")
    return zbest, curve, index


def optimal_focus(z, scores, interp_factor=10, return_curve=False):
    """``get_optimal_z`` (fresnel_env.py:188-208) without the microscope: the interpolating cubic spline through (z, scores)
    (``InterpolatedUnivariateSpline(z, scores)``: not-a-knot end conditions), evaluated on
    ``np.linspace(z[0], z[-1], interp_factor * len(z))``; the z of the first smallest value.

    z ``[N]`` float64, strictly increasing (checked only when z is host data); scores ``[N]`` or ``[B,N]`` float64, finite.  The
    reference's ``z_incr`` is the NUMBER of samples N (its ``np.linspace(first_z, last_z, self.z_incr)``), not an increment, and the
    spline needs at least four: 4 <= N <= 256.  -> zbest (``[B]``, or a scalar for ``[N]`` scores); with return_curve
    ``(zbest, curve [.., interp_factor * N], index)``, index the grid point's position (int64)."""
    z, scores, _ = _spline_args("optimal_focus", z, scores, interp_factor)
    as_np = not _is_tensor(scores)
    one = len(scores.shape) == 1
    sd = _to_device_f64(scores)
    sd = sd.reshape(1, -1) if one else sd
    zd = _to_device_f64(z, sd.device)
    zbest, curve, index = _spline_device(zd, sd, interp_factor, return_curve)
    outs = [zbest, curve, index] if return_curve else [zbest]
    if one:
        outs = [o[0] for o in outs]
    if as_np:
        outs = [o.cpu().numpy() for o in outs]
    return tuple(outs) if return_curve else outs[0]


def autofocus(stack, z, rectify=True, ksize=3, interp_factor=10):
    """A through-focus series ``[N,H,W]`` taken at the heights z ``[N]`` -> ``(zbest, scores)``: ``fresnel_quantifier`` of every image,
    then ``optimal_focus`` of (z, scores), with no host round trip between them: for a device stack (and a device z) the whole
    sequence is launches on the current stream and can be captured in a graph.  zbest is a scalar, scores ``[N]`` float64."""
    B, _, _ = _image_dims("autofocus", stack)
    if len(stack.shape) != 3:
        raise ValueError(f"autofocus: the stack is [N,H,W] (got shape {tuple(stack.shape)})")
    ksize = _check_ksize("autofocus", ksize)
    if not _is_tensor(z):
        z = np.ascontiguousarray(z, dtype=np.float64)
    if len(z.shape) != 1 or int(z.shape[0]) != B:
        raise ValueError(f"autofocus: z is [N] with N = {B} images (got shape {tuple(z.shape)})")
    z, _, _ = _spline_args("autofocus", z, np.zeros(B), interp_factor)
    xd, as_np = _device_images(stack)
    scores = _moments_device(xd, ksize, rectify)[:, NMOMENTS - 1].contiguous()
    zbest = _spline_device(_to_device_f64(z, xd.device), scores.reshape(1, B), interp_factor, False)[0][0]
    return (zbest.cpu().numpy(), scores.cpu().numpy()) if as_np else (zbest, scores)
