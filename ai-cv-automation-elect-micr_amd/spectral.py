"""The 2-D FFT of any side on the device (csrc/fft_any.hip): ``numpy.fft.fft2`` / ``ifft2`` / ``rfft2`` and Fresnel
propagation of ``[B,H,W]`` (or ``[H,W]``) with H and W independent, in double precision (complex128).

Each side is 2..2048, or a power of two up to 4096.  A power of two, 8..4096, is the Stockham line that ``exitwave.fft2`` runs (the
same bits on a square); any other side is Bluestein's chirp-z transform on two power-of-two lines of ``line_length(n)`` elements.
``exitwave``, ``harvest``, ``register`` and ``psiart`` keep their own limit, a square whose side is a power of two.

numpy in -> numpy out; torch CUDA tensor in -> device tensor out, on the current stream, with no host synchronisation; arguments are
checked on shape and dtype before anything moves to the device.  A defocus argument that is a float64 CUDA tensor is used where it
is: such calls can be captured in a ``torch.cuda.graph`` and replayed after the tensor is overwritten.  Anything else is uploaded
before the call, which a capture does not allow."""
from __future__ import annotations

import numpy as np

from . import _lib
from .exitwave import _defocus, _device, _positive, _ret, _wave
from .metrics import _p, _ws

MIN_SIDE, MAX_SIDE, MAX_POW2_SIDE, MAX_BATCH = 2, 2048, 4096, 65535
RULE = "each side 2..2048, or a power of two up to 4096"


def line_length(n):
    """The length of the LDS line that a transform of length ``n`` occupies (``emd_fft_any_line``, restated on the host): ``n`` for a
    power of two 8..4096; ``max(8, the smallest power of two >= 2 n - 1)`` for any other n in 2..2048; 0 for an n that is not served."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)):
        raise ValueError(f"line_length: n must be an integer (got {n!r})")
    n = int(n)
    if 8 <= n <= MAX_POW2_SIDE and n & (n - 1) == 0:
        return n
    if not MIN_SIDE <= n <= MAX_SIDE:
        return 0
    M = 8
    while M < 2 * n - 1:
        M <<= 1
    return M


def _shape(name, a):
    """(B, H, W, ndim) of a [B,H,W] or [H,W] argument, before anything is moved to the device."""
    shp = tuple(a.shape) if hasattr(a, "shape") else np.shape(a)
    ndim = len(shp)
    if ndim == 2:
        shp = (1,) + shp
    if len(shp) != 3:
        raise ValueError(f"{name}: [B,H,W] or [H,W] (got a shape of {ndim} dimensions)")
    B, H, W = (int(v) for v in shp)
    if not line_length(H) or not line_length(W):
        raise ValueError(f"{name}: {RULE} (got {H} x {W})")
    if not 1 <= B <= MAX_BATCH:
        raise ValueError(f"{name}: 1..{MAX_BATCH} images (got {B})")
    return B, H, W, ndim


def _is_complex(a):
    return a.is_complex() if hasattr(a, "is_complex") else np.iscomplexobj(a)


def _numeric(name, a):
    """Refuses what is neither a real nor a complex floating-point or integer array (bool, object, strings)."""
    import torch

    if isinstance(a, torch.Tensor):
        ok = a.dtype != torch.bool
    else:
        ok = np.asarray(a).dtype.kind in "iufc"
    if not ok:
        raise ValueError(f"{name}: a real or complex numeric array (got dtype {getattr(a, 'dtype', type(a))})")


def _cfft2(name, z, inverse):
    import torch

    B, H, W, ndim = _shape(name, z)
    _numeric(name, z)
    x, as_np = _wave(z, _device(z), False)
    lib = _lib.load()
    out = torch.empty_like(x)
    nbytes = lib.emd_cfft2_any_workspace_bytes(B, H, W)
    ws = _ws(nbytes, x.device)
    _lib.check(lib.emd_cfft2_any_f64(_p(x), 0, B, H, W, int(inverse), _p(out), _p(ws), nbytes, _lib.stream_ptr()), "emd_cfft2_any_f64")
    return _ret(out, ndim, as_np)


def fft2(z):
    """``numpy.fft.fft2`` over the last two axes of ``[B,H,W]`` (or ``[H,W]``), complex128; real input is cast."""
    return _cfft2("fft2", z, False)


def ifft2(z):
    """``numpy.fft.ifft2`` (normalised by 1 / (H W)), by conjugation around the forward transform."""
    return _cfft2("ifft2", z, True)


def rfft2(x):
    """``numpy.fft.rfft2`` of real ``[B,H,W]`` (or ``[H,W]``) images, which are cast to float32: complex128 ``[B,H,W//2+1]``.  Every
    row is transformed as a complex line: twice the row work of ``harvest.rfft2``, which packs two real rows into one."""
    import torch

    B, H, W, ndim = _shape("rfft2", x)
    _numeric("rfft2", x)
    if _is_complex(x):
        raise ValueError("rfft2: the images are real (float32)")
    device = _device(x)
    is_np = not isinstance(x, torch.Tensor)
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)) if is_np else x
    t = t.to(device=device, dtype=torch.float32).reshape(B, H, W).contiguous()
    lib = _lib.load()
    out = torch.empty((B, H, W // 2 + 1), dtype=torch.complex128, device=device)
    nbytes = lib.emd_rfft2_any_workspace_bytes(B, H, W)
    ws = _ws(nbytes, device)
    _lib.check(lib.emd_rfft2_any_f64(_p(t), B, H, W, _p(out), _p(ws), nbytes, _lib.stream_ptr()), "emd_rfft2_any_f64")
    return _ret(out, ndim, is_np)


def propagate(psi, defocus, wavelength, px=1.0, cs=0.0):
    """``ifft2(fft2(psi) * Hf(defocus_b))`` of every wave of ``[B,H,W]`` (complex128, or real: a float32 image), complex128, with
    ``Hf = exp(i pi (lam df q^2 + 0.5 lam^3 Cs q^4))``, ``q^2 = qx^2 + qy^2``, ``qx = fftfreq(W, px)``, ``qy = fftfreq(H, px)``: the
    periodic boundary of the image itself, no padding.  ``defocus``: one number, or one per wave.  Three launches after the tables'."""
    import torch

    B, H, W, ndim = _shape("propagate", psi)
    _numeric("propagate", psi)
    _positive("propagate", wavelength=wavelength, px=px)
    if not np.isfinite(cs):
        raise ValueError(f"propagate: cs must be finite (got {cs!r})")
    device = _device(psi)
    d = _defocus("propagate", defocus, B, device)
    x, as_np = _wave(psi, device, True)
    lib = _lib.load()
    out = torch.empty((B, H, W), dtype=torch.complex128, device=device)
    nbytes = lib.emd_propagate_any_workspace_bytes(B, H, W)
    ws = _ws(nbytes, device)
    _lib.check(lib.emd_propagate_any_f64(_p(x), int(x.dtype == torch.float32), B, H, W, _p(d), float(wavelength), float(px), float(cs),
                                         _p(out), _p(ws), nbytes, _lib.stream_ptr()), "emd_propagate_any_f64")
    return _ret(out, ndim, as_np)
