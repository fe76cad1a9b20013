"""Exit-wave reconstruction from a through-focus series on the device (csrc/exitwave.hip): the reference's
``ewrec.py`` / ``ewrec_class.py``.  Every image is propagated with a Fresnel transfer function between two 2-D FFTs, the results are
averaged into an exit wave, the exit wave is propagated back to every focus, the measured amplitudes are restored, and so on.  The
reference runs it on ArrayFire (and does not run as committed); here the formulas of include/emdenoise.h are the specification.

Everything is double precision (complex128).  Images are square, of side s; the padded side ``S = s * (1 + pad_periods)`` is a power
of two, 8..4096.  numpy in -> numpy out; torch CUDA tensor in -> device tensor out, on the current stream, with no host
synchronisation; arguments are checked on the shape before anything moves to the device.  A defocus argument that is a float64 CUDA
tensor is used where it is: such calls can be captured in a ``torch.cuda.graph`` and replayed after the tensor is overwritten.
Anything else (a number, a list, a numpy array) is uploaded before the call, which a capture does not allow.

Deviations from the reference: ``px`` (the pixel size) replaces its ``px_dim = 1 + pad_periods`` in the transfer function; where
``|b_k| = 0`` the modulus constraint gives ``a_k`` (the reference: NaN); with ``from_intensity`` the amplitude is
``sqrt(max(image_k, 0))`` and ``psi_k`` starts as that amplitude, not as the image; with ``cs != 0`` the back-propagation multiplies
by ``H(-df)`` as the reference does, which is not ``conj H(df)`` (the Cs term keeps its sign; at ``cs == 0`` the two are equal bit
for bit); ``aperture_mask``, TIFF reading, a gradient-based refinement of the positions and the display
helpers are not here; ``refine_params`` is a compass search, since the reference's ``minimize`` call cannot run.  ``resize_stack`` (``cv2.resize`` of the crops) is ``emdenoise.resample.resize``.

Registration (csrc/register.hip) is what the reference's ``EWREC.__init__`` does before it reconstructs:
``phase_correlate`` / ``rel_pos_estimate`` (``cv2.phaseCorrelate`` restated in include/emdenoise.h; OpenCV is not run), the cropping
centres, ``crop_stack`` (a bilinear sub-pixel crop), and ``align`` / ``reconstruct_series`` that chain them on the device.  Deviations:
``R = P / |P|`` is 0 where ``|P| = 0`` (OpenCV adds an epsilon); images of zeros give shift (0, 0) and response 0 (cv2: NaN); the
centres are ``S/2 + pos - mean(pos)`` (the reference's loop does not run and its sign moves the crop against the drift); the crop is
bilinear (the reference weights the wrong tap and returns the integer crop).

Refinement is the constructor's ``param_refinement=True``: ``crop_candidates`` and ``reconstruct_candidate_stacks``
(candidates that have their own images), ``refine_params`` (the compass search over crop centres and defocuses, decided on the
device) and ``refine_series`` (align, refine, crop, reconstruct)."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np

from . import _lib
from .metrics import _p, _ws

MIN_SIDE, MAX_SIDE, MAX_IMAGES = 8, 4096, 64
FROM_INTENSITY = 1               # EMD_EXITWAVE_FROM_INTENSITY
COMPOSED_KNOB = "exitwave_composed"   # include/emdenoise_dev.h: the composed path at pad_periods == 0, for measurements and tests
PC_WINDOW, PC_CHAIN = 1, 2       # EMD_PC_WINDOW, EMD_PC_CHAIN
MAX_PAIRS, MAX_CROPS = 64, 65535
MAX_CANDIDATES, MAX_ROUNDS = 64, 1024   # emd_exitwave_candidates_f64, emd_exitwave_search_f64
SEARCH_SECTION, SEARCH_PLATEAU = 0, 1   # EMD_SEARCH_SECTION, EMD_SEARCH_PLATEAU
SEARCH_NONFINITE, SEARCH_UNFINISHED = 1, 2   # the status bits: a non-finite loss met; the plateau search never stopped
CANDIDATES_WORKSPACE_CAP = 4 << 30      # bytes: reconstruct_candidates runs chunks of candidates above it
BATCHED_SWEEP_MAX_SIDE = 1024           # defocus_sweep: one candidate-batched call up to this padded side (measured no slower up to
                                        # it, profiles/exitwave_search_bench.json; not measured above), the sequential loop above it


def _padded_side(name, s, pad_periods=0):
    """S = s (1 + pad_periods), checked."""
    if int(pad_periods) != pad_periods or pad_periods < 0:
        raise ValueError(f"{name}: pad_periods must be a non-negative integer (got {pad_periods!r})")
    if int(s) != s or s < 1:
        raise ValueError(f"{name}: the side must be a positive integer (got {s!r})")
    S = int(s) * (1 + int(pad_periods))
    if not MIN_SIDE <= S <= MAX_SIDE or S & (S - 1):
        raise ValueError(f"{name}: the padded side s (1 + pad_periods) must be a power of two, {MIN_SIDE}..{MAX_SIDE} "
                         f"(got {s} x {1 + int(pad_periods)} = {S})")
    return S


def _shape3(name, a):
    """(B, s, ndim) of a [B,s,s] or [s,s] argument, before anything is moved to the device."""
    shp = tuple(a.shape) if hasattr(a, "shape") else np.shape(a)
    if len(shp) == 2:
        shp = (1,) + shp
    if len(shp) != 3:
        raise ValueError(f"{name}: [B,s,s] or [s,s] (got a shape of {len(shp)} dimensions)")
    if shp[1] != shp[2]:
        raise ValueError(f"{name}: square images, the padded side a power of two (got {shp[1]} x {shp[2]})")
    return int(shp[0]), int(shp[1])


def _positive(name, **kw):
    for k, v in kw.items():
        if not (np.isfinite(v) and v > 0):
            raise ValueError(f"{name}: {k} must be positive and finite (got {v!r})")


def _device(a):
    import torch

    return a.device if isinstance(a, torch.Tensor) and a.is_cuda else torch.device("cuda", torch.cuda.current_device())


def _wave(a, device, real_ok):
    """-> (contiguous CUDA tensor [B,s,s], complex128 -- or float32 where real_ok and a is real --, was_numpy)."""
    import torch

    is_np = not isinstance(a, torch.Tensor)
    t = torch.from_numpy(np.ascontiguousarray(a)) if is_np else a
    if t.dim() == 2:
        t = t.reshape(1, *t.shape)
    if not t.is_cuda:
        t = t.to(device)
    if t.is_complex() or not real_ok:
        t = t.to(torch.complex128)
    else:
        t = t.to(torch.float32)
    return t.contiguous(), is_np


def _defocus(name, defocus, B, device):
    """-> float64 CUDA tensor [B].  A float64 CUDA tensor of B entries is used where it is."""
    import torch

    if isinstance(defocus, torch.Tensor) and defocus.is_cuda:
        if defocus.dtype != torch.float64 or defocus.numel() != B or not defocus.is_contiguous():
            raise ValueError(f"{name}: a device defocus must be a contiguous float64 tensor of {B} entries")
        return defocus.reshape(B)
    d = np.asarray(defocus.cpu() if isinstance(defocus, torch.Tensor) else defocus, np.float64)
    if d.ndim == 0:
        d = np.full(B, float(d))
    if d.shape != (B,):
        raise ValueError(f"{name}: one defocus, or one per image ({B}); got a shape of {d.shape}")
    if not np.isfinite(d).all():
        raise ValueError(f"{name}: the defocuses must be finite")
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f"{name}: the defocuses are not on the device; pass a float64 CUDA tensor when capturing")
    return torch.from_numpy(np.ascontiguousarray(d)).to(device)


def _ret(t, ndim, as_np):
    if ndim == 2:
        t = t.reshape(t.shape[-2], t.shape[-1])
    return t.cpu().numpy() if as_np else t


def transfer_function(S, wavelength, defocus, px=1.0, cs=0.0):
    """The Fresnel transfer function ``H = exp(i pi (lam df q^2 + 0.5 lam^3 Cs q^4))`` on the S x S grid of ``numpy.fft.fftfreq(S, px)``
    (FFT order), complex128 ``[S,S]``; a sequence of N defocuses gives ``[N,S,S]``.  The phase is evaluated as include/emdenoise.h
    writes it, operation by operation, and goes through ``sincospi``.  numpy out, unless ``defocus`` is a CUDA tensor."""
    import torch

    S = _padded_side("transfer_function", S)
    _positive("transfer_function", wavelength=wavelength, px=px)
    as_np = not (isinstance(defocus, torch.Tensor) and defocus.is_cuda)
    scalar = (defocus.dim() if isinstance(defocus, torch.Tensor) else np.ndim(defocus)) == 0
    n = 1 if scalar else len(defocus)
    if not 1 <= n <= 65535:
        raise ValueError(f"transfer_function: 1..65535 defocuses (got {n})")
    device = _device(defocus)
    d = _defocus("transfer_function", defocus, n, device)
    H = torch.empty((n, S, S), dtype=torch.complex128, device=device)
    _lib.check(_lib.load().emd_transfer_function_f64(S, n, _p(d), float(wavelength), float(px), float(cs), _p(H), _lib.stream_ptr()),
               "emd_transfer_function_f64")
    return _ret(H, 2 if scalar else 3, as_np)


def _cfft2(name, z, inverse):
    import torch

    B, S = _shape3(name, z)
    _padded_side(name, S)
    ndim = len(np.shape(z)) if not hasattr(z, "dim") else z.dim()
    x, as_np = _wave(z, _device(z), False)
    lib = _lib.load()
    out = torch.empty_like(x)
    nbytes = lib.emd_cfft2_workspace_bytes(B, S)
    ws = _ws(nbytes, x.device)
    _lib.check(lib.emd_cfft2_f64(_p(x), B, S, int(inverse), _p(out), _p(ws), nbytes, _lib.stream_ptr()), "emd_cfft2_f64")
    return _ret(out, ndim, as_np)


def fft2(z):
    """``numpy.fft.fft2`` over the last two axes of ``[B,S,S]`` (or ``[S,S]``), complex128; real input is cast."""
    return _cfft2("fft2", z, False)


def ifft2(z):
    """``numpy.fft.ifft2`` (normalised by 1 / S^2), by conjugation around the forward transform."""
    return _cfft2("ifft2", z, True)


def propagate(psi, defocus, wavelength, px=1.0, cs=0.0, pad_periods=0):
    """``ifft2(fft2(zero-pad psi to S x S, image at the top-left) * H(defocus_b))[:s, :s]`` of every wave of ``[B,s,s]`` (complex128, or
    float32: a real image), complex128.  ``defocus``: one number, or one per wave.  Three launches after the twiddle table."""
    import torch

    B, s = _shape3("propagate", psi)
    _padded_side("propagate", s, pad_periods)
    _positive("propagate", wavelength=wavelength, px=px)
    ndim = len(np.shape(psi)) if not hasattr(psi, "dim") else psi.dim()
    device = _device(psi)
    d = _defocus("propagate", defocus, B, device)
    x, as_np = _wave(psi, device, True)
    lib = _lib.load()
    out = torch.empty((B, s, s), dtype=torch.complex128, device=device)
    nbytes = lib.emd_propagate_workspace_bytes(B, s, int(pad_periods))
    ws = _ws(nbytes, device)
    _lib.check(lib.emd_propagate_f64(_p(x), int(x.dtype == torch.float32), B, s, int(pad_periods), _p(d), float(wavelength), float(px),
                                     float(cs), _p(out), _p(ws), nbytes, _lib.stream_ptr()), "emd_propagate_f64")
    return _ret(out, ndim, as_np)


def _reconstruct(name, images, defocuses, wavelength, kw, want_stack, want_losses):
    """-> (E [s,s], stack [N,s,s] or None, losses [N] or None) on the device, and was_numpy.  ``kw``: the keywords of ``_recon_kw``."""
    import torch

    args, composed = _recon_kw(name, kw)
    N, s = _images(name, images, args["pad_periods"])
    _positive(name, wavelength=wavelength)
    device = _device(images)
    d = _defocus(name, defocuses, N, device)
    x, as_np = _wave(images, device, True)
    lib = _lib.load()
    E = torch.empty((s, s), dtype=torch.complex128, device=device)
    stack = torch.empty((N, s, s), dtype=torch.complex128, device=device) if want_stack else None
    losses = torch.empty((N,), dtype=torch.float64, device=device) if want_losses else None
    with _composed_knob(composed):   # read by the size query and by the call (host side, at launch time)
        nbytes = lib.emd_exitwave_workspace_bytes(N, s, int(args["pad_periods"]))
        ws = _ws(nbytes, device)
        rc = lib.emd_exitwave_reconstruct_f64(_p(x), N, s, int(args["pad_periods"]), _p(d), float(wavelength), float(args["px"]),
                                              float(args["cs"]), int(args["iterations"]), FROM_INTENSITY if args["from_intensity"] else 0,
                                              _p(E), _p(stack), _p(losses), _p(ws), nbytes, _lib.stream_ptr())
    _lib.check(rc, "emd_exitwave_reconstruct_f64")
    return (E, stack, losses), as_np


def reconstruct(images, defocuses, wavelength, px=1.0, cs=0.0, iterations=50, pad_periods=0, from_intensity=False, return_stack=False,
                return_losses=False, _composed=False):
    """The exit wave of a focal series ``images`` ``[N,s,s]`` float32 (1 <= N <= 64) taken at ``defocuses``.  The amplitudes are
    ``|image_k|`` and ``psi_k`` starts as the image (``from_intensity``: ``sqrt(max(image_k, 0))``, and ``psi_k`` starts as that); every iteration
    ``E = mean_k P(psi_k, -df_k)``, ``b_k = P(E, +df_k)``, ``psi_k = a_k b_k / |b_k|``.  Returns E of the last iteration, complex128
    ``[s,s]``; with ``return_stack`` / ``return_losses`` a tuple that also holds the last psi ``[N,s,s]`` and the losses ``[N]`` (see
    ``reconstruction_loss``).  With ``pad_periods == 0`` an iteration is two launches for the whole stack (the iteration restated in
    the frequency domain); ``_composed`` (the library's development knob ``exitwave_composed``, for measurements and tests) runs it
    through the launches of ``propagate`` instead, as ``pad_periods > 0`` does."""
    kw = {"px": px, "cs": cs, "iterations": iterations, "pad_periods": pad_periods, "from_intensity": from_intensity, "_composed": _composed}
    outs, as_np = _reconstruct("reconstruct", images, defocuses, wavelength, kw, return_stack, return_losses)
    outs = [o.cpu().numpy() if as_np else o for o in outs if o is not None]
    return outs[0] if len(outs) == 1 else tuple(outs)


def reconstruction_loss(images, defocuses, wavelength, per_image=False, **kw):
    """``reconstruction_loss`` (ewrec_class.py:364-380): with E the reconstruction, ``I = |P(E, df_k)|^2`` and
    ``c = mean(image_k) / mean(I)``, ``loss_k = mean((image_k - c I)^2)`` (two-pass, in double); the largest over the images, as the
    reference returns it, or all of them (``per_image``: ``[N]``).  Keywords: ``px``, ``cs``, ``iterations``, ``pad_periods``,
    ``from_intensity``, as ``reconstruct`` has them."""
    (_, _, losses), as_np = _reconstruct("reconstruction_loss", images, defocuses, wavelength, kw, False, True)
    if not per_image:
        losses = losses.max()
    return (losses.cpu().numpy() if per_image else float(losses)) if as_np else losses


def focal_ramp(n, series_type="cubic", middle=None, alternating=True, increasing=True):
    """The relative defocuses of a series of n images (ewrec_class.py:387-404): ``dir * sign(x - mid) * gen(x - mid)``, gen the
    identity ("linear"), the square ("quadratic") or the cube ("cubic"); mid = ``middle`` or n // 2 when ``alternating``, else 0.
    float64 ``[n]``, on the host."""
    gens = {"linear": lambda x: x, "quadratic": lambda x: x ** 2, "cubic": lambda x: x ** 3}
    if series_type not in gens:
        raise ValueError(f"focal_ramp: series_type is one of {sorted(gens)} (got {series_type!r})")
    if int(n) != n or n < 1:
        raise ValueError(f"focal_ramp: n must be a positive integer (got {n!r})")
    mid = (middle if middle else int(n) // 2) if alternating else 0
    direction = 1.0 if increasing else -1.0
    x = np.arange(int(n), dtype=np.float64) - mid
    return direction * np.sign(x) * gens[series_type](x)


def defocus_sweep(images, wavelength, increments, ramp, **kw):
    """``reconstruction_loss`` for every increment, the defocuses being ``increment * ramp``: float64 ``[len(increments)]``.  The
    defocuses of all increments are uploaded once, the reconstructions run as one candidate-batched call (``reconstruct_candidates``;
    the same bits) up to a padded side of ``BATCHED_SWEEP_MAX_SIDE``, above it one after the other, and the losses are read back
    once at the end (numpy out for numpy images, else a device tensor).  Keywords: ``px``, ``cs``, ``iterations``,
    ``pad_periods``, ``from_intensity``; always the largest loss over the images, so ``per_image`` is refused."""
    import torch

    kw = dict(kw)
    sequential = kw.pop("_sequential", None)
    unknown = sorted(set(kw) - {"px", "cs", "iterations", "pad_periods", "from_intensity", "_composed"})
    if unknown:
        raise TypeError(f"defocus_sweep: unexpected keyword(s) {unknown}")

    inc = np.asarray(increments, np.float64).reshape(-1)
    ramp = np.asarray(ramp, np.float64).reshape(-1)
    shp = tuple(images.shape) if hasattr(images, "shape") else np.shape(images)
    if len(shp) != 3 or ramp.shape[0] != shp[0]:
        raise ValueError(f"defocus_sweep: images are [N,s,s] and the ramp has N entries (got {shp} and {ramp.shape[0]})")
    if inc.size < 1 or not np.isfinite(inc).all() or not np.isfinite(ramp).all():
        raise ValueError("defocus_sweep: at least one increment; increments and ramp finite")
    _padded_side("defocus_sweep", shp[1], kw.get("pad_periods", 0))
    device = _device(images)
    x, as_np = _wave(images, device, True)
    table = torch.from_numpy(inc[:, None] * ramp[None, :]).to(device)
    S = shp[1] * (1 + int(kw.get("pad_periods", 0)))
    if sequential is None:   # one candidate-batched call where that was measured to be no slower (tools/exitwave_search_bench.py)
        sequential = S > BATCHED_SWEEP_MAX_SIDE or inc.size * ramp.shape[0] > 65535
    if sequential:
        out = torch.stack([reconstruction_loss(x, table[i], wavelength, **kw) for i in range(inc.size)])
    else:
        out = reconstruct_candidates(x, table, wavelength, **kw)
    return out.cpu().numpy() if as_np else out


def _recon_kw(name, kw):
    """The reconstruction's keywords with their defaults; anything else is refused."""
    kw = dict(kw)
    composed = bool(kw.pop("_composed", False))
    args = {"px": 1.0, "cs": 0.0, "iterations": 50, "pad_periods": 0, "from_intensity": False}
    unknown = sorted(set(kw) - set(args))
    if unknown:
        raise TypeError(f"{name}: unexpected keyword(s) {unknown}; it takes {sorted(args)}")
    args.update(kw)
    _positive(name, px=args["px"])
    if int(args["iterations"]) != args["iterations"] or args["iterations"] < 1:
        raise ValueError(f"{name}: iterations must be a positive integer (got {args['iterations']!r})")
    return args, composed


def _images(name, images, pad_periods):
    shp = tuple(images.shape) if hasattr(images, "shape") else np.shape(images)
    if len(shp) != 3 or shp[1] != shp[2]:
        raise ValueError(f"{name}: images are [N,s,s], square (got a shape of {shp})")
    N, s = int(shp[0]), int(shp[1])
    if not 1 <= N <= MAX_IMAGES:
        raise ValueError(f"{name}: 1..{MAX_IMAGES} images (got {N})")
    _padded_side(name, s, pad_periods)
    if hasattr(images, "is_complex") and images.is_complex() or not hasattr(images, "is_complex") and np.iscomplexobj(images):
        raise ValueError(f"{name}: the images are real (float32)")
    return N, s


class _composed_knob:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        if self.on:
            _lib.knob(COMPOSED_KNOB, 1)

    def __exit__(self, *exc):
        if self.on:
            _lib.knob(COMPOSED_KNOB, 0)


def reconstruct_candidates(images, defocus_table, wavelength, px=1.0, cs=0.0, iterations=50, pad_periods=0, from_intensity=False,
                           per_image=False, return_waves=False, return_stack=False, candidates_per_launch=None, _composed=False):
    """One stack ``images`` ``[N,s,s]`` reconstructed under every row of ``defocus_table`` ``[C,N]`` in one call
    (``emd_exitwave_candidates_f64``): the largest loss over the images of every candidate, float64 ``[C]``, or all of
    them (``per_image``: ``[C,N]``); ``return_waves`` adds the exit waves ``[C,s,s]``, ``return_stack`` the last psi ``[C,N,s,s]`` (then
    a tuple).  Every candidate's numbers are bit for bit those of ``reconstruct`` / ``reconstruction_loss`` with its row alone.  A
    float64 CUDA table is used where it is (capturable); anything else is uploaded and must be finite.  When the workspace for all C
    exceeds ``CANDIDATES_WORKSPACE_CAP`` bytes the candidates run in chunks, one call after the other on the stream with no
    synchronisation between them; ``candidates_per_launch`` sets the chunk.  The bits are the same for any chunking."""
    return _candidates("reconstruct_candidates", False, images, defocus_table, wavelength, px, cs, iterations, pad_periods, from_intensity,
                       per_image, return_waves, return_stack, candidates_per_launch, _composed)


def _candidates(name, own_stacks, images, defocus_table, wavelength, px, cs, iterations, pad_periods, from_intensity, per_image,
                return_waves, return_stack, candidates_per_launch, _composed):
    """``reconstruct_candidates`` (images [N,s,s]) and ``reconstruct_candidate_stacks`` (``own_stacks``: [C,N,s,s])."""
    import torch

    tshape = tuple(defocus_table.shape) if hasattr(defocus_table, "shape") else np.shape(defocus_table)
    if own_stacks:
        shp = tuple(images.shape) if hasattr(images, "shape") else np.shape(images)
        if len(shp) != 4 or shp[0] < 1:
            raise ValueError(f"{name}: the stacks are [C,N,s,s], C >= 1 (got a shape of {shp})")
        N, s = _images(name, images[0], pad_periods)
        if len(tshape) != 2 or tshape != (shp[0], N):
            raise ValueError(f"{name}: the defocus table is [C,N] = [{shp[0]},{N}] (got a shape of {tshape})")
    else:
        N, s = _images(name, images, pad_periods)
    _recon_kw(name, {"px": px, "iterations": iterations})
    _positive(name, wavelength=wavelength)
    if len(tshape) != 2 or tshape[1] != N or tshape[0] < 1:
        raise ValueError(f"{name}: the defocus table is [C,N] = [C,{N}], C >= 1 (got a shape of {tshape})")
    Ct = int(tshape[0])
    device = _device(images)
    if isinstance(defocus_table, torch.Tensor) and defocus_table.is_cuda:
        if defocus_table.dtype != torch.float64 or not defocus_table.is_contiguous():
            raise ValueError(f"{name}: a device defocus table must be a contiguous float64 tensor")
        table = defocus_table
    else:
        t = np.ascontiguousarray(defocus_table.cpu() if isinstance(defocus_table, torch.Tensor) else defocus_table, dtype=np.float64)
        if not np.isfinite(t).all():
            raise ValueError(f"{name}: the defocuses must be finite")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{name}: the defocus table is not on the device; pass a float64 CUDA tensor when capturing")
        table = torch.from_numpy(t).to(device)
    lib = _lib.load()
    per = min(Ct, MAX_CANDIDATES, 65535 // N)
    with _composed_knob(_composed):
        if candidates_per_launch is None:
            while per > 1 and lib.emd_exitwave_candidates_workspace_bytes(per, N, s, int(pad_periods)) > CANDIDATES_WORKSPACE_CAP:
                per = (per + 1) // 2
        else:
            if int(candidates_per_launch) != candidates_per_launch or not 1 <= candidates_per_launch <= per:
                raise ValueError(f"{name}: candidates_per_launch must be an integer, 1..{per} (got {candidates_per_launch!r})")
            per = int(candidates_per_launch)
        if own_stacks:
            x, as_np = _real(images, device)
        else:
            x, as_np = _wave(images, device, True)
        losses = torch.empty((Ct, N), dtype=torch.float64, device=device)
        worst = torch.empty((Ct,), dtype=torch.float64, device=device)
        E = torch.empty((Ct, s, s), dtype=torch.complex128, device=device) if return_waves else None
        stack = torch.empty((Ct, N, s, s), dtype=torch.complex128, device=device) if return_stack else None
        nbytes = lib.emd_exitwave_candidates_workspace_bytes(per, N, s, int(pad_periods))
        ws = _ws(nbytes, device)
        flags = FROM_INTENSITY if from_intensity else 0
        entry = "emd_exitwave_candidate_stacks_f64" if own_stacks else "emd_exitwave_candidates_f64"
        for c0 in range(0, Ct, per):
            n = min(per, Ct - c0)
            sub = lambda t: _p(t[c0:c0 + n]) if t is not None else None
            _lib.check(getattr(lib, entry)(sub(x) if own_stacks else _p(x), n, N, s, int(pad_periods), sub(table), float(wavelength),
                                           float(px), float(cs), int(iterations), flags, sub(losses), sub(worst), sub(E), sub(stack), _p(ws),
                                           nbytes, _lib.stream_ptr()), entry)
    outs = [losses if per_image else worst] + [o for o in (E, stack) if o is not None]
    outs = [o.cpu().numpy() if as_np else o for o in outs]
    return outs[0] if len(outs) == 1 else tuple(outs)


def reconstruct_candidate_stacks(stacks, defocus_table, wavelength, px=1.0, cs=0.0, iterations=50, pad_periods=0, from_intensity=False,
                                 per_image=False, return_waves=False, return_stack=False, candidates_per_launch=None, _composed=False):
    """``reconstruct_candidates`` for candidates that have their own images (``emd_exitwave_candidate_stacks_f64``):
    ``stacks`` ``[C,N,s,s]`` float32 under ``defocus_table`` ``[C,N]``.  It returns what ``reconstruct_candidates`` returns, chunks under
    ``CANDIDATES_WORKSPACE_CAP`` in the same way, and every candidate's numbers are bit for bit those of ``reconstruct`` /
    ``reconstruction_loss`` with its stack and its row alone."""
    return _candidates("reconstruct_candidate_stacks", True, stacks, defocus_table, wavelength, px, cs, iterations, pad_periods,
                       from_intensity, per_image, return_waves, return_stack, candidates_per_launch, _composed)


def search_increments(search_range, num):
    """The increments of the reference's initial sweep (ewrec_class.py:406-414): ``c + m 2^x / 2^num`` for x = 0..num-1 with
    ``(c, m) = (search_range[0], search_range[1] - search_range[0])``, a geometric ramp from ``c + m / 2^num`` to ``c + m / 2``.
    Deviation: the reference subtracts 1 from ``2^x / 2^num``, which puts every increment below the range."""
    lo, hi = (float(v) for v in search_range)
    if int(num) != num or num < 1 or not (np.isfinite(lo) and np.isfinite(hi)):
        raise ValueError(f"search_increments: a finite range and a positive integer number (got {search_range!r}, {num!r})")
    x = np.arange(int(num), dtype=np.float64)
    return lo + (hi - lo) * (2.0 ** x / 2.0 ** int(num))


def plateau_seed(increments, losses):
    """(incr1, incr2, prev) for the plateau search from a sweep: i = the first smallest loss; the neighbour is i + 1 at the left end,
    i - 1 at the right end, else the one with the smaller loss (the left one on a tie); incr2 = the increment at i, incr1 = the
    neighbour's, prev = the loss at i."""
    inc, loss = np.asarray(increments, np.float64).reshape(-1), np.asarray(losses, np.float64).reshape(-1)
    if inc.size < 2 or inc.shape != loss.shape or not np.isfinite(loss).all():
        raise ValueError("plateau_seed: at least two increments, as many finite losses")
    i = int(np.argmin(loss))
    j = 1 if i == 0 else i - 1 if i == inc.size - 1 else (i - 1 if loss[i - 1] <= loss[i + 1] else i + 1)
    return float(inc[j]), float(inc[i]), float(loss[i])


class DefocusSearchResult(NamedTuple):
    increment: object          # the result, and its (largest over the images) loss
    loss: object
    defocuses: object          # increment * ramp, [N]
    history_increments: object   # [rounds, candidates] ("plateau": [max_steps]): every candidate that was reconstructed
    history_losses: object
    status: int                # SEARCH_NONFINITE | SEARCH_UNFINISHED
    steps: int
    wave: object               # E at the result with return_wave, else None


def defocus_search(images, wavelength, ramp, bracket=None, method="section", candidates=8, rounds=4, sweep_increments=None, max_steps=16,
                   return_wave=False, **kw):
    """The defocus increment of a focal series whose defocuses are ``increment * ramp``, searched on the device
    (``emd_exitwave_search_f64``; the reference's ``defocus_initial_estimate``, ewrec_class.py:382-434, repaired).

    ``method="section"``: ``rounds`` rounds of ``candidates`` (3..64) equidistant increments over ``bracket`` = (lo, hi), reconstructed
    together; every round narrows the bracket to the neighbours of its best candidate; the result is the best over all rounds.
    ``method="plateau"``: the reference's bisection from the two best neighbours of a sweep over ``sweep_increments`` (run by
    ``defocus_sweep`` and read back), or from ``bracket`` = (incr1, incr2, prev); at most ``max_steps`` reconstructions.

    ``ramp`` ``[N]`` and ``bracket`` may be float64 CUDA tensors, which are used where they are: then the call is launches only, can be
    captured, and reads new contents on replay.  Host values are uploaded, and a non-finite bracket is refused.  Keywords: ``px``,
    ``cs``, ``iterations``, ``pad_periods``, ``from_intensity``.  numpy images: numpy / float fields in the result; CUDA images: device
    tensors, and ``status`` / ``steps`` are read back unless the stream is capturing (then they are device tensors too)."""
    import torch

    name = "defocus_search"
    args, composed = _recon_kw(name, kw)
    N, s = _images(name, images, args["pad_periods"])
    _positive(name, wavelength=wavelength)
    if method not in ("section", "plateau"):
        raise ValueError(f"{name}: method is 'section' or 'plateau' (got {method!r})")
    plateau = method == "plateau"
    C = 1 if plateau else candidates
    R = max_steps if plateau else rounds
    if not plateau and (int(C) != C or not 3 <= C <= MAX_CANDIDATES):
        raise ValueError(f"{name}: 3..{MAX_CANDIDATES} candidates (got {C!r})")
    if int(R) != R or not 1 <= R <= MAX_ROUNDS:
        raise ValueError(f"{name}: 1..{MAX_ROUNDS} rounds or steps (got {R!r})")
    if C * N > 65535:
        raise ValueError(f"{name}: candidates x images <= 65535 (got {C} x {N})")

    def checked(what, v, n):   # on the host, before anything moves
        if isinstance(v, torch.Tensor) and v.is_cuda:
            if v.dtype != torch.float64 or v.numel() != n or not v.is_contiguous():
                raise ValueError(f"{name}: a device {what} must be a contiguous float64 tensor of {n} entries")
            return v
        a = np.asarray(v, np.float64).reshape(-1)
        if a.shape != (n,) or not np.isfinite(a).all():
            raise ValueError(f"{name}: the {what} has {n} finite entries (got {a!r})")
        return np.ascontiguousarray(a)

    def on_device(what, v):
        if isinstance(v, torch.Tensor):
            return v
        if capturing:
            raise RuntimeError(f"{name}: the {what} is not on the device; pass a float64 CUDA tensor when capturing")
        return torch.from_numpy(v).to(device)

    ramp = checked("ramp", ramp, N)
    if bracket is not None:
        bracket = checked("bracket", bracket, 3 if plateau else 2)
    elif not plateau:
        raise ValueError(f"{name}: the section search needs bracket = (lo, hi)")
    elif sweep_increments is None:
        raise ValueError(f"{name}: the plateau search starts from sweep_increments, or from bracket = (incr1, incr2, prev)")
    device = _device(images)
    x, as_np = _wave(images, device, True)
    capturing = torch.cuda.is_current_stream_capturing()
    if bracket is None:
        host_ramp = np.asarray(ramp.cpu() if isinstance(ramp, torch.Tensor) else ramp, np.float64).reshape(-1)
        sweep = defocus_sweep(x, wavelength, sweep_increments, host_ramp, _composed=composed, **args)
        bracket = np.array(plateau_seed(sweep_increments, sweep.cpu().numpy()), np.float64)
    r = on_device("ramp", ramp)
    seed = on_device("bracket", bracket)
    lib = _lib.load()
    result = torch.empty((2,), dtype=torch.float64, device=device)
    hist_inc = torch.empty((int(R), int(C)), dtype=torch.float64, device=device)
    hist_loss = torch.empty((int(R), int(C)), dtype=torch.float64, device=device)
    status = torch.empty((2,), dtype=torch.int32, device=device)
    E = torch.empty((s, s), dtype=torch.complex128, device=device) if return_wave else None
    m = SEARCH_PLATEAU if plateau else SEARCH_SECTION
    with _composed_knob(composed):
        nbytes = lib.emd_exitwave_search_workspace_bytes(m, int(C), N, s, int(args["pad_periods"]))
        ws = _ws(nbytes, device)
        rc = lib.emd_exitwave_search_f64(_p(x), N, s, int(args["pad_periods"]), _p(r), _p(seed), m, int(C), int(R), float(wavelength),
                                         float(args["px"]), float(args["cs"]), int(args["iterations"]),
                                         FROM_INTENSITY if args["from_intensity"] else 0, _p(result), _p(hist_inc), _p(hist_loss),
                                         _p(status), _p(E), _p(ws), nbytes, _lib.stream_ptr())
    _lib.check(rc, "emd_exitwave_search_f64")
    if plateau:
        hist_inc, hist_loss = hist_inc.reshape(-1), hist_loss.reshape(-1)
    defocuses = result[0] * r
    if capturing:
        return DefocusSearchResult(result[0], result[1], defocuses, hist_inc, hist_loss, status[0], status[1], E)
    st = status.cpu().numpy()
    if as_np:
        res = result.cpu().numpy()
        return DefocusSearchResult(float(res[0]), float(res[1]), defocuses.cpu().numpy(), hist_inc.cpu().numpy(), hist_loss.cpu().numpy(),
                                   int(st[0]), int(st[1]), None if E is None else E.cpu().numpy())
    return DefocusSearchResult(result[0], result[1], defocuses, hist_inc, hist_loss, int(st[0]), int(st[1]), E)


def estimate_defocuses(stack, wavelength, series_type="cubic", middle=None, alternating=True, increasing=True, search_range=(0.0, 1e-7),
                       sweep_num=8, max_steps=16, return_wave=False, **kw):
    """``EWREC.defocus_initial_estimate`` (ewrec_class.py:382-434): ``focal_ramp`` of the series, a sweep over
    ``search_increments(search_range, sweep_num)``, then the plateau search from its two best neighbours.  A ``DefocusSearchResult``;
    its ``defocuses`` are the estimate."""
    shp = tuple(stack.shape) if hasattr(stack, "shape") else np.shape(stack)
    if len(shp) != 3:
        raise ValueError(f"estimate_defocuses: the stack is [N,s,s] (got a shape of {shp})")
    ramp = focal_ramp(shp[0], series_type, middle, alternating, increasing)
    return defocus_search(stack, wavelength, ramp, method="plateau", sweep_increments=search_increments(search_range, sweep_num),
                          max_steps=max_steps, return_wave=return_wave, **kw)


# ---- registration and cropping (csrc/register.hip) -----------------------------------------------------------------

def _stack(name, a, min_images=1, max_images=MAX_CROPS, power_of_two=True):
    """(N, S) of an [N,S,S] argument, checked before anything moves."""
    import torch

    shp = tuple(a.shape) if hasattr(a, "shape") else np.shape(a)
    if len(shp) != 3 or shp[1] != shp[2]:
        raise ValueError(f"{name}: images are [N,S,S], square (got a shape of {shp})")
    N, S = int(shp[0]), int(shp[1])
    if not min_images <= N <= max_images:
        raise ValueError(f"{name}: {min_images}..{max_images} images (got {N})")
    if power_of_two:
        _padded_side(name, S)
    elif not 1 <= S <= MAX_SIDE:
        raise ValueError(f"{name}: the side of the images must be 1..{MAX_SIDE} (got {S})")
    if isinstance(a, torch.Tensor) and a.is_complex() or not isinstance(a, torch.Tensor) and np.iscomplexobj(a):
        raise ValueError(f"{name}: the images are real (float32)")
    return N, S


def _real(a, device):
    """-> (contiguous float32 CUDA tensor, was_numpy)."""
    import torch

    is_np = not isinstance(a, torch.Tensor)
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)) if is_np else a
    return t.to(device=device, dtype=torch.float32).contiguous(), is_np


def hanning_window(S, one_d=False):
    """``cv2.createHanningWindow((S, S), CV_64F)``: ``sqrt(w[y] w[x])`` with ``w[i] = 0.5 (1 - cos(2 pi i / (S - 1)))``, float64
    ``[S,S]`` on the host -- the bits that ``phase_correlate(window=True)`` multiplies the images by, computed by the same device
    function.  ``one_d``: the table ``w`` ``[S]`` instead."""
    import torch

    S = _padded_side("hanning_window", S)
    device = torch.device("cuda", torch.cuda.current_device())
    w = torch.empty((S,) if one_d else (S, S), dtype=torch.float64, device=device)
    _lib.check(_lib.load().emd_hanning_window_f64(S, _p(w if one_d else None), _p(None if one_d else w), _lib.stream_ptr()),
               "emd_hanning_window_f64")
    return w.cpu().numpy()


def _correlate(name, a, b, P, S, flags, want_surface):
    """-> (shifts [P,3], surface [P,S,S] or None) on the device of ``a`` (a contiguous float32 CUDA tensor, as ``b`` or None)."""
    import torch

    lib = _lib.load()
    shifts = torch.empty((P, 3), dtype=torch.float64, device=a.device)
    surface = torch.empty((P, S, S), dtype=torch.float64, device=a.device) if want_surface else None
    nbytes = lib.emd_phase_correlate_workspace_bytes(P, S, flags)
    ws = _ws(nbytes, a.device)
    _lib.check(lib.emd_phase_correlate_f64(_p(a), _p(b), P, S, flags, _p(shifts), _p(surface), _p(ws), nbytes, _lib.stream_ptr()), name)
    return shifts, surface


def phase_correlate(a, b, window=False, return_response=False, return_surface=False):
    """``cv2.phaseCorrelate(a, b[, hanning window])`` of every pair of ``a``, ``b`` ``[B,S,S]`` (1 <= B <= 64; or ``[S,S]``: one pair),
    float32, S a power of two, 8..4096, as include/emdenoise.h restates it: float64 ``[B,2]`` = (dx, dy) (``[2]`` for one ``[S,S]`` pair);
    if b is a displaced by +d the shift is +d; a and b may be the same tensor (an autocorrelation) or overlapping views.  ``return_response`` adds the responses ``[B]`` (the sum of the 5 x 5 window around the
    peak), ``return_surface`` the correlation surfaces ``[B,S,S]`` in ``fftshift`` order; then a tuple is returned."""
    B, S = _shape3("phase_correlate", a)
    if _shape3("phase_correlate", b) != (B, S):
        raise ValueError(f"phase_correlate: a and b must have the same shape (got {tuple(np.shape(a))} and {tuple(np.shape(b))})")
    _padded_side("phase_correlate", S)
    if not 1 <= B <= MAX_PAIRS:
        raise ValueError(f"phase_correlate: 1..{MAX_PAIRS} pairs (got {B})")
    ndim = len(np.shape(a)) if not hasattr(a, "dim") else a.dim()
    device = _device(a)
    x, as_np = _real(a, device)
    y, _ = _real(b, device)
    shifts, surface = _correlate("emd_phase_correlate_f64", x.reshape(B, S, S), y.reshape(B, S, S), B, S, PC_WINDOW if window else 0,
                                 return_surface)
    outs = [shifts[:, :2]] + ([shifts[:, 2]] if return_response else []) + ([surface] if return_surface else [])
    if ndim == 2:
        outs = [o[0] for o in outs]
    outs = [o.cpu().numpy() if as_np else o for o in outs]
    return outs[0] if len(outs) == 1 else tuple(outs)


def _stack_centres(shifts, N, S):
    import torch

    centres = torch.empty((N, 2), dtype=torch.float64, device=shifts.device)
    _lib.check(_lib.load().emd_stack_centres_f64(_p(shifts), N, S, _p(centres), _lib.stream_ptr()), "emd_stack_centres_f64")
    return centres


def rel_pos_estimate(stack, window=False, as_cropping_centres=True):
    """``rel_pos_estimate`` (ewrec_class.py:240-269): the shifts between consecutive images of ``stack`` ``[N,S,S]`` (2 <= N <= 65) by
    phase correlation, every image transformed once; float64 ``[N-1,2]`` = (dx, dy) of the pairs (k, k+1), or, with
    ``as_cropping_centres``, ``[N,2]`` = (x, y): ``S/2 + pos_k - mean(pos)`` with ``pos_0 = 0``, ``pos_k = pos_{k-1} + shift_{k-1}``."""
    N, S = _stack("rel_pos_estimate", stack, 2, MAX_PAIRS + 1)
    x, as_np = _real(stack, _device(stack))
    shifts, _ = _correlate("emd_phase_correlate_f64", x, None, N - 1, S, PC_CHAIN | (PC_WINDOW if window else 0), False)
    out = _stack_centres(shifts, N, S) if as_cropping_centres else shifts[:, :2]
    return out.cpu().numpy() if as_np else out


def largest_crop_side(centres, S, power_of_two=True):
    """The largest side a crop around every one of ``centres`` ``[N,2]`` can have inside images of side S (ewrec_class.py:193-200, with
    ``min`` where the reference has a comparison that never fires): ``int(2 min(x, y, S - x, S - y))`` over all centres, floored to a
    power of two unless ``power_of_two`` is false.  On the host (a device tensor is read back)."""
    c = np.asarray(centres.detach().cpu() if hasattr(centres, "detach") else centres, np.float64)
    if c.ndim != 2 or c.shape[1] != 2 or c.shape[0] < 1 or not np.isfinite(c).all():
        raise ValueError(f"largest_crop_side: centres are [N,2], finite (got a shape of {c.shape})")
    side = int(2.0 * min(c.min(), (float(S) - c).min()))
    if side < 1:
        raise ValueError(f"largest_crop_side: a centre lies outside the images (side {S})")
    return 1 << (side.bit_length() - 1) if power_of_two else side


def _crop(x, centres, side, pad_val):
    import torch

    N, S = int(x.shape[0]), int(x.shape[1])
    out = torch.empty((N, side, side), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().emd_crop_stack_f32(_p(x), N, S, _p(centres), side, float(pad_val), _p(out), _lib.stream_ptr()),
               "emd_crop_stack_f32")
    return out


def _side(name, side, S):
    if int(side) != side or not 1 <= side <= S:
        raise ValueError(f"{name}: side must be an integer, 1..{S} (got {side!r})")
    return int(side)


def crop_stack(stack, centres, side, pad_val=0.0):
    """``crop_stack`` (ewrec_class.py:190-229) as a bilinear sub-pixel crop: ``side x side`` pixels around ``centres[k]`` = (x, y) from
    image k of ``stack`` ``[N,S,S]`` float32 (S 1..4096, 1 <= side <= S): float32 ``[N,side,side]``.  The window starts at
    ``centre - side / 2``; a tap outside the image reads ``pad_val``.  ``centres``: ``[N,2]``; a contiguous float64 CUDA tensor is used
    where it is (capturable), anything else is uploaded."""
    import torch

    N, S = _stack("crop_stack", stack, 1, MAX_CROPS, power_of_two=False)
    side = _side("crop_stack", side, S)
    if tuple(centres.shape if hasattr(centres, "shape") else np.shape(centres)) != (N, 2):
        raise ValueError(f"crop_stack: centres are [N,2] = [{N},2]")
    if not np.isfinite(pad_val):
        raise ValueError(f"crop_stack: pad_val must be finite (got {pad_val!r})")
    device = _device(stack)
    if isinstance(centres, torch.Tensor) and centres.is_cuda:
        if centres.dtype != torch.float64 or not centres.is_contiguous():
            raise ValueError("crop_stack: device centres must be a contiguous float64 tensor")
        c = centres
    else:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("crop_stack: the centres are not on the device; pass a float64 CUDA tensor when capturing")
        c = torch.from_numpy(np.ascontiguousarray(centres.cpu() if isinstance(centres, torch.Tensor) else centres, dtype=np.float64)).to(device)
    x, as_np = _real(stack, device)
    out = _crop(x, c, side, pad_val)
    return out.cpu().numpy() if as_np else out


def resize_stack(stack, side, interpolation="linear"):
    """``EWREC.resize_stack`` (ewrec_class.py:236-238): ``cv2.resize(img, (side, side))`` of every image of ``stack`` ``[N,H,W]`` float32
    -> ``[N,side,side]``, with cv2's default ``INTER_LINEAR``; a thin call of ``emdenoise.resample.resize``."""
    from . import resample

    if len(np.shape(stack)) != 3:
        raise ValueError(f"resize_stack: a stack [N,H,W] (got shape {tuple(np.shape(stack))})")
    return resample.resize(stack, side, interpolation)


def align(stack, side=None, window=False, pad_val=0.0):
    """Registers ``stack`` ``[N,S,S]`` (2 <= N <= 65) and cuts the aligned crops: ``(crops [N,side,side] float32, centres [N,2]
    float64)``.  With ``side`` given and a CUDA tensor in, it is three C calls on the current stream (correlation in chain mode,
    centres, crop) with no read-back; ``side=None`` reads the centres back for ``largest_crop_side``."""
    N, S = _stack("align", stack, 2, MAX_PAIRS + 1)
    if side is not None:
        side = _side("align", side, S)
    x, as_np = _real(stack, _device(stack))
    shifts, _ = _correlate("emd_phase_correlate_f64", x, None, N - 1, S, PC_CHAIN | (PC_WINDOW if window else 0), False)
    centres = _stack_centres(shifts, N, S)
    if side is None:
        side = largest_crop_side(centres, S)
    crops = _crop(x, centres, side, pad_val)
    return (crops.cpu().numpy(), centres.cpu().numpy()) if as_np else (crops, centres)


def reconstruct_series(stack, defocuses, wavelength, side, window=False, **reconstruct_kw):
    """``align(stack, side, window)``, then ``reconstruct`` of the crops with ``reconstruct_kw``: what ``EWREC.__init__`` does with a
    recorded series.  2 <= N <= 64 images (``reconstruct``'s limit; ``align`` and ``rel_pos_estimate`` alone take 65);
    ``side (1 + pad_periods)`` is a power of two, 8..4096.  With a CUDA stack and float64 CUDA defocuses the whole
    call is launches on the current stream and can be captured in one ``torch.cuda.graph``."""
    N, S = _stack("reconstruct_series", stack, 2, MAX_PAIRS)
    side = _side("reconstruct_series", side, S)
    _padded_side("reconstruct_series", side, reconstruct_kw.get("pad_periods", 0))
    crops, _ = align(stack, side, window)
    return reconstruct(crops, defocuses, wavelength, **reconstruct_kw)


# ---- refinement of the crop centres and the defocuses (csrc/exitwave.hip, csrc/register.hip) ------------------------

def _checked_doubles(name, what, v, shape):
    """On the host, before anything moves: a contiguous float64 CUDA tensor of ``shape`` as it is, anything else as a finite float64
    array of that shape."""
    import torch

    if isinstance(v, torch.Tensor) and v.is_cuda:
        if v.dtype != torch.float64 or tuple(v.shape) != shape or not v.is_contiguous():
            raise ValueError(f"{name}: device {what} must be a contiguous float64 tensor of shape {list(shape)}")
        return v
    a = np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v, np.float64)
    if a.shape != shape or not np.isfinite(a).all():
        raise ValueError(f"{name}: the {what} are {list(shape)}, finite (got a shape of {a.shape})")
    return np.ascontiguousarray(a)


def _uploaded(name, what, v, device):
    """A value ``_checked_doubles`` let through, on the device."""
    import torch

    if isinstance(v, torch.Tensor):
        return v
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f"{name}: the {what} are not on the device; pass a float64 CUDA tensor when capturing")
    return torch.from_numpy(v).to(device)


def crop_candidates(stack, centres_table, side, pad_val=0.0):
    """``crop_stack`` under every one of C sets of centres in one launch (``emd_crop_candidates_f32``): ``stack`` ``[N,S,S]`` float32,
    ``centres_table`` ``[C,N,2]`` -> float32 ``[C,N,side,side]``; ``out[c]`` is bit for bit ``crop_stack(stack, centres_table[c], side)``.
    C N <= 65535.  A contiguous float64 CUDA table is used where it is (capturable), anything else is uploaded."""
    import torch

    name = "crop_candidates"
    N, S = _stack(name, stack, 1, MAX_CROPS, power_of_two=False)
    side = _side(name, side, S)
    tshape = tuple(centres_table.shape if hasattr(centres_table, "shape") else np.shape(centres_table))
    if len(tshape) != 3 or tshape[1:] != (N, 2) or not 1 <= tshape[0] <= MAX_CROPS // N:
        raise ValueError(f"{name}: the centres table is [C,N,2] = [C,{N},2], 1 <= C <= {MAX_CROPS // N} (got a shape of {tshape})")
    if not np.isfinite(pad_val):
        raise ValueError(f"{name}: pad_val must be finite (got {pad_val!r})")
    if isinstance(centres_table, torch.Tensor) and centres_table.is_cuda:
        table = _checked_doubles(name, "centres", centres_table, tshape)
    else:   # as crop_stack: host centres are uploaded as they are (a non-finite centre puts every tap outside)
        table = np.ascontiguousarray(centres_table.cpu() if isinstance(centres_table, torch.Tensor) else centres_table, dtype=np.float64)
    device = _device(stack)
    table = _uploaded(name, "centres", table, device)
    x, as_np = _real(stack, device)
    out = torch.empty((tshape[0], N, side, side), dtype=torch.float32, device=device)
    _lib.check(_lib.load().emd_crop_candidates_f32(_p(x), N, S, _p(table), int(tshape[0]), side, float(pad_val), _p(out), _lib.stream_ptr()),
               "emd_crop_candidates_f32")
    return out.cpu().numpy() if as_np else out


class RefineResult(NamedTuple):
    centres: object            # [N,2] = (x, y) and [N]: the state after the last round
    defocuses: object
    loss: object               # its (largest over the images) loss: the smallest finite one met, the seed's included
    loss0: object              # the seed's
    history_losses: object     # [rounds, 6 (N - 1)]: every poll of every round
    history_choice: object     # [rounds] int32: the poll that was taken, -1 the steps were halved, -2 no poll was finite
    history_steps: object      # [rounds, 2] = (step_xy, step_defocus) the round polled with
    status: int                # SEARCH_NONFINITE
    moves: int
    wave: object               # E at the result with return_exit_wave, else None


def refine_polls(N, anchor):
    """[(axis, k)] of the parameters p = 0..3 (N - 1) - 1 of ``refine_params``: axis 0 = x, 1 = y, 2 = defocus of image k, the images
    in ascending k without the anchor.  Poll q = 2 p adds the axis' step to that entry, q = 2 p + 1 subtracts it."""
    free = [k for k in range(N) if k != anchor]
    return [(axis, k) for axis in range(3) for k in free]


def refine_params(stack, centres, defocuses, wavelength, side, anchor=None, step_xy=1.0, step_defocus=None, rounds=8, candidates=None,
                  pad_val=0.0, return_exit_wave=False, **kw):
    """``EWREC.refine_params`` (ewrec_class.py:436-478, which does not run): the crop centres ``[N,2]`` and the
    defocuses ``[N]`` of a series ``stack`` ``[N,S,S]`` float32 (2 <= N <= 64) refined jointly, on the device
    (``emd_exitwave_refine_f64``), so that the largest per-image ``reconstruction_loss`` of the ``side x side`` crops gets smaller.

    A compass search: every round polls each of the 3 (N - 1) free parameters at plus and minus its step (``step_xy`` pixels for the
    centres, ``step_defocus`` for the defocuses; default 0.1 max|defocuses|), all 6 (N - 1) polls reconstructed as candidates, ``candidates``
    (1..64) at a time -- by default as many as fit ``CANDIDATES_WORKSPACE_CAP`` --, with the same bits whatever that number is.  The
    best poll is taken if it is strictly better than the best so far; otherwise both steps are halved.  Image ``anchor`` (default
    N // 2) keeps its centre and defocus: it is the gauge.  The loss never increases; the true parameters are NOT what it converges to
    (DESIGN.md 3.30).

    ``centres``, ``defocuses`` and ``steps`` = (step_xy, step_defocus) given as one float64 CUDA tensor ``[2]`` in ``step_xy`` (then
    ``step_defocus`` must be None) are used where they are: the call is launches only and can be captured.  Keywords: ``px``, ``cs``,
    ``iterations``, ``pad_periods``, ``from_intensity``.  A ``RefineResult``: numpy / float / int fields for a numpy stack, device
    tensors for a CUDA stack (``status`` and ``moves`` are read back unless the stream is capturing)."""
    import torch

    name = "refine_params"
    args, composed = _recon_kw(name, kw)
    N, S0 = _stack(name, stack, 2, MAX_IMAGES, power_of_two=False)
    side = _side(name, side, S0)
    _padded_side(name, side, args["pad_periods"])
    _positive(name, wavelength=wavelength)
    if anchor is None:
        anchor = N // 2
    if int(anchor) != anchor or not 0 <= anchor < N:
        raise ValueError(f"{name}: anchor must be an integer, 0..{N - 1} (got {anchor!r})")
    if int(rounds) != rounds or not 1 <= rounds <= MAX_ROUNDS:
        raise ValueError(f"{name}: 1..{MAX_ROUNDS} rounds (got {rounds!r})")
    if not np.isfinite(pad_val):
        raise ValueError(f"{name}: pad_val must be finite (got {pad_val!r})")
    Q = 6 * (N - 1)
    if candidates is not None and (int(candidates) != candidates or not 1 <= candidates <= MAX_CANDIDATES):
        raise ValueError(f"{name}: 1..{MAX_CANDIDATES} candidates (got {candidates!r})")
    c0 = _checked_doubles(name, "centres", centres, (N, 2))
    d0 = _checked_doubles(name, "defocuses", defocuses, (N,))
    if isinstance(step_xy, torch.Tensor) and step_xy.is_cuda:
        if step_defocus is not None:
            raise ValueError(f"{name}: device steps are one tensor (step_xy, step_defocus); step_defocus must be None")
        steps = _checked_doubles(name, "steps", step_xy, (2,))
    else:
        if step_defocus is None:
            if isinstance(d0, torch.Tensor):
                raise ValueError(f"{name}: with device defocuses give step_defocus (its default reads them)")
            step_defocus = 0.1 * float(np.abs(d0).max())
        _positive(name, step_xy=step_xy, step_defocus=step_defocus)
        steps = np.array([step_xy, step_defocus], np.float64)
    device = _device(stack)
    c0, d0, steps = (_uploaded(name, what, v, device) for what, v in (("centres", c0), ("defocuses", d0), ("steps", steps)))
    x, as_np = _real(stack, device)
    capturing = torch.cuda.is_current_stream_capturing()
    lib = _lib.load()
    pad, R = int(args["pad_periods"]), int(rounds)
    out_c = torch.empty((N, 2), dtype=torch.float64, device=device)
    out_d = torch.empty((N,), dtype=torch.float64, device=device)
    result = torch.empty((2,), dtype=torch.float64, device=device)
    status = torch.empty((2,), dtype=torch.int32, device=device)
    hist_loss = torch.empty((R, Q), dtype=torch.float64, device=device)
    hist_choice = torch.empty((R,), dtype=torch.int32, device=device)
    hist_steps = torch.empty((R, 2), dtype=torch.float64, device=device)
    E = torch.empty((side, side), dtype=torch.complex128, device=device) if return_exit_wave else None
    with _composed_knob(composed):
        if candidates is None:   # the largest chunk whose workspace fits the cap
            candidates = min(Q, MAX_CANDIDATES)
            while candidates > 1 and lib.emd_exitwave_refine_workspace_bytes(candidates, N, side, pad) > CANDIDATES_WORKSPACE_CAP:
                candidates -= 1
        Cn = int(candidates)
        nbytes = lib.emd_exitwave_refine_workspace_bytes(Cn, N, side, pad)
        ws = _ws(nbytes, device)
        rc = lib.emd_exitwave_refine_f64(_p(x), N, S0, side, pad, float(pad_val), _p(c0), _p(d0), _p(steps), int(anchor), Cn, R,
                                         float(wavelength), float(args["px"]), float(args["cs"]), int(args["iterations"]),
                                         FROM_INTENSITY if args["from_intensity"] else 0, _p(out_c), _p(out_d), _p(result), _p(status),
                                         _p(hist_loss), _p(hist_choice), _p(hist_steps), _p(E), _p(ws), nbytes, _lib.stream_ptr())
    _lib.check(rc, "emd_exitwave_refine_f64")
    if capturing:
        return RefineResult(out_c, out_d, result[0], result[1], hist_loss, hist_choice, hist_steps, status[0], status[1], E)
    st = status.cpu().numpy()
    if as_np:
        res = result.cpu().numpy()
        return RefineResult(out_c.cpu().numpy(), out_d.cpu().numpy(), float(res[0]), float(res[1]), hist_loss.cpu().numpy(),
                            hist_choice.cpu().numpy(), hist_steps.cpu().numpy(), int(st[0]), int(st[1]), None if E is None else E.cpu().numpy())
    return RefineResult(out_c, out_d, result[0], result[1], hist_loss, hist_choice, hist_steps, int(st[0]), int(st[1]), E)


def refine_series(stack, defocuses, wavelength, side, window=False, refine_kw=None, **reconstruct_kw):
    """``EWREC.__init__`` with ``param_refinement=True``: ``align`` (the centres), ``refine_params`` from them and ``defocuses``, then
    ``crop_stack`` and ``reconstruct`` at the refined parameters: ``(exit wave [side,side], RefineResult)``.  ``refine_kw``: ``anchor``,
    ``step_xy``, ``step_defocus``, ``rounds``, ``candidates``, ``pad_val``, and ``iterations`` for the polls' reconstructions (default:
    ``reconstruct_kw``'s); the optics and ``pad_periods`` of ``reconstruct_kw`` hold for both."""
    name = "refine_series"
    N, S = _stack(name, stack, 2, MAX_PAIRS)
    side = _side(name, side, S)
    _padded_side(name, side, reconstruct_kw.get("pad_periods", 0))
    _recon_kw(name, {k: v for k, v in reconstruct_kw.items() if k not in ("return_stack", "return_losses")})
    rkw = dict(refine_kw or {})
    unknown = sorted(set(rkw) - {"anchor", "step_xy", "step_defocus", "rounds", "candidates", "pad_val", "iterations"})
    if unknown:
        raise TypeError(f"{name}: unexpected refine_kw key(s) {unknown}")
    shared = {k: v for k, v in reconstruct_kw.items() if k in ("px", "cs", "iterations", "pad_periods", "from_intensity", "_composed")}
    shared.update({k: rkw.pop(k) for k in ("iterations",) if k in rkw})
    x, as_np = _real(stack, _device(stack))
    _, centres = align(x, side, window, rkw.get("pad_val", 0.0))
    ref = refine_params(x, centres, defocuses, wavelength, side, **rkw, **shared)
    crops = _crop(x, ref.centres, side, rkw.get("pad_val", 0.0))
    out = reconstruct(crops, ref.defocuses, wavelength, **reconstruct_kw)
    if not as_np:
        return out, ref
    to_np = lambda v: v.cpu().numpy() if hasattr(v, "cpu") else v
    ref = RefineResult(*(to_np(v) if i not in (2, 3) else float(v) for i, v in enumerate(ref)))
    return (tuple(to_np(o) for o in out) if isinstance(out, tuple) else to_np(out)), ref
