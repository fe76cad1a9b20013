"""The exit wave and the aberrations of a focal series by gradient descent on the device (csrc/psiart.hip): the
reference's ``machine_learning/psi-art.py``.  The exit wave is ``A exp(i P)``; it goes through ``fft2``, the contrast transfer function
of every image (14 aberration amplitudes and 11 azimuths up to sixth order, a focal-spread envelope, a bounded defocus offset),
``ifft2`` and the modulus; the weighted mean-squared distance from the roots of the images is minimised with Adam over the wave, the
coefficients and the offset at once.  The reference builds this as a TensorFlow graph (and does not run as committed); here the
formulas of include/emdenoise.h are the specification and the reverse pass is hand-written.

Everything is float64.  Images are ``[N,S,S]`` float32, S a power of two, 8..2048, 1 <= N <= 64.  numpy in -> numpy out; torch CUDA
tensor in -> device tensors out, on the current stream, with no host synchronisation; arguments are checked on the shape before
anything moves to the device.  Parameters, ramp, weights and rates that are float64 CUDA tensors are used where they are: such calls
can be captured in a ``torch.cuda.graph`` and replayed after the tensors are overwritten (the bootstrapping loop of psi-art.py:334-348
is ``set_weights`` once with a device tensor, then overwriting it between replays).

Deviations from the reference: the normalisation is ``mean(r_k) / mean|b_k|`` (the reference: a complex mean against the mean of the
intensity); the loss is on ``|b_k|`` (the reference subtracts a complex tensor from a real one); the ramp and the weights are
arguments; a rate per parameter replaces ``var_to_train``.  Not here: the spatial-coherence and aperture envelopes, the rotation,
scale and shear of the per-image affine transforms and ``central_crop`` (align first with ``emdenoise.affine.align``), TIFF I/O, the
``learning_rate.txt`` polling, checkpoints, padding.

Per-image shifts, the translation part of the per-image transforms of psi-art.py:229-266: ``shifts`` ``[N,2]`` in
pixels, along axis 0 then axis 1, move prediction k by ``(d0_k, d1_k)`` as a linear phase on its transfer function; whole pixels
``(a, b)`` are ``numpy.roll(p_k, (a, b), (0, 1))``.  The shift is circular: what leaves on one side enters on the other, so a residual
of up to a pixel after ``crop_stack`` wraps one border line into the loss.  ``PsiArtFit(shifts=True)`` trains them with Adam beside
everything else, one rate per image; the middle image's rate is 0 by default, because a translation of every image at once is a
translation of the wave and one image has to fix that gauge."""
from __future__ import annotations

import numpy as np

from . import _lib
from .metrics import _p, _ws

MIN_SIDE, MAX_SIDE, MAX_IMAGES = 8, 2048, 64
NORMALISE, AMPLITUDES = 1, 2     # EMD_PSIART_NORMALISE, EMD_PSIART_AMPLITUDES
SYMBOLS = ("a22", "phi22", "a20", "a33", "phi33", "a31", "phi31", "a44", "phi44", "a42", "phi42", "a40", "a55", "phi55", "a53", "phi53",
           "a51", "phi51", "a66", "phi66", "a64", "phi64", "a62", "phi62", "a60")
NPARAM = 27                      # EMD_PSIART_NPARAM: the 25 symbols, focal_spread, the raw defocus offset
PARAM_NAMES = SYMBOLS + ("focal_spread", "defocus_offset")
RATE_NAMES = ("amplitude", "phase") + PARAM_NAMES


def energy2wavelength(v0):
    """The electron wavelength in Angstrom at ``v0`` keV (psi-art.py:85-92, its constants)."""
    m0 = 0.5109989461 * 10 ** 3      # keV / c**2
    h = 4.135667662 * 10 ** (-15) * 10 ** (-3)   # eV * s
    c = 2.99792458 * 10 ** 8         # m / s
    return h * c / np.sqrt(v0 * (2 * m0 + v0)) * 1.e10


def _side(name, S):
    if int(S) != S or not MIN_SIDE <= S <= MAX_SIDE or int(S) & (int(S) - 1):
        raise ValueError(f"{name}: the side must be a power of two, {MIN_SIDE}..{MAX_SIDE} (got {S!r})")
    return int(S)


def _positive(name, **kw):
    for k, v in kw.items():
        if not (np.isfinite(v) and v > 0):
            raise ValueError(f"{name}: {k} must be positive and finite (got {v!r})")


def polar_grid(S, sampling, wavelength):
    """``spatial_frequencies(..., return_polar=True)`` (psi-art.py:97-130) in FFT order: ``(theta, phi)``, float64 ``[S,S]`` on the
    host, with ``kx[i][j] = f[i]``, ``ky[i][j] = f[j]``, ``f = numpy.fft.fftfreq(S, sampling)``, ``theta = lam sqrt(kx^2 + ky^2)``,
    ``phi = atan2(ky, kx)``."""
    S = _side("polar_grid", S)
    _positive("polar_grid", sampling=sampling, wavelength=wavelength)
    f = np.fft.fftfreq(S, sampling)
    kx, ky = np.broadcast_to(f[:, None], (S, S)), np.broadcast_to(f[None, :], (S, S))
    return wavelength * np.sqrt(kx * kx + ky * ky), np.arctan2(ky, kx)


def defocus_ramp(n, middle=None):
    """``3 |k - middle|`` for k = 0..n-1 (psi-art.py:293-294; middle defaults to n // 2): what multiplies a20 in image k."""
    if int(n) != n or n < 1:
        raise ValueError(f"defocus_ramp: n must be a positive integer (got {n!r})")
    middle = int(n) // 2 if middle is None else middle
    if int(middle) != middle or not 0 <= middle < n:
        raise ValueError(f"defocus_ramp: middle must be an integer in 0..{int(n) - 1} (got {middle!r})")
    return 3.0 * np.abs(np.arange(int(n), dtype=np.float64) - int(middle))


def boot_weights(n, middle, boot_size):
    """The weights of the reference's bootstrapping window (psi-art.py:338-348), literally: ``lb = middle - boot_size // 2 -
    boot_size % 2``, ``ub = middle + boot_size // 2``, both pushed back inside 0..n-1, the half-open slice ``[lb:ub]`` and the divisor
    ``boot_size + 1``.  float64 ``[n]`` on the host."""
    for k, v in (("n", n), ("middle", middle), ("boot_size", boot_size)):
        if int(v) != v:
            raise ValueError(f"boot_weights: {k} must be an integer (got {v!r})")
    n, middle, boot_size = int(n), int(middle), int(boot_size)
    if n < 1 or not 0 <= middle < n or not 0 <= boot_size < n:   # the reference: boot_size in range(boot_size0, num_imgs)
        raise ValueError(f"boot_weights: n >= 1, 0 <= middle < n, 0 <= boot_size < n (got {n}, {middle}, {boot_size})")
    lb = middle - boot_size // 2 - boot_size % 2
    ub = middle + boot_size // 2
    if lb < 0:
        ub += abs(lb)
        lb = 0
    if ub >= n:
        lb -= ub - (n - 1)
        ub = n - 1
    w = np.zeros(n, np.float64)
    w[lb:ub] = 1.0 / (boot_size + 1)
    return w


def params_vector(params):
    """float64 ``[27]`` on the host from a mapping name -> value (``SYMBOLS``, "focal_spread", "defocus_offset"; the others 0) or a
    sequence of 27 numbers."""
    if isinstance(params, dict):
        unknown = sorted(set(params) - set(PARAM_NAMES))
        if unknown:
            raise ValueError(f"psiart: unknown parameter name(s) {unknown}; the names are {list(PARAM_NAMES)}")
        v = np.zeros(NPARAM, np.float64)
        for k, x in params.items():
            v[PARAM_NAMES.index(k)] = float(x)
    else:
        v = np.asarray(params, np.float64).reshape(-1).copy()
        if v.shape != (NPARAM,):
            raise ValueError(f"psiart: the parameters are {NPARAM} numbers, or a mapping by name (got {v.shape[0]})")
    if not np.isfinite(v).all():
        raise ValueError("psiart: the parameters must be finite")
    return v


def _is_dev(t):
    import torch

    return isinstance(t, torch.Tensor) and t.is_cuda


def _device(*args):
    import torch

    for a in args:
        if _is_dev(a):
            return a.device
    return torch.device("cuda", torch.cuda.current_device())


def _host_vector(name, what, v, n):
    """float64 [n] on the host, checked; a CUDA tensor is checked for its type and size only and returned as it is."""
    import torch

    if _is_dev(v):
        if v.dtype != torch.float64 or v.numel() != n or not v.is_contiguous():
            raise ValueError(f"{name}: device {what} must be a contiguous float64 tensor of {n} entries")
        return v
    if what == "params":
        return params_vector(v)
    h = np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v, np.float64).reshape(-1)
    if h.shape != (n,) or not np.isfinite(h).all():
        raise ValueError(f"{name}: {what} must be {n} finite numbers (got a shape of {h.shape})")
    return h


def _vector(name, what, v, n, device):
    """-> float64 CUDA tensor [n].  A contiguous float64 CUDA tensor of n entries is used where it is; anything else is checked on the
    host and uploaded (not while capturing)."""
    import torch

    h = _host_vector(name, what, v, n)
    if _is_dev(h):
        return h.reshape(n)
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f"{name}: {what} is not on the device; pass a float64 CUDA tensor when capturing")
    return torch.from_numpy(np.ascontiguousarray(h)).to(device)


def _images(name, images):
    """(N, S) of [N,S,S] real images, checked before anything moves."""
    import torch

    shp = tuple(images.shape) if hasattr(images, "shape") else np.shape(images)
    if len(shp) != 3 or shp[1] != shp[2]:
        raise ValueError(f"{name}: images are [N,S,S], square (got a shape of {shp})")
    N, S = int(shp[0]), _side(name, shp[1])
    if not 1 <= N <= MAX_IMAGES:
        raise ValueError(f"{name}: 1..{MAX_IMAGES} images (got {N})")
    if isinstance(images, torch.Tensor) and images.is_complex() or not isinstance(images, torch.Tensor) and np.iscomplexobj(images):
        raise ValueError(f"{name}: the images are real (float32)")
    return N, S


def _shift_pairs(name, v, N, device):
    """``shifts`` -> float64 CUDA tensor [N,2].  A contiguous float64 CUDA tensor of that shape is used where it is; anything else is
    checked on the host and uploaded (not while capturing)."""
    import torch

    shp = tuple(v.shape) if hasattr(v, "shape") else np.shape(v)
    if shp != (N, 2):
        raise ValueError(f"{name}: shifts are [N,2] = [{N},2], in pixels (got a shape of {shp})")
    return _vector(name, "shifts", v.reshape(-1) if isinstance(v, torch.Tensor) else np.asarray(v, np.float64).reshape(-1), 2 * N,
                   device).view(N, 2)


def _to_dev(a, dtype, device):
    import torch

    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(device=device, dtype=dtype).contiguous()


def ctf(S, wavelength, sampling, params, ramp=(0.0,), offset_scale=1.0):
    """The contrast transfer functions ``C_k = exp(-i chi_k) T`` of the images whose a20 multipliers are ``ramp`` (get_ctf,
    psi-art.py:204-220, without the spatial and aperture envelopes): complex128 ``[len(ramp),S,S]`` in FFT order.  ``params``: 27
    numbers or a mapping by name.  numpy out, unless ``params`` or ``ramp`` is a CUDA tensor."""
    import torch

    S = _side("ctf", S)
    _positive("ctf", wavelength=wavelength, sampling=sampling, offset_scale=offset_scale)
    n = int(ramp.numel()) if isinstance(ramp, torch.Tensor) else int(np.size(ramp))
    if not 1 <= n <= 65535:
        raise ValueError(f"ctf: 1..65535 ramp entries (got {n})")
    params, ramp = _host_vector("ctf", "params", params, NPARAM), _host_vector("ctf", "ramp", ramp, n)
    as_np = not (_is_dev(params) or _is_dev(ramp))
    device = _device(params, ramp)
    p = _vector("ctf", "params", params, NPARAM, device)
    r = _vector("ctf", "ramp", ramp, n, device)
    out = torch.empty((n, S, S), dtype=torch.complex128, device=device)
    _lib.check(_lib.load().emd_psiart_ctf_f64(S, n, _p(p), _p(r), float(wavelength), float(sampling), float(offset_scale), _p(out),
                                              _lib.stream_ptr()), "emd_psiart_ctf_f64")
    return out.cpu().numpy() if as_np else out


def _loss_grad(name, images, amplitude, phase, params, ramp, weights, wavelength, sampling, offset_scale, flags, want_pred, want_grad,
               shifts=None):
    import torch

    N, S = _images(name, images)
    _positive(name, wavelength=wavelength, sampling=sampling, offset_scale=offset_scale)
    for what, a in (("amplitude", amplitude), ("phase", phase)):
        shp = tuple(a.shape) if hasattr(a, "shape") else np.shape(a)
        if shp != (S, S):
            raise ValueError(f"{name}: {what} is [S,S] = [{S},{S}] (got a shape of {shp})")
    params = _host_vector(name, "params", params, NPARAM)
    ramp = _host_vector(name, "ramp", defocus_ramp(N) if ramp is None else ramp, N)
    weights = _host_vector(name, "weights", np.full(N, 1.0 / N) if weights is None else weights, N)
    if shifts is not None and not _is_dev(shifts):   # checked on the host before anything moves
        if np.shape(shifts) != (N, 2) or not np.isfinite(np.asarray(shifts, np.float64)).all():
            raise ValueError(f"{name}: shifts are [N,2] = [{N},2] finite numbers, in pixels (got a shape of {np.shape(shifts)})")
    as_np = not _is_dev(images) and not _is_dev(amplitude)
    device = _device(images, amplitude, phase)
    A, P = _to_dev(amplitude, torch.float64, device), _to_dev(phase, torch.float64, device)
    p, r, w = _vector(name, "params", params, NPARAM, device), _vector(name, "ramp", ramp, N, device), _vector(name, "weights", weights, N, device)
    x = _to_dev(images, torch.float32, device)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=device)
    out = {"losses": f64(N + 1), "predictions": f64(N, S, S) if want_pred else None, "g_amplitude": f64(S, S) if want_grad else None,
           "g_phase": f64(S, S) if want_grad else None, "g_params": f64(NPARAM) if want_grad else None}
    lib = _lib.load()
    if shifts is None:
        nbytes = lib.emd_psiart_workspace_bytes(N, S)
        ws = _ws(nbytes, device)
        _lib.check(lib.emd_psiart_loss_grad_f64(_p(x), N, S, _p(A), _p(P), _p(p), _p(r), _p(w), float(wavelength), float(sampling),
                                                float(offset_scale), flags, _p(out["losses"]), _p(out["predictions"]),
                                                _p(out["g_amplitude"]), _p(out["g_phase"]), _p(out["g_params"]), _p(ws), nbytes,
                                                _lib.stream_ptr()),
                   "emd_psiart_loss_grad_f64")
    else:
        d = _shift_pairs(name, shifts, N, device)
        out["g_shifts"] = f64(N, 2) if want_grad else None
        nbytes = lib.emd_psiart_shift_workspace_bytes(N, S)
        ws = _ws(nbytes, device)
        _lib.check(lib.emd_psiart_shift_loss_grad_f64(_p(x), N, S, _p(A), _p(P), _p(p), _p(d), _p(r), _p(w), float(wavelength),
                                                      float(sampling), float(offset_scale), flags, _p(out["losses"]),
                                                      _p(out["predictions"]), _p(out["g_amplitude"]), _p(out["g_phase"]),
                                                      _p(out["g_params"]), _p(out["g_shifts"]), _p(ws), nbytes, _lib.stream_ptr()),
                   "emd_psiart_shift_loss_grad_f64")
    out = {k: v for k, v in out.items() if v is not None}
    out["loss"] = out["losses"][N]
    out["losses"] = out["losses"][:N]
    return {k: v.cpu().numpy() for k, v in out.items()} if as_np else out


def forward(amplitude, phase, params, ramp, wavelength, sampling, offset_scale=1.0, images=None, from_intensity=True, shifts=None):
    """The model's images ``p_k = c_k |ifft2(C_k fft2(A exp(i P)))|``, float64 ``[len(ramp),S,S]``.  Without ``images`` ``c_k = 1``;
    with them ``c_k = mean(r_k) / mean|b_k|`` (``r_k`` the root of image k; ``from_intensity=False``: ``|image_k|``).  ``shifts``
    ``[len(ramp),2]`` (numpy or a float64 CUDA tensor): image k moved circularly by ``(d0_k, d1_k)`` pixels."""
    import torch

    shp = tuple(amplitude.shape) if hasattr(amplitude, "shape") else np.shape(amplitude)
    if len(shp) != 2 or shp[0] != shp[1]:
        raise ValueError(f"forward: amplitude is [S,S] (got a shape of {shp})")
    n = int(ramp.numel()) if isinstance(ramp, torch.Tensor) else int(np.size(ramp))
    flags = (0 if from_intensity else AMPLITUDES) | (NORMALISE if images is not None else 0)
    if images is None:
        if not 1 <= n <= MAX_IMAGES:
            raise ValueError(f"forward: 1..{MAX_IMAGES} ramp entries (got {n})")
        _side("forward", shp[0])
        images = torch.zeros((n, shp[0], shp[0]), dtype=torch.float32, device=_device(amplitude, phase)) if _is_dev(amplitude) else \
            np.zeros((n, shp[0], shp[0]), np.float32)
    return _loss_grad("forward", images, amplitude, phase, params, ramp, None, wavelength, sampling, offset_scale, flags, True, False,
                      shifts)["predictions"]


def loss_and_gradients(images, amplitude, phase, params, wavelength, sampling, ramp=None, weights=None, offset_scale=1.0, normalise=True,
                       from_intensity=True, gradients=True, predictions=False, shifts=None):
    """The loss of the model against ``images`` and its gradients: a dict with ``losses`` ``[N]`` (``mean((p_k - r_k)^2)``), ``loss``
    (``sum_k w_k loss_k``) and, with ``gradients``, ``g_amplitude`` and ``g_phase`` ``[S,S]`` and ``g_params`` ``[27]`` (the order of
    ``PARAM_NAMES``; the last is the gradient by the raw offset u); with ``predictions`` also ``predictions`` ``[N,S,S]``.  ``ramp``
    defaults to ``defocus_ramp(N)``, ``weights`` to ``1 / N``.  Without ``gradients`` the reverse launches are not made.  With
    ``shifts`` ``[N,2]`` (pixels along axis 0, then axis 1; numpy or a float64 CUDA tensor) image k of the model is moved circularly by
    ``(d0_k, d1_k)`` and the gradients gain ``g_shifts`` ``[N,2]``."""
    flags = (NORMALISE if normalise else 0) | (0 if from_intensity else AMPLITUDES)
    return _loss_grad("loss_and_gradients", images, amplitude, phase, params, ramp, weights, wavelength, sampling, offset_scale, flags,
                      predictions, gradients, shifts)


class PsiArtFit:
    """The fit of psi-art.py's ``experiment``: the exit wave ``A exp(i P)``, the aberration coefficients and the defocus offset, fitted
    to the roots of ``images`` ``[N,S,S]`` with Adam (``tf.train.AdamOptimizer``'s form; the reference's beta1 = 0.99, epsilon = 0.1).

    The amplitude starts as the root of the middle image and the phase as 0 (psi-art.py:61-66).  The coefficients named in ``symbols``
    start at ``estimates`` and are trained; the others are constants 0 (:76-80).  The defocus offset is trained too, and the focal
    spread when ``focal_spread`` (its estimate) is given.  ``rates`` overrides the rate of anything: a mapping by name (``RATE_NAMES``:
    "amplitude", "phase", the symbols, "focal_spread", "defocus_offset"), 29 numbers in that order, or a float64 CUDA tensor of 29
    entries that is used where it is.  A rate of 0 means "not trained".

    ``shifts=True`` (from 0) or an ``[N,2]`` array (pixels along axis 0, then axis 1) also trains a circular sub-pixel shift of every
    image, at ``shift_rate`` (default ``learning_rate``); ``set_shift_rates`` takes one rate per image.  The ``middle`` image's rate
    starts at 0: moving every image by the same amount is the same as moving the wave, so one image is the gauge and stays where it
    is.  With ``shifts=None`` nothing of this exists and the calls are the ones without shifts.

    ``step(n)`` makes n steps, each ten launches on the current stream and nothing else: it can be captured."""

    def __init__(self, images, wavelength, sampling, symbols=("a20", "a40"), estimates=(50., 0.), middle=None, ramp=None, normalise=True,
                 from_intensity=True, learning_rate=1e-3, rates=None, beta1=0.99, beta2=0.999, epsilon=0.1, offset_scale=1.0,
                 focal_spread=None, shifts=None, shift_rate=None):
        import torch

        N, S = _images("PsiArtFit", images)
        _positive("PsiArtFit", wavelength=wavelength, sampling=sampling, offset_scale=offset_scale, epsilon=epsilon)
        if not (0 <= beta1 < 1 and 0 <= beta2 < 1):
            raise ValueError(f"PsiArtFit: 0 <= beta1, beta2 < 1 (got {beta1!r}, {beta2!r})")
        if not (np.isfinite(learning_rate) and learning_rate >= 0):
            raise ValueError(f"PsiArtFit: learning_rate must be finite and not negative (got {learning_rate!r})")
        symbols, estimates = tuple(symbols), tuple(estimates)
        if len(symbols) != len(estimates) or len(set(symbols)) != len(symbols) or not set(symbols) <= set(SYMBOLS):
            raise ValueError(f"PsiArtFit: symbols are distinct names out of {list(SYMBOLS)}, one estimate each (got {symbols}, "
                             f"{len(estimates)} estimates)")
        middle = N // 2 if middle is None else middle
        if int(middle) != middle or not 0 <= middle < N:
            raise ValueError(f"PsiArtFit: middle must be an integer in 0..{N - 1} (got {middle!r})")
        p0 = params_vector(dict(zip(symbols, estimates), focal_spread=0.0 if focal_spread is None else focal_spread))
        self.N, self.S, self.middle = N, S, int(middle)
        self.wavelength, self.sampling, self.offset_scale = float(wavelength), float(sampling), float(offset_scale)
        self.beta1, self.beta2, self.epsilon = float(beta1), float(beta2), float(epsilon)
        self.flags = (NORMALISE if normalise else 0) | (0 if from_intensity else AMPLITUDES)
        default = {"amplitude": learning_rate, "phase": learning_rate, "defocus_offset": learning_rate}
        default.update({s: learning_rate for s in symbols})
        if focal_spread is not None:
            default["focal_spread"] = learning_rate
        if rates is None or not _is_dev(rates):   # checked on the host before anything moves
            rates = self._rates_host(default if rates is None else rates)
        if ramp is not None and not _is_dev(ramp) and (np.shape(ramp) != (N,) or not np.isfinite(np.asarray(ramp, np.float64)).all()):
            raise ValueError(f"PsiArtFit: ramp must be {N} finite numbers")
        if shifts is None and shift_rate is not None:
            raise ValueError("PsiArtFit: shift_rate without shifts (pass shifts=True to train them from 0)")
        if shifts is not None:
            shift_rate = learning_rate if shift_rate is None else shift_rate
            if not (np.isfinite(shift_rate) and shift_rate >= 0):
                raise ValueError(f"PsiArtFit: shift_rate must be finite and not negative (got {shift_rate!r})")
            d0 = np.zeros((N, 2), np.float64) if shifts is True else shifts
            if not _is_dev(d0) and (np.shape(d0) != (N, 2) or not np.isfinite(np.asarray(d0, np.float64)).all()):
                raise ValueError(f"PsiArtFit: shifts are True or [N,2] = [{N},2] finite numbers, in pixels")
        self._as_np = not _is_dev(images)
        self.device = device = _device(images)
        self._rates = self._rate_tensor(rates)
        self._ramp = _vector("PsiArtFit", "ramp", defocus_ramp(N, self.middle) if ramp is None else ramp, N, device)
        self._weights = _vector("PsiArtFit", "weights", np.full(N, 1.0 / N), N, device)
        self.images = _to_dev(images, torch.float32, device)      # a contiguous float32 CUDA tensor is used where it is
        mid = self.images[self.middle].to(torch.float64)
        self._amp = (mid.clamp_min(0.0).sqrt() if from_intensity else mid.abs()).contiguous()
        self._phase = torch.zeros((S, S), dtype=torch.float64, device=device)
        self._params = torch.from_numpy(p0).to(device)
        self._moments = [torch.zeros_like(t) for t in (self._amp, self._amp, self._phase, self._phase, self._params, self._params)]
        self._step = torch.zeros(1, dtype=torch.int32, device=device)
        self._losses = torch.zeros(N + 1, dtype=torch.float64, device=device)
        self._shifts = None
        if shifts is not None:
            self._shifts = _shift_pairs("PsiArtFit", d0, N, device).clone()
            self._shift_moments = [torch.zeros_like(self._shifts), torch.zeros_like(self._shifts)]
            r0 = np.full(N, float(shift_rate))
            r0[self.middle] = 0.0                     # the gauge: a common translation belongs to the wave
            self._shift_rates = torch.from_numpy(r0).to(device)
        self._nbytes = (_lib.load().emd_psiart_workspace_bytes if shifts is None else _lib.load().emd_psiart_shift_workspace_bytes)(N, S)
        self._ws = _ws(self._nbytes, device)

    @staticmethod
    def _rates_host(rates):
        if isinstance(rates, dict):
            unknown = sorted(set(rates) - set(RATE_NAMES))
            if unknown:
                raise ValueError(f"PsiArtFit: unknown rate name(s) {unknown}; the names are {list(RATE_NAMES)}")
            v = np.zeros(len(RATE_NAMES), np.float64)
            for k, x in rates.items():
                v[RATE_NAMES.index(k)] = float(x)
        else:
            v = np.asarray(rates, np.float64).reshape(-1).copy()
        if v.shape != (len(RATE_NAMES),) or not np.isfinite(v).all() or (v < 0).any():
            raise ValueError(f"PsiArtFit: the rates are {len(RATE_NAMES)} finite numbers >= 0, or a mapping by name")
        return v

    def _rate_tensor(self, rates):
        return _vector("PsiArtFit", "rates", rates if _is_dev(rates) else self._rates_host(rates), len(RATE_NAMES), self.device)

    def set_rates(self, rates=None, **by_name):
        """New rates: a float64 CUDA tensor of 29 entries is adopted where it is; 29 numbers or a mapping by name (or keywords, on top of
        the current ones) are copied into the tensor in use, so that a captured ``step`` sees them on replay."""
        if _is_dev(rates):
            self._rates = self._rate_tensor(rates)
            return self
        if rates is None:
            v = self._rates.cpu().numpy()
            extra = self._rates_host(by_name)
            for k in by_name:
                v[RATE_NAMES.index(k)] = extra[RATE_NAMES.index(k)]
        else:
            v = self._rates_host(rates)
        import torch

        self._rates.copy_(torch.from_numpy(v))
        return self

    def set_weights(self, w):
        """The weights of the images' losses in L (for instance ``boot_weights``).  A float64 CUDA tensor of N entries is adopted where
        it is; anything else is copied into the tensor in use."""
        import torch

        if _is_dev(w):
            self._weights = _vector("PsiArtFit", "weights", w, self.N, self.device)
        else:
            h = np.asarray(w, np.float64).reshape(-1)
            if h.shape != (self.N,) or not np.isfinite(h).all():
                raise ValueError(f"PsiArtFit: weights must be {self.N} finite numbers")
            self._weights.copy_(torch.from_numpy(h.copy()))
        return self

    def set_shift_rates(self, v):
        """One rate per image for its shift (both axes).  A float64 CUDA tensor of N entries is adopted where it is; anything else is
        copied into the tensor in use, so that a captured ``step`` sees it on replay.  A rate of 0 freezes that image's shift."""
        import torch

        if self._shifts is None:
            raise ValueError("PsiArtFit.set_shift_rates: this fit has no shifts (construct it with shifts=True or an [N,2] array)")
        if _is_dev(v):
            self._shift_rates = _vector("PsiArtFit", "shift rates", v, self.N, self.device)
        else:
            h = np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v, np.float64).reshape(-1)
            if h.shape != (self.N,) or not np.isfinite(h).all() or (h < 0).any():
                raise ValueError(f"PsiArtFit: the shift rates are {self.N} finite numbers >= 0")
            self._shift_rates.copy_(torch.from_numpy(h.copy()))
        return self

    def step(self, n=1):
        """n Adam steps.  ``losses`` and ``loss`` afterwards are those of the last step, before its update."""
        if int(n) != n or n < 0:
            raise ValueError(f"PsiArtFit.step: n must be a non-negative integer (got {n!r})")
        lib = _lib.load()
        m = self._moments
        if self._shifts is not None:
            sm = self._shift_moments
            for _ in range(int(n)):
                _lib.check(lib.emd_psiart_shift_step_f64(_p(self.images), self.N, self.S, _p(self._amp), _p(self._phase), _p(self._params),
                                                         _p(self._shifts), _p(self._ramp), _p(self._weights), self.wavelength,
                                                         self.sampling, self.offset_scale, self.flags, _p(m[0]), _p(m[1]), _p(m[2]),
                                                         _p(m[3]), _p(m[4]), _p(m[5]), _p(sm[0]), _p(sm[1]), _p(self._step),
                                                         _p(self._rates), _p(self._shift_rates), self.beta1, self.beta2, self.epsilon,
                                                         _p(self._losses), _p(None), _p(None), _p(None), _p(None), _p(None), _p(self._ws),
                                                         self._nbytes, _lib.stream_ptr()),
                           "emd_psiart_shift_step_f64")
            return self
        for _ in range(int(n)):
            _lib.check(lib.emd_psiart_step_f64(_p(self.images), self.N, self.S, _p(self._amp), _p(self._phase), _p(self._params),
                                               _p(self._ramp), _p(self._weights), self.wavelength, self.sampling, self.offset_scale,
                                               self.flags, _p(m[0]), _p(m[1]), _p(m[2]), _p(m[3]), _p(m[4]), _p(m[5]), _p(self._step),
                                               _p(self._rates), self.beta1, self.beta2, self.epsilon, _p(self._losses), _p(None),
                                               _p(None), _p(None), _p(None), _p(self._ws), self._nbytes, _lib.stream_ptr()),
                       "emd_psiart_step_f64")
        return self

    def _out(self, t):
        return t.cpu().numpy() if self._as_np else t

    @property
    def losses(self):
        return self._out(self._losses[:self.N])

    @property
    def loss(self):
        return float(self._losses[self.N]) if self._as_np else self._losses[self.N]

    @property
    def amplitude(self):
        return self._out(self._amp)

    @property
    def phase(self):
        return self._out(self._phase)

    @property
    def wave(self):
        import torch

        return self._out(torch.polar(self._amp, self._phase))

    @property
    def params(self):
        """The 27 scalars in the order of ``PARAM_NAMES`` (the last is the raw offset u)."""
        return self._out(self._params)

    @property
    def shifts(self):
        """The shifts ``[N,2]`` in pixels (axis 0, then axis 1), or None for a fit without them."""
        return None if self._shifts is None else self._out(self._shifts)

    @property
    def steps(self):
        return int(self._step)

    @property
    def aberrations(self):
        """name -> value on the host: the 25 symbols, "focal_spread" and "defocus_offset" = scale tanh(u / scale) (a read-back)."""
        v = self._params.cpu().numpy()
        out = {k: float(x) for k, x in zip(PARAM_NAMES, v)}
        out["defocus_offset"] = float(self.offset_scale * np.tanh(v[NPARAM - 1] / self.offset_scale))
        return out
