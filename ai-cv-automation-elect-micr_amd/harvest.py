"""Harvesting raw micrographs on the device (csrc/harvest.hip): the step of the reference that turns a raw
micrograph of any size into a 2048 x 2048 float32 training image in [0, 1] and a table of statistics -- the MATLAB harvester,
DM3stoTIFs-batch/img_params.m, img_params_lq.m and estimate_noise.m.  Crop to the smaller dimension (top-left), box-resize
(``imresize(..., 'method', 'box')``: the unweighted mean of each output's member pixels), statistics, ``(x - min) / (max - min)``.
MATLAB is not used: the arithmetic is restated from the formulas in include/emdenoise.h.

The conventions of ``emdenoise.filters``: images are float32 ``[H,W]``, ``[B,H,W]`` or ``[B,H,W,1]``; numpy in -> numpy out; torch
CUDA tensor in -> device tensor out, on the current stream, with no host synchronisation; arguments are checked on the shape
before anything moves to the device.  Python here only shapes buffers: every number comes from a HIP kernel (the box-resize table
from the library's host function).  Values must be finite: NaN / Inf are the caller's problem.  3 <= H, W <= 32768; size <= 8192.

The four ``*Freq2048`` fields of img_params.m (:53-77) come from csrc/fft.hip: ``rfft2`` (the 2-D real-to-complex
FFT in double), ``radial_profile`` and ``freq_stats`` (the moments of the radial profile of ``|fftshift(fft2(x))|``), for square
images whose side is a power of two, 8..4096.  ``img_params(..., freq=True)`` adds them to the table."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .metrics import _dims, _images, _p, _ws

NSTATS = 17   # EMD_NSTATS
STAT_NAMES = ["min", "max", "nonzero", "negative", "mean", "std", "skewness", "kurtosis", "median", "rms", "coeff_variation", "noise",
              "sqrt_mean", "sqrt_std", "sqrt_skewness", "sqrt_kurtosis", "sqrt_mean_ratio"]
MAX_EXTENT, MAX_SIZE = 32768, 8192
NFREQ = 4     # EMD_NFREQ
FREQ_NAMES = ["mean", "std", "skewness", "kurtosis"]
MIN_FFT, MAX_FFT = 8, 4096

# img_params.m's field names -> STAT_NAMES.  From the resized image (the reference wrote "2048" into the names whatever the size):
FIELDS_2048 = {"noise2048": "noise", "mean2048": "mean", "stddev2048": "std", "skewness": "skewness", "kurtosis": "kurtosis",
               "min2048": "min", "max2048": "max", "median2048": "median", "coeffVariation2048": "coeff_variation", "rms2048": "rms",
               "mean_of_noiseFromGauss": "sqrt_mean", "stddev_of_noiseFromGauss": "sqrt_std", "skewness_of_noiseFromGauss": "sqrt_skewness",
               "kurtosis_of_noiseFromGauss": "sqrt_kurtosis", "ratio_of_meanNoise_to_mean": "sqrt_mean_ratio"}
# from the image scaled to [0, 1]:
FIELDS_0TO1 = {"noise2048_for_0to1": "noise", "mean2048_for_0to1": "mean", "stddev2048_for_0to1": "std", "median2048_for_0to1": "median",
               "coeffVariation2048_for_0to1": "coeff_variation", "rms_0to1": "rms", "mean_of_noiseFromGauss_for_0to1": "sqrt_mean",
               "stddev_of_noiseFromGauss_for_0to1": "sqrt_std", "skewness_of_noiseFromGauss_for_0to1": "sqrt_skewness",
               "kurtosis_of_noiseFromGauss_for_0to1": "sqrt_kurtosis", "ratio_of_meanNoise_to_mean_for_0to1": "sqrt_mean_ratio"}
# from the raw image (besides smallestDim, imageDims, num_px and the two proportions):
FIELDS_RAW = {"min": "min", "max": "max", "numberNonZero": "nonzero", "numNegative": "negative"}
# img_params(freq=True): from the radial profile of the resized image's spectrum -> FREQ_NAMES ("mean" is the profile's sum)
FIELDS_FREQ = {"meanFreq2048": "mean", "stddevFreq2048": "std", "skewnessFreq2048": "skewness", "kurtosisFreq2048": "kurtosis"}

_tables = {}   # (d, S, device) -> the device copy of box_table(d, S): an upload cannot happen inside a capture


def _check_size(name, size):
    if int(size) != size or not 1 <= size <= MAX_SIZE:
        raise ValueError(f"{name}: size must be an integer, 1..{MAX_SIZE} (got {size!r})")
    return int(size)


def _check_fft_size(name, S):
    if int(S) != S or not MIN_FFT <= S <= MAX_FFT or int(S) & (int(S) - 1):
        raise ValueError(f"{name}: the FFT needs a size that is a power of two, {MIN_FFT}..{MAX_FFT} (got {S!r})")
    return int(S)


def _check_square(name, x):
    B, H, W = _dims(x)
    if H != W:
        raise ValueError(f"{name}: square images, the side a power of two, {MIN_FFT}..{MAX_FFT} (got {H} x {W})")
    return B, _check_fft_size(name, H)


def _check_extent(name, H, W, least=3):
    if min(H, W) < least or max(H, W) > MAX_EXTENT:
        raise ValueError(f"{name}: {least} <= H, W <= {MAX_EXTENT} (got {H} x {W})")


def _shaped(y, like_ndim, as_np):
    """[B,h,w] in the rank of the argument."""
    if like_ndim == 2:
        y = y.reshape(y.shape[1], y.shape[2])
    elif like_ndim == 4:
        y = y.reshape(*y.shape, 1)
    return y.cpu().numpy() if as_np else y


def box_table(n_in, n_out):
    """int32 ``[n_out, 2]``: (first member, 0-based; member count) of every output sample of MATLAB's box resize n_in -> n_out along
    one axis, from the library's host function (``emd_box_resize_table``: the one copy of that arithmetic)."""
    if int(n_in) != n_in or not 1 <= n_in <= MAX_EXTENT:
        raise ValueError(f"box_table: n_in must be an integer, 1..{MAX_EXTENT} (got {n_in!r})")
    n_out = _check_size("box_table", n_out)
    tab = np.empty((n_out, 2), np.int32)
    _lib.check(_lib.load().emd_box_resize_table(int(n_in), n_out, tab.ctypes.data_as(C.c_void_p)), "emd_box_resize_table")
    return tab


def _device_table(d, S, device):
    import torch

    key = (d, S, str(device))
    if key not in _tables:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"box_resize: the table of {d} -> {S} is not on the device yet; call box_resize once before capturing")
        _tables[key] = torch.from_numpy(box_table(d, S)).to(device)
    return _tables[key]


def box_resize(x, size=2048):
    """Crop to the top-left d x d pixels, d = min(H, W), and box-resize to size x size: every output pixel is the unweighted mean of
    the pixels of its row run x its column run (``box_table(d, size)``), summed in double in a fixed order.  size > d is nearest
    neighbour; size == d returns the crop, bit for bit.  -> ``[B,size,size]`` in the rank of x."""
    import torch

    B, H, W = _dims(x)
    size = _check_size("box_resize", size)
    _check_extent("box_resize", H, W, least=1)
    xd, as_np = _images(x)
    d = min(H, W)
    tab = _device_table(d, size, xd.device)
    out = torch.empty((B, size, size), dtype=torch.float32, device=xd.device)
    _lib.check(_lib.load().emd_box_resize_f32(_p(xd), C.c_long(H * W), W, B, d, _p(out), size, _p(tab), _lib.stream_ptr()),
               "emd_box_resize_f32")
    return _shaped(out, len(np.shape(x)), as_np)


def _stats_device(xd):
    """[B,H,W] device tensor -> [B,17] float64 device tensor."""
    import torch

    B, H, W = xd.shape
    lib = _lib.load()
    stats = torch.empty((B, NSTATS), dtype=torch.float64, device=xd.device)
    nbytes = lib.emd_image_stats_workspace_bytes(B, H, W)
    ws = _ws(nbytes, xd.device)
    _lib.check(lib.emd_image_stats_f64(_p(xd), B, H, W, _p(stats), _p(ws), nbytes, _lib.stream_ptr()), "emd_image_stats_f64")
    return stats


def image_stats(x):
    """``[B, 17]`` float64, the columns named by ``STAT_NAMES``: min, max, the counts of non-zero and of negative pixels, mean, std
    (N - 1), skewness and kurtosis (population central moments; not excess), the exact median, rms, 100 std / mean, the Immerkaer noise
    level of estimate_noise.m (over the full, zero-padded convolution), the four moments of sqrt(max(x, 0)) and sqrt_mean / mean.
    Two-pass central moments in double; bitwise reproducible, and an image's row does not depend on the batch it is in."""
    _, H, W = _dims(x)
    _check_extent("image_stats", H, W)
    xd, as_np = _images(x)
    stats = _stats_device(xd)
    return stats.cpu().numpy() if as_np else stats


def estimate_noise(x):
    """``estimate_noise.m``: sum |conv2(x, [1 -2 1; -2 4 -2; 1 -2 1])| sqrt(pi / 2) / (6 (W - 2) (H - 2)) per image, ``[B]`` float64: the
    number ``filters.wiener(noise=)`` (its square) and ``filters.denoise_wavelet(sigma=)`` take."""
    return image_stats(x)[:, STAT_NAMES.index("noise")]


def _scale_device(xd, stats):
    import torch

    out = torch.empty_like(xd)
    B = xd.shape[0]
    _lib.check(_lib.load().emd_scale01_f32(_p(xd), _p(out), B, C.c_long(xd.numel() // max(B, 1)), _p(stats), _lib.stream_ptr()),
               "emd_scale01_f32")
    return out


def scale01(x):
    """(x - min) / (max - min) of every image, in float32, min and max found (and read) on the device.  A constant image
    (|max - min| < 1e-6) becomes 0.5 (the MATLAB gives NaN there)."""
    _, H, W = _dims(x)
    _check_extent("scale01", H, W)
    xd, as_np = _images(x)
    return _shaped(_scale_device(xd, _stats_device(xd)), len(np.shape(x)), as_np)


def radial_bins(S):
    """R = ceil(sqrt(2 (S / 2 + 1)^2)), the length of the radial profile of an S x S spectrum: 1450 at 2048, img_params.m's
    ``maxRadius``."""
    return int(_lib.load().emd_radial_bins(_check_fft_size("radial_bins", S)))


def rfft2(x):
    """``numpy.fft.rfft2`` of the float64 cast: complex128 ``[B,S,S/2+1]`` in the rank of x (forward, unnormalised, unshifted), by a
    hand-written FFT in double.  Square images, the side a power of two, 8..4096."""
    import torch

    B, S = _check_square("rfft2", x)
    xd, as_np = _images(x)
    lib = _lib.load()
    spec = torch.empty((B, S, S // 2 + 1), dtype=torch.complex128, device=xd.device)
    nbytes = lib.emd_rfft2_workspace_bytes(B, S)
    ws = _ws(nbytes, xd.device)
    _lib.check(lib.emd_rfft2_f64(_p(xd), B, S, _p(spec), _p(ws), nbytes, _lib.stream_ptr()), "emd_rfft2_f64")
    return _shaped(spec, len(np.shape(x)), as_np)


def _freq_device(xd, want_profile):
    """[B,S,S] device tensor -> ([B,R] float64 or None, [B,4] float64)."""
    import torch

    B, S = int(xd.shape[0]), int(xd.shape[1])
    lib = _lib.load()
    prof = torch.empty((B, lib.emd_radial_bins(S)), dtype=torch.float64, device=xd.device) if want_profile else None
    out = torch.empty((B, NFREQ), dtype=torch.float64, device=xd.device)
    nbytes = lib.emd_freq_stats_workspace_bytes(B, S)
    ws = _ws(nbytes, xd.device)
    _lib.check(lib.emd_freq_stats_f64(_p(xd), B, S, _p(prof), _p(out), _p(ws), nbytes, _lib.stream_ptr()), "emd_freq_stats_f64")
    return prof, out


def radial_profile(x):
    """``[B, R]`` float64, R = ``radial_bins(S)``: img_params.m's ``radialProfile`` after its last two statements,
    ``profile / sum(profile) * radialFreqs``, where ``profile[t]`` sums ``|fft2(x)|`` over the pixels whose distance from the
    shifted spectrum's centre has ``ceil`` t and ``radialFreqs[t]`` is distance / R of the last such pixel the reference's loop
    visits (largest column, then largest row); a bin without a pixel is 0."""
    _check_square("radial_profile", x)
    xd, as_np = _images(x)
    prof = _freq_device(xd, True)[0]
    return prof.cpu().numpy() if as_np else prof


def freq_stats(x):
    """``[B, 4]`` float64, the columns named by ``FREQ_NAMES``: of ``p = radial_profile(x)``, its SUM (the reference calls it the
    mean), std (R - 1), skewness and kurtosis (population central moments about sum / R; not excess), two-pass in double.  An
    all-zero image gives four NaN; a constant non-zero image has p = 0: mean 0, std 0, skewness and kurtosis NaN (as MATLAB)."""
    _check_square("freq_stats", x)
    xd, as_np = _images(x)
    out = _freq_device(xd, False)[1]
    return out.cpu().numpy() if as_np else out


def _one_image(name, img):
    shp = tuple(np.shape(img))
    if len(shp) != 2:
        raise ValueError(f"{name}: one image [H,W] (got shape {shp})")
    _check_extent(name, *shp)


def img_params(img, size=2048, freq=False):
    """``img_params.m`` for one raw image ``[H,W]`` -> ``(stats, image)``: the dict of the reference's own field names and the image
    cropped, box-resized to size x size and scaled to [0, 1] (float32; numpy for a numpy argument, else a device tensor).

    From the raw image: ``smallestDim``, ``imageDims``, ``num_px``, ``min``, ``max``, ``numberNonZero``, ``proportionZero`` (the
    reference's value, numberNonZero / num_px: the proportion of NON-zero pixels, whatever the name says), ``numNegative``,
    ``proportionNegative``.  From the resized image: the ``*2048`` fields and the moments of its square root (``FIELDS_2048``; the
    names say 2048 whatever the size).  From the scaled image: the ``*_for_0to1`` fields and ``rms_0to1`` (``FIELDS_0TO1``).
    freq=True adds the four ``*Freq2048`` fields (``FIELDS_FREQ``: ``freq_stats`` of the resized, unscaled image); size must then
    be a power of two, 8..4096."""
    import torch

    size = _check_size("img_params", size)
    if freq:
        _check_fft_size("img_params", size)
    _one_image("img_params", img)
    xd, as_np = _images(img)
    H, W = int(xd.shape[1]), int(xd.shape[2])
    raw = _stats_device(xd)
    small = box_resize(xd, size)
    s2048 = _stats_device(small)
    scaled = _scale_device(small, s2048)
    s01 = _stats_device(scaled)
    parts = [raw[0], s2048[0], s01[0]] + ([_freq_device(small, False)[1][0]] if freq else [])
    host = torch.cat(parts).cpu().numpy()   # the one read-back
    raw, s2048, s01, sfreq = host[:NSTATS], host[NSTATS:2 * NSTATS], host[2 * NSTATS:3 * NSTATS], host[3 * NSTATS:]
    col = {n: i for i, n in enumerate(STAT_NAMES)}
    n = H * W
    stats = {"smallestDim": min(H, W), "imageDims": (H, W), "num_px": n}
    stats.update({k: float(raw[col[v]]) for k, v in FIELDS_RAW.items()})
    stats["numberNonZero"], stats["numNegative"] = int(stats["numberNonZero"]), int(stats["numNegative"])
    stats["proportionZero"] = stats["numberNonZero"] / n
    stats["proportionNegative"] = stats["numNegative"] / n
    stats.update({k: float(s2048[col[v]]) for k, v in FIELDS_2048.items()})
    stats.update({k: float(s01[col[v]]) for k, v in FIELDS_0TO1.items()})
    if freq:
        stats.update({k: float(sfreq[FREQ_NAMES.index(v)]) for k, v in FIELDS_FREQ.items()})
    image = scaled[0]
    return stats, (image.cpu().numpy() if as_np else image)


def img_params_lq(img, size=2048):
    """``img_params_lq.m``: the image of ``img_params`` without the statistics table."""
    size = _check_size("img_params_lq", size)
    _one_image("img_params_lq", img)
    xd, as_np = _images(img)
    small = box_resize(xd, size)
    image = _scale_device(small, _stats_device(small))[0]
    return image.cpu().numpy() if as_np else image


def harvest(images, size=2048, freq=False):
    """An iterable of raw images ``[H,W]`` of differing shapes -> ``(stack, stats)``: the float32 ``[N,size,size,1]`` stack of
    ``img_params`` images (numpy: ready for ``input_pipeline.write_tfrecord``) and the list of their statistics dicts (with the
    ``*Freq2048`` fields if freq)."""
    size = _check_size("harvest", size)
    if freq:
        _check_fft_size("harvest", size)
    out, table = [], []
    for img in images:
        stats, image = img_params(img, size, freq)
        table.append(stats)
        out.append(image if isinstance(image, np.ndarray) else image.cpu().numpy())
    stack = np.stack(out)[..., None] if out else np.empty((0, size, size, 1), np.float32)
    return stack, table
