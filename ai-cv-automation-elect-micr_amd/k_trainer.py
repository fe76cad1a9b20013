"""Graph K training: the trainer of the learned D4-symmetric-kernel denoiser (misc_py/noise-removal-kernels.py:602-718).

What the reference does per step (``main``, :657-705): draw a batch of 10 x 10 crops through its host input path
(``record_parser``, :450-538), run every filter of ``architectures`` (:360-431) on it, and take one step of each filter's own
AdamOptimizer on its own MSE loss (:435-446) at lr = 0.005 (1 - t / 20001); every ``val_skip_n`` steps it reports the losses
on a validation batch; at the end ``saver.save`` writes a TF checkpoint (:717).

Here each step is, per filter, one forward + backward launch and one reduce + Adam launch of csrc/k_train.hip
(emd_k_train_step_f32); the crops come from a device-resident image stack through emd_k_sample_crops_f32.  The only host reads
are the per-step losses, once per chunk of steps.  ``k_record_parser`` restates the host input path in numpy (the check of the
device sampler).

Paired training (misc_py/noise_removal_kernels_duplicate.py, fed by misc_py/autoencoder_train-val-test.py): ``train_step_pair`` /
``train_pairs`` train the same filters to turn one patch into another (emd_k_train_pair_step_f32), ``make_pairs`` cuts the patch
pairs from two aligned stacks (emd_k_make_pairs_f32) and ``distill`` makes them from a trained autoencoder and its input crops.
``PAIR_PRESET`` holds the reference's settings for that trainer.
"""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np

from . import _lib, tf_checkpoint
from .kernel_denoiser import KernelParams, sym_pairs

EMD_K_LOSS_REFERENCE = 0
EMD_K_LOSS_IMAGE = 1
EMD_K_TRAIN_UPDATE = 1
EMD_K_TRAIN_LOSS_ONLY = 2
EMD_K_TRAIN_SQRT_ABOVE_1 = 4
EMD_K_PAD_REFLECT = 0
EMD_K_PAD_VALID = 1
PADS = {"reflect": EMD_K_PAD_REFLECT, "valid": EMD_K_PAD_VALID}
FUSED_MAX_STEPS = 1000      # EMD_K_FUSED_MAX_STEPS: steps per fused launch
FUSED_MAX_PIXELS = 8192     # EMD_K_FUSED_MAX_PIXELS: batch_size * crop^2 held in LDS by the fused launch
LOSSES = {"reference": EMD_K_LOSS_REFERENCE, "image": EMD_K_LOSS_IMAGE}
MAX_WIDTH, MAX_DEPTH = 15, 5
VAL_SKIP_N = 10          # noise-removal-kernels.py:89
VAL_SEED_XOR = 0x76616C  # the validation crops' Philox key: the seed with this mixed in ("val")
# The paired trainer's settings (noise_removal_kernels_duplicate.py): lr = 0.01 (1 - t / 10001) over 10 000 steps (:720-724), Adam
# at beta1 = 0.5 (:449), depth-1 filters of width 3, 5 and 7 (:87-88).  KernelDenoiserTrainer(**PAIR_PRESET) is that trainer; its
# patches are PAIR_PATCH = 20 pixels (:74), one pair per step (:54).
PAIR_PRESET = {"configs": ((1, 3), (1, 5), (1, 7)), "lr0": 0.01, "total_steps": 10000, "beta1": 0.5}
PAIR_PATCH = 20
PAIR_TEACHER_CROP = 160  # autoencoder_train-val-test.py:36


# ---- the host input path (noise-removal-kernels.py:450-538) -----------------------------------------------------------
def k_flip_rotate(img, choice: int):
    """flip_rotate (:498-515): the 8 elements of D4, selected by ``choice`` in 0..7."""
    if choice == 0:
        return img
    if choice in (1, 2, 3):
        return np.rot90(img, choice)
    if choice == 4:
        return np.flip(img, 0)
    if choice == 5:
        return np.flip(img, 1)
    if choice == 6:
        return np.flip(np.rot90(img, 1), 0)
    if choice == 7:
        return np.flip(np.rot90(img, 1), 1)
    raise ValueError("choice must be 0..7")


def k_preprocess(img):
    """preprocess (:517-529): NaN / Inf -> 0, scale0to1 (a constant crop -> 0.5), divide by the mean."""
    img = np.array(img, dtype=np.float32, copy=True)
    img[np.isnan(img)] = 0.0
    img[np.isinf(img)] = 0.0
    lo, hi = np.min(img), np.max(img)
    if lo == hi:
        img.fill(0.5)
    else:
        img = ((img - lo) / (hi - lo)).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        img /= np.mean(img)
    return img.astype(np.float32)


def k_crop(img, x: int, y: int, choice: int, crop: int):
    """The crop of load_image at (x, y), then flip_rotate(choice), preprocess and record_parser's finiteness check."""
    img = np.asarray(img, dtype=np.float32)
    img = img.reshape(img.shape[0], img.shape[1])
    out = k_preprocess(k_flip_rotate(img[x:x + crop, y:y + crop], choice))
    if np.sum(np.isfinite(out)) != crop * crop:   # record_parser (:534-535)
        out = np.zeros((crop, crop), np.float32)
    return out


def k_record_parser(img, rng, crop: int = 10):
    """record_parser(load_image) of the reference (:457-538) for one [H,W(,1)] image: draws x = randint(0, H - crop),
    y = randint(0, W - crop) and the D4 element from ``rng`` (numpy Generator), in that order.  H and W must exceed crop."""
    img = np.asarray(img, dtype=np.float32)
    H, W = img.shape[0], img.shape[1]
    if H <= crop or W <= crop:
        raise ValueError(f"crop {crop} needs an image larger than it, got {H}x{W}")
    x = int(rng.integers(0, H - crop))
    y = int(rng.integers(0, W - crop))
    choice = int(rng.integers(0, 8))
    return k_crop(img, x, y, choice, crop)



def s_crop(img, x: int, y: int, choice: int, crop: int = 160):
    """Graph S's crop (misc_py/autoencoder.py:190-274): the crop of load_image at (x, y), flip_rotate(choice), preprocess -- the
    steps of k_crop -- but a crop with any non-finite value afterwards becomes ONES (:271-272), where K's becomes zeros."""
    img = np.asarray(img, dtype=np.float32)
    img = img.reshape(img.shape[0], img.shape[1])
    out = k_preprocess(k_flip_rotate(img[x:x + crop, y:y + crop], choice))
    if np.sum(np.isfinite(out)) != crop * crop:
        out = np.ones((crop, crop), np.float32)
    return out


def s_record_parser(img, rng, crop: int = 160):
    """Graph S's host input path for one [H,W(,1)] image: draws x = randint(0, H - crop), y = randint(0, W - crop) and the D4
    element from ``rng`` (numpy Generator), in that order (autoencoder.py:190-233), then s_crop."""
    img = np.asarray(img, dtype=np.float32)
    H, W = img.shape[0], img.shape[1]
    if H <= crop or W <= crop:
        raise ValueError(f"crop {crop} needs an image larger than it, got {H}x{W}")
    x = int(rng.integers(0, H - crop))
    y = int(rng.integers(0, W - crop))
    choice = int(rng.integers(0, 8))
    return s_crop(img, x, y, choice, crop)

# ---- schedule and parameter vectors -------------------------------------------------------------------------------------
def lr_schedule(t: int, lr0: float = 0.005, total_steps: int = 20000) -> float:
    """:665-669: lr = lr0 (1 - t / (total_steps + 1)) for the 1-based step t."""
    return lr0 * (1.0 - t / (total_steps + 1))


def adam_lr_t(lr: float, t: int, beta1: float = 0.9, beta2: float = 0.999) -> float:
    """TF AdamOptimizer's bias-corrected step size lr sqrt(1 - beta2^t) / (1 - beta1^t)."""
    return lr * (1.0 - beta2 ** t) ** 0.5 / (1.0 - beta1 ** t)


def check_config(depth: int, width: int):
    if not (isinstance(depth, (int, np.integer)) and 1 <= depth <= MAX_DEPTH):
        raise ValueError(f"depth must be 1..{MAX_DEPTH}, got {depth}")
    if not (isinstance(width, (int, np.integer)) and width % 2 == 1 and 3 <= width <= MAX_WIDTH):
        raise ValueError(f"width must be odd and 3..{MAX_WIDTH}, got {width}")


def scalar_count(depth: int, width: int) -> int:
    n = len(sym_pairs(width))
    return (2 * depth - 1) * n + depth - 1


def theta_from_params(p: KernelParams) -> np.ndarray:
    """Full D4-symmetric maps -> the make_layer scalar vector [w (depth x nsym) | b1.. | s1..] of emd_k_train_step_f32."""
    if not p.symmetric:
        raise ValueError("K training needs D4-symmetric maps (make_layer's parameterisation)")
    o = p.width // 2
    idx = [(o + x, o + y) for (x, y) in sym_pairs(p.width)]
    w = [p.wmaps[l][tuple(np.array(idx).T)] for l in range(p.depth)]
    b = [p.bmaps[l][tuple(np.array(idx).T)] for l in range(1, p.depth)]
    return np.concatenate(w + b + [p.s[1:]]).astype(np.float32)


def params_from_theta(theta, depth: int, width: int) -> KernelParams:
    n = len(sym_pairs(width))
    theta = np.asarray(theta, np.float32)
    ws = [theta[l * n:(l + 1) * n] for l in range(depth)]
    bs = [np.zeros(n, np.float32)] + [theta[depth * n + (l - 1) * n: depth * n + l * n] for l in range(1, depth)]
    s = np.concatenate([[1.0], theta[(2 * depth - 1) * n:]]).astype(np.float32)
    return KernelParams.from_symmetric(ws, bs, s, width)


def initial_params(depth: int, width: int, rng) -> KernelParams:
    """The reference's initial values: weights 1/w^2, biases 0 (:109-112); the fully_connected scalars are TF's default
    glorot-uniform for a [1,1] weight, U(-sqrt(3), sqrt(3)) (weights_initializer=None, :391-396), drawn from ``rng``."""
    p = KernelParams.initial(depth, width)
    s = p.s.copy()
    for l in range(1, depth):
        s[l] = np.float32(rng.uniform(-np.sqrt(3.0), np.sqrt(3.0)))
    return KernelParams(p.wmaps, p.bmaps, s)


def tf_names(depth: int, width: int):
    """The TF variable names of theta's entries, in theta's order (scope depth-{d}_size-{w}, :365-405)."""
    scope = f"depth-{depth}_size-{width}"
    pairs = sym_pairs(width)
    names = [f"{scope}/w{l}/var_x-{x}_y-{y}/v" for l in range(depth) for (x, y) in pairs]
    names += [f"{scope}/b{l}/var_x-{x}_y-{y}/v" for l in range(1, depth) for (x, y) in pairs]
    names += [f"{scope}/fully_connected/weights" if l == 1 else f"{scope}/fully_connected_{l - 1}/weights" for l in range(1, depth)]
    return names


def tf_shape(name: str):
    return (1, 1) if name.endswith("/weights") else (1,)


def _beta_power_names(i: int):
    sfx = "" if i == 0 else f"_{i}"
    return f"beta1_power{sfx}", f"beta2_power{sfx}"


def step_from_beta_powers(beta1_power: float, beta2_power: float, beta1: float = 0.9, beta2: float = 0.999):
    """Adam's step count t from the saved float32 beta1^t / beta2^t (the beta2 power, which decays slowest, decides; the
    beta1 power must agree where it is still a normal float32).  None when both have underflowed."""
    tiny = float(np.finfo(np.float32).tiny)
    cands = [(p, b) for p, b in ((beta2_power, beta2), (beta1_power, beta1)) if p >= tiny and 0.0 < b < 1.0]
    if not cands:
        return None
    if any(p > 1.0 for p, _ in cands):
        raise ValueError("beta power above 1")
    t = int(round(np.log(cands[0][0]) / np.log(cands[0][1])))
    for p, b in cands[1:]:
        if abs(np.log(p) / np.log(b) - t) > 0.5:
            raise ValueError(f"beta powers disagree on the step count ({t} vs {np.log(p) / np.log(b):.2f})")
    return t


def kernel_state_dict(filters, step: int, beta1: float = 0.9, beta2: float = 0.999):
    """The checkpoint tensors of filters [(depth, width, theta, adam_m, adam_v)] after ``step`` Adam steps, under the names
    tf.train.Saver gives the reference's variables: the trainables, Adam's ``<var>/Adam`` and ``<var>/Adam_1`` slots, and
    beta1_power / beta2_power (suffixed _1, _2 .. for the optimizers of the second, third .. filter)."""
    out = {}
    for i, (depth, width, theta, m, v) in enumerate(filters):
        theta, m, v = (np.asarray(a, np.float32).reshape(-1) for a in (theta, m, v))
        for k, name in enumerate(tf_names(depth, width)):
            shp = tf_shape(name)
            out[name] = np.full(shp, theta[k], np.float32)
            out[name + "/Adam"] = np.full(shp, m[k], np.float32)
            out[name + "/Adam_1"] = np.full(shp, v[k], np.float32)
        b1, b2 = _beta_power_names(i)
        out[b1] = np.float32(beta1 ** step)
        out[b2] = np.float32(beta2 ** step)
    return out


# ---- device entry points ----------------------------------------------------------------------------------------------
def _as_batch(batch, device):
    """host or device [B,H,W(,1)] -> contiguous float32 CUDA [B,H,W]."""
    import torch

    x = batch if isinstance(batch, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(batch, dtype=np.float32))
    if x.dim() == 4:
        if x.shape[3] != 1:
            raise ValueError("channel dimension must be 1")
        x = x[..., 0]
    if x.dim() != 3:
        raise ValueError("expected a [B,H,W] or [B,H,W,1] batch")
    return x.to(device=device, dtype=torch.float32).contiguous()


def sample_crops(stack_dev, B: int, crop: int, seed: int, first_index: int, out=None, draws=None, stream=None):
    """emd_k_sample_crops_f32: B preprocessed crop x crop crops of the device stack [N,H,W]; draws (int32 [B,4] CUDA tensor or
    None) receives (image, x, y, D4 element) per crop."""
    import torch

    N, H, W = stack_dev.shape
    if out is None:
        out = torch.empty((B, crop, crop), dtype=torch.float32, device=stack_dev.device)
    rc = _lib.load().emd_k_sample_crops_f32(_lib.ptr(stack_dev), N, H, W, _lib.ptr(out), B, crop,
                                            C.c_ulonglong(int(seed) & 0xFFFFFFFFFFFFFFFF), C.c_ulonglong(int(first_index)),
                                            _lib.ptr(draws) if draws is not None else None, _lib.stream_ptr(stream))
    _lib.check(rc, "emd_k_sample_crops_f32")
    return out


def check_pair_window(S: int, patch: int, lo: int, hi):
    """The offset window [lo, hi) of make_pairs on images of side S; hi = None is the reference's S - 2 * patch
    (randint(20, 160 - 20 - 20), autoencoder_train-val-test.py:51-52).  Returns hi."""
    if hi is None:
        hi = S - 2 * patch
    if patch < 1 or lo < 0:
        raise ValueError(f"bad patch / lo ({patch}, {lo})")
    if hi <= lo:
        raise ValueError(f"the offset window [{lo}, {hi}) is empty")
    if hi - 1 + patch > S:
        raise ValueError(f"a {patch}-px patch at offset {hi - 1} does not fit a {S}-px image")
    return int(hi)


def make_pairs(a, b, patch: int = PAIR_PATCH, lo: int = 20, hi=None, seed: int = 0, first_index: int = 0, return_draws: bool = False,
               device=None, stream=None):
    """emd_k_make_pairs_f32: autoencoder_train-val-test.py:35-55 for two aligned stacks a, b [N,H,W] (host or device): each image
    rescaled by (img - min) / (mean - min), one patch x patch window per pair at offsets (i, j) uniform in [lo, hi) (Philox, keyed
    by ``seed``, pair n at counter first_index + n), both patches 0.5 where either holds a non-finite value.
    Returns (x, t) CUDA float32 [N,patch,patch], and the draws (int32 [N,2]) with ``return_draws``."""
    import torch

    if device is None:
        device = a.device if isinstance(a, torch.Tensor) and a.is_cuda else torch.device("cuda", torch.cuda.current_device())
    a, b = _as_batch(a, device), _as_batch(b, device)
    if a.shape != b.shape:
        raise ValueError(f"the two stacks differ in shape: {tuple(a.shape)} and {tuple(b.shape)}")
    N, H, W = a.shape
    hi = check_pair_window(min(H, W), patch, lo, hi)
    x = torch.empty((N, patch, patch), dtype=torch.float32, device=device)
    t = torch.empty_like(x)
    draws = torch.empty((N, 2), dtype=torch.int32, device=device) if return_draws else None
    rc = _lib.load().emd_k_make_pairs_f32(_lib.ptr(a), _lib.ptr(b), N, H, W, patch, lo, hi, C.c_ulonglong(int(seed) & 0xFFFFFFFFFFFFFFFF),
                                          C.c_ulonglong(int(first_index)), _lib.ptr(x), _lib.ptr(t),
                                          _lib.ptr(draws) if draws is not None else None, _lib.stream_ptr(stream))
    _lib.check(rc, "emd_k_make_pairs_f32")
    return (x, t, draws) if return_draws else (x, t)


def teacher_crops(teacher, stack, max_batch: int = 64):
    """The first half of ``distill``: (crops, outputs), both CUDA float32 [N,160,160].  crops = stack[:, :160, :160]; outputs[n] is
    ``teacher.denoise_crop(crops[n])`` at its default arguments, computed on the device in batches of ``max_batch``: the crop's
    rescale by (min, mean - min) (emd_tile_gather_f32), preprocess on the result (emd_tile_prep_f32, EMD_TILE_PREP_S, per crop),
    the engine, and the inverse map with denoise_crop's flat-crop branch (emd_s_crop_unscale_f32)."""
    import torch

    from . import tiling

    if max_batch < 1:
        raise ValueError("max_batch must be >= 1")
    cs = teacher.cropsize
    src = _as_batch(stack, teacher.device)
    N, H, W = src.shape
    if H < cs or W < cs:
        raise ValueError(f"distill needs images of at least {cs}x{cs}, got {H}x{W}")
    crops = src[:, :cs, :cs].contiguous()   # img[:160, :160] (autoencoder_train-val-test.py:36)
    plan = tiling.TilePlan(cs, cs, cs, 0, 0, [0], [0])   # one tile per image: the crop itself
    keep, dev_plan = plan.device_arrays(src.device)
    net_in = torch.empty((N, cs, cs), dtype=torch.float32, device=src.device)
    cstats = torch.empty((N, 2), dtype=torch.float32, device=src.device)
    for g0 in range(0, N, tiling._MAX_TILES_PER_LAUNCH):
        n = min(tiling._MAX_TILES_PER_LAUNCH, N - g0)
        tiling.gather(crops, plan, dev_plan, g0, n, net_in[g0:g0 + n], cstats[g0:g0 + n])
    net_in, _ = tiling.prepare(net_in, tiling.PREP_S)
    preds = torch.empty((N, cs, cs), dtype=torch.float32, device=src.device)
    for t0 in range(0, N, max_batch):
        n = min(max_batch, N - t0)
        preds[t0:t0 + n] = teacher.engine.forward(net_in[t0:t0 + n, :, :, None])[..., 0]
    rc = _lib.load().emd_s_crop_unscale_f32(_lib.ptr(preds), _lib.ptr(cstats), N, cs * cs, _lib.ptr(preds), _lib.stream_ptr())
    _lib.check(rc, "emd_s_crop_unscale_f32")
    del keep
    return crops, preds


def distill(teacher, stack, patch: int = PAIR_PATCH, lo: int = 20, hi=None, seed: int = 0, first_index: int = 0,
            max_batch: int = 64, return_draws: bool = False):
    """autoencoder_train-val-test.py as one device pass: the training pairs of the paired K trainer from a trained autoencoder.
    ``teacher`` is an autoencoder.Micrograph_Autoencoder, ``stack`` [N,H,W(,1)] with H, W >= 160 (host or device).  Every image's
    160 x 160 corner goes through the teacher (teacher_crops), then make_pairs cuts one patch pair per image.  Returns make_pairs'
    result: (x, t) with x the input's patch and t the teacher's.  Nothing returns to the host in between.  Unlike the script, the
    whole stack is processed (it stops after 6076 pairs) and errors are raised (it swallows them)."""
    cs = teacher.cropsize
    check_pair_window(cs, patch, lo, hi)
    crops, preds = teacher_crops(teacher, stack, max_batch)
    return make_pairs(crops, preds, patch, lo, hi, seed, first_index, return_draws, device=teacher.device)


def pair_order(n_pairs: int, start: int, steps: int, batch_size: int = 1):
    """The pair indices train_pairs feeds: step k (0-based, counted from ``start`` completed steps) takes pairs
    ((start + k) * batch_size + b) % n_pairs, b = 0..batch_size-1 -- the stacks in stored order, wrapping round
    (Dataset.zip(...).repeat().batch(), noise_removal_kernels_duplicate.py:561-590)."""
    k = (start + np.arange(steps, dtype=np.int64))[:, None] * batch_size + np.arange(batch_size, dtype=np.int64)[None]
    return k % n_pairs


class _Filter:
    """Device state of one (depth, width) filter: theta, Adam's m and v, the step counter and the packed inference block."""

    def __init__(self, depth, width, params: KernelParams, device):
        import torch

        self.depth, self.width = depth, width
        self.n = scalar_count(depth, width)
        self.theta = torch.from_numpy(theta_from_params(params)).to(device)
        self.m = torch.zeros(self.n, dtype=torch.float32, device=device)
        self.v = torch.zeros(self.n, dtype=torch.float32, device=device)
        self.step = torch.zeros(1, dtype=torch.int32, device=device)
        self.packed = torch.from_numpy(params.packed()).to(device)


class KernelDenoiserTrainer:
    """Trains one or more (depth, width) filters of graph K, each with its own loss and its own Adam, on the same batches
    (architectures' depths x widths loop, :360-363; experiment(), :433-446).

    configs      (depth, width) pairs, depth 1..5, width odd 3..15.
    loss         "reference": mean((F(x)^T - x)^2), what the reference minimises (its output is assembled transposed,
                 :421-424, and compared with the input, :438; square crops); "image": mean((F(x) - x)^2).
    lr0, total_steps: lr = lr0 (1 - t / (total_steps + 1)) at the 1-based step t (:665-669).
    initial      optional {(depth, width): KernelParams} (or a list in configs' order) of D4-symmetric starting maps; the
                 default is the reference's initialisation with the fully_connected scalars drawn from a generator seeded
                 by ``seed`` (initial_params).
    seed         also keys the Philox stream of train()'s device crop sampler."""

    def __init__(self, configs=((2, 3),), device=None, seed: int = 0, lr0: float = 0.005, total_steps: int = 20000,
                 loss: str = "reference", initial=None, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8):
        configs = [tuple(int(v) for v in c) for c in configs]
        if not configs:
            raise ValueError("no (depth, width) configs")
        for d, w in configs:
            check_config(d, w)
        if len(set(configs)) != len(configs):
            raise ValueError("duplicate (depth, width) config")
        if loss not in LOSSES:
            raise ValueError(f"loss must be one of {sorted(LOSSES)}")
        if total_steps < 1 or lr0 < 0:
            raise ValueError("bad learning-rate schedule")
        if isinstance(initial, (list, tuple)):
            initial = dict(zip(configs, initial))
        initial = initial or {}
        for c, p in initial.items():
            if (p.depth, p.width) != tuple(c):
                raise ValueError(f"initial params for {c} are {p.depth, p.width}")
        import torch

        self.configs, self.loss, self.loss_mode = configs, loss, LOSSES[loss]
        self.lr0, self.total_steps = float(lr0), int(total_steps)
        self.beta1, self.beta2, self.eps = float(beta1), float(beta2), float(eps)
        self.seed = int(seed)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.lib = _lib.load()
        rng = np.random.default_rng(self.seed)
        self.filters = []
        for c in configs:
            p = initial.get(c)
            if p is None:
                p = initial_params(c[0], c[1], rng)
            self.filters.append(_Filter(c[0], c[1], p, self.device))
        self.step = 0            # completed training steps (every filter's device counter holds the same)
        self._ws = {}
        self._loss_buf = torch.zeros(len(configs), dtype=torch.float32, device=self.device)

    # ---- one launch pair per filter
    def _workspace(self, f: _Filter, B, H, W):
        import torch

        key = (B, H, W, f.depth, f.width)
        if key not in self._ws:
            n = self.lib.emd_k_train_workspace_bytes(B, H, W, f.width, f.depth)
            self._ws[key] = torch.empty((n + 3) // 4, dtype=torch.float32, device=self.device)
        return self._ws[key]

    def _launch(self, f: _Filter, x, flags, loss_out, grad_out=None):
        B, H, W = x.shape
        ws = self._workspace(f, B, H, W)
        upd = flags & EMD_K_TRAIN_UPDATE
        rc = self.lib.emd_k_train_step_f32(
            _lib.ptr(x), B, H, W, f.width, f.depth, self.loss_mode, _lib.ptr(f.theta), _lib.ptr(f.m), _lib.ptr(f.v),
            _lib.ptr(f.step), C.c_double(self.lr0), self.total_steps, self.beta1, self.beta2, self.eps, flags,
            _lib.ptr(grad_out) if grad_out is not None else None, loss_out, _lib.ptr(f.packed) if upd else None,
            _lib.ptr(ws), ws.numel() * 4, _lib.stream_ptr())
        _lib.check(rc, "emd_k_train_step_f32")

    @staticmethod
    def _elem_ptr(t, i):
        return C.c_void_p(t.data_ptr() + 4 * i)

    def _check_batch(self, x):
        if self.loss_mode == EMD_K_LOSS_REFERENCE and x.shape[1] != x.shape[2]:
            raise ValueError('loss="reference" compares the transposed output with the input: square crops only')

    def train_step(self, batch):
        """One Adam step of every filter on ``batch`` (host or device [B,S,S(,1)]).  Returns the per-filter losses, computed
        with the parameters before the update (the loss and the train op share one sess.run, :678)."""
        x = _as_batch(batch, self.device)
        self._check_batch(x)
        self._check_steps(1)
        for i, f in enumerate(self.filters):
            self._launch(f, x, EMD_K_TRAIN_UPDATE, self._elem_ptr(self._loss_buf, i))
        self.step += 1
        return self._loss_buf.cpu().numpy().copy()

    def evaluate(self, batch):
        """Per-filter losses on ``batch`` with the current parameters (the validation pass, :689-705)."""
        x = _as_batch(batch, self.device)
        self._check_batch(x)
        for i, f in enumerate(self.filters):
            self._launch(f, x, EMD_K_TRAIN_LOSS_ONLY, self._elem_ptr(self._loss_buf, i))
        return self._loss_buf.cpu().numpy().copy()

    def loss_and_grad(self, batch, config=None):
        """(loss, dL/dtheta) of one filter on ``batch`` without updating it (theta's layout: emd_k_train_step_f32)."""
        import torch

        x = _as_batch(batch, self.device)
        self._check_batch(x)
        f = self._filter(config)
        g = torch.empty(f.n, dtype=torch.float32, device=self.device)
        self._launch(f, x, 0, self._elem_ptr(self._loss_buf, 0), grad_out=g)
        return float(self._loss_buf[0].item()), g.cpu().numpy()

    # ---- paired training (noise_removal_kernels_duplicate.py)
    def _launch_pair(self, f: _Filter, x, truth, pad_mode, flags, loss_out, grad_out=None):
        B, H, W = x.shape
        ws = self._workspace(f, B, H, W)
        upd = flags & EMD_K_TRAIN_UPDATE
        rc = self.lib.emd_k_train_pair_step_f32(
            _lib.ptr(x), _lib.ptr(truth), B, H, W, f.width, f.depth, pad_mode, _lib.ptr(f.theta), _lib.ptr(f.m), _lib.ptr(f.v),
            _lib.ptr(f.step), C.c_double(self.lr0), self.total_steps, self.beta1, self.beta2, self.eps, flags,
            _lib.ptr(grad_out) if grad_out is not None else None, loss_out, _lib.ptr(f.packed) if upd else None,
            _lib.ptr(ws), ws.numel() * 4, _lib.stream_ptr())
        _lib.check(rc, "emd_k_train_pair_step_f32")

    def _check_pair_shape(self, shape, pad, filters=None):
        """(pad mode) for [B,H,W] pair batches; every filter trained on them must fit."""
        if pad not in PADS:
            raise ValueError(f"pad must be one of {sorted(PADS)}")
        H, W = int(shape[1]), int(shape[2])
        for f in (self.filters if filters is None else filters):
            if pad == "valid" and f.width > min(H, W):
                raise ValueError(f'pad="valid" needs width <= min(H, W): width {f.width}, batch {H}x{W}')
            if pad == "reflect" and f.width // 2 >= min(H, W):
                raise ValueError(f'pad="reflect" needs width/2 < min(H, W): width {f.width}, batch {H}x{W}')
        return PADS[pad]

    def _as_pair(self, x, truth, pad, filters=None):
        x, truth = _as_batch(x, self.device), _as_batch(truth, self.device)
        if x.shape != truth.shape:
            raise ValueError(f"x and truth differ in shape: {tuple(x.shape)} and {tuple(truth.shape)}")
        return x, truth, self._check_pair_shape(x.shape, pad, filters)

    def train_step_pair(self, x, truth, pad: str = "valid", sqrt_above_1: bool = True):
        """One Adam step of every filter towards ``truth`` from ``x`` (both host or device [B,H,W(,1)]).  pad "valid": each filter
        is evaluated on its own (H-w+1) x (W-w+1) interior and compared with the same interior of ``truth``
        (noise_removal_kernels_duplicate.py:406-432); "reflect": the unpaired trainer's border, H x W outputs.
        sqrt_above_1: the loss is sqrt(MSE) while the MSE exceeds 1 (:433).  Returns the per-filter losses, computed with the
        parameters before the update."""
        x, truth, pm = self._as_pair(x, truth, pad)
        self._check_steps(1)
        flags = EMD_K_TRAIN_UPDATE | (EMD_K_TRAIN_SQRT_ABOVE_1 if sqrt_above_1 else 0)
        for i, f in enumerate(self.filters):
            self._launch_pair(f, x, truth, pm, flags, self._elem_ptr(self._loss_buf, i))
        self.step += 1
        return self._loss_buf.cpu().numpy().copy()

    def evaluate_pair(self, x, truth, pad: str = "valid", sqrt_above_1: bool = True):
        """Per-filter paired losses on (x, truth) with the current parameters."""
        x, truth, pm = self._as_pair(x, truth, pad)
        flags = EMD_K_TRAIN_LOSS_ONLY | (EMD_K_TRAIN_SQRT_ABOVE_1 if sqrt_above_1 else 0)
        for i, f in enumerate(self.filters):
            self._launch_pair(f, x, truth, pm, flags, self._elem_ptr(self._loss_buf, i))
        return self._loss_buf.cpu().numpy().copy()

    def loss_and_grad_pair(self, x, truth, config=None, pad: str = "valid", sqrt_above_1: bool = True):
        """(loss, dL/dtheta) of one filter on the pair batch without updating it (theta's layout: emd_k_train_step_f32)."""
        import torch

        f = self._filter(config)
        x, truth, pm = self._as_pair(x, truth, pad, [f])
        g = torch.empty(f.n, dtype=torch.float32, device=self.device)
        self._launch_pair(f, x, truth, pm, EMD_K_TRAIN_SQRT_ABOVE_1 if sqrt_above_1 else 0, self._elem_ptr(self._loss_buf, 0),
                          grad_out=g)
        return float(self._loss_buf[0].item()), g.cpu().numpy()

    def _pair_step(self, x, truth, pad_mode, flags, buf, k):
        """One paired step of every filter on device batches; the losses go to row k of buf.  (train_pairs' only device work.)"""
        nf = len(self.filters)
        for i, f in enumerate(self.filters):
            self._launch_pair(f, x, truth, pad_mode, flags, self._elem_ptr(buf, k * nf + i))

    def train_pairs(self, x_stack, t_stack, steps: int, batch_size: int = 1, shuffle: bool = False, pad: str = "valid",
                    sqrt_above_1: bool = True, val_x=None, val_t=None, val_skip_n: int = VAL_SKIP_N, chunk: int = 1000,
                    save_every: int = 0, directory=None):
        """``steps`` paired steps over two aligned stacks [N,p,p(,1)] (host or device), x_stack the inputs and t_stack the targets,
        as make_pairs / distill return them.  The pairs are used as stored, in order, wrapping round (pair_order; the reference
        zips two sorted file lists, repeats, and takes one pair per step, noise_removal_kernels_duplicate.py:54, :561-590; its
        flip_rotate is pinned to the identity, :460, and its random crop is commented out, :485-488, so there is no augmentation).
        shuffle: one permutation of the pairs, drawn from a generator seeded by the trainer's seed, replaces the stored order.
        val_x / val_t: an optional validation pair stack, evaluated whole after every ``val_skip_n``-th step (the reference has
        its validation commented out).  save_every > 0 writes a checkpoint to ``directory`` whenever the step count reaches a
        multiple of it (the reference: every 5000 steps, :784-785).  The device is read once per ``chunk`` steps.
        Returns {"loss": [steps, configs], "val_step": [k], "val_loss": [k, configs]}."""
        import torch

        if steps < 0 or batch_size < 1 or chunk < 1:
            raise ValueError("bad steps / batch_size / chunk")
        if val_skip_n < 1:
            raise ValueError("val_skip_n must be >= 1")
        if save_every < 0 or (save_every and directory is None):
            raise ValueError("save_every needs a directory")
        if (val_x is None) != (val_t is None):
            raise ValueError("val_x and val_t come together")
        n_x, n_t = len(x_stack), len(t_stack)
        if n_x != n_t:
            raise ValueError(f"the stacks hold {n_x} and {n_t} pairs")
        if n_x < 1:
            raise ValueError("no pairs")
        self._check_steps(steps)
        xs, ts, pm = self._as_pair(x_stack, t_stack, pad)
        val = self._as_pair(val_x, val_t, pad)[:2] if val_x is not None else None
        nf = len(self.filters)
        flags = EMD_K_TRAIN_UPDATE | (EMD_K_TRAIN_SQRT_ABOVE_1 if sqrt_above_1 else 0)
        vflags = EMD_K_TRAIN_LOSS_ONLY | (EMD_K_TRAIN_SQRT_ABOVE_1 if sqrt_above_1 else 0)
        if shuffle:
            perm = torch.from_numpy(np.random.default_rng(self.seed).permutation(n_x)).to(self.device)
            xs, ts = xs[perm].contiguous(), ts[perm].contiguous()
        losses, val_steps, val_losses = [], [], []
        done = 0
        while done < steps:
            n = min(chunk, steps - done)
            order = pair_order(n_x, self.step, n, batch_size)
            buf = torch.empty((n, nf), dtype=torch.float32, device=self.device)
            vbuf = torch.empty((n // val_skip_n + 1, nf), dtype=torch.float32, device=self.device)
            nval = 0
            for k in range(n):
                first = int(order[k, 0])
                if first + batch_size <= n_x:   # a contiguous run of the stacks: no copy
                    xb, tb = xs[first:first + batch_size], ts[first:first + batch_size]
                else:                           # the batch wraps round the end
                    idx = torch.from_numpy(order[k]).to(self.device)
                    xb, tb = xs[idx].contiguous(), ts[idx].contiguous()
                self._pair_step(xb, tb, pm, flags, buf, k)
                self.step += 1
                if val is not None and self.step % val_skip_n == 0:
                    self._pair_step(val[0], val[1], pm, vflags, vbuf, nval)
                    val_steps.append(self.step)
                    nval += 1
                if save_every and self.step % save_every == 0:
                    self.save_checkpoint(directory)
            losses.append(buf.cpu().numpy())
            if nval:
                val_losses.append(vbuf[:nval].cpu().numpy())
            done += n
        return {"loss": np.concatenate(losses) if losses else np.zeros((0, nf), np.float32),
                "val_step": np.asarray(val_steps, np.int64),
                "val_loss": np.concatenate(val_losses) if val_losses else np.zeros((0, nf), np.float32)}

    def _check_steps(self, steps):
        if self.step + steps > self.total_steps:
            raise ValueError(f"{self.step} + {steps} steps run past total_steps={self.total_steps}: the learning rate "
                             "lr0 (1 - t / (total_steps + 1)) would turn negative")

    @staticmethod
    def fused_allowed(batch_size: int, crop: int) -> bool:
        """The fused launch keeps the batch in LDS: batch_size * crop^2 <= EMD_K_FUSED_MAX_PIXELS (32 KiB)."""
        return batch_size * crop * crop <= FUSED_MAX_PIXELS

    def _fused(self, nsteps, losses, B, crop, src=None, batches=None, nbatches=0):
        """emd_k_train_fused_f32 over every filter; losses: CUDA float32 [configs, >= nsteps] (row i = filter i)."""
        jobs = (_lib.KFusedJob * len(self.filters))()
        for i, f in enumerate(self.filters):
            jobs[i] = _lib.KFusedJob(f.theta.data_ptr(), f.m.data_ptr(), f.v.data_ptr(), f.step.data_ptr(), f.packed.data_ptr(),
                                     losses[i].data_ptr(), f.width, f.depth)
        N, H, W = src.shape if src is not None else (0, 0, 0)
        rc = self.lib.emd_k_train_fused_f32(jobs, len(self.filters), _lib.ptr(src) if src is not None else None, N, H, W,
                                            _lib.ptr(batches) if batches is not None else None, nbatches, B, crop,
                                            C.c_ulonglong(self.seed & 0xFFFFFFFFFFFFFFFF), nsteps, self.loss_mode,
                                            C.c_double(self.lr0), self.total_steps, self.beta1, self.beta2, self.eps,
                                            _lib.stream_ptr())
        _lib.check(rc, "emd_k_train_fused_f32")
        self.step += nsteps

    def train_fused(self, batches, steps: int):
        """``steps`` steps of the fused launch on fixed batches (host or device [nb,B,S,S]; step k uses batch k % nb), as
        train_step(batches[k % nb]) would take them.  Returns the losses [steps, configs]."""
        import torch

        x = batches if isinstance(batches, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(batches, dtype=np.float32))
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        if x.dim() != 4 or x.shape[2] != x.shape[3]:
            raise ValueError("expected [nbatches, B, S, S] batches")
        nb, B, S = x.shape[0], x.shape[1], x.shape[2]
        if not self.fused_allowed(B, S):
            raise ValueError(f"a [{B},{S},{S}] batch does not fit the fused launch's LDS budget")
        self._check_steps(steps)
        out = []
        done = 0
        while done < steps:
            n = min(FUSED_MAX_STEPS, steps - done)
            buf = torch.empty((len(self.filters), n), dtype=torch.float32, device=self.device)
            # the kernel cycles it % nb from its own step 0: hand it the batches rotated to where this call stands
            xs = torch.roll(x, -(done % nb), dims=0).contiguous() if done % nb else x
            self._fused(n, buf, B, S, batches=xs, nbatches=nb)
            out.append(buf.t().cpu().numpy())
            done += n
        return np.concatenate(out) if out else np.zeros((0, len(self.filters)), np.float32)

    def train(self, stack, steps: int, batch_size: int = 32, crop: int = 10, val_stack=None, val_skip_n: int = VAL_SKIP_N,
              chunk: int = 1000, fused: bool = False):
        """``steps`` training steps on crops sampled on the device from ``stack`` ([N,H,W(,1)], host or device; H, W > crop).
        Step t (counting every step this trainer has taken) draws crops b = 0..batch_size-1 from Philox(seed, t*B + b).
        Every ``val_skip_n``-th step a batch from ``val_stack`` is evaluated after the update.  The device is read once per
        ``chunk`` steps.  ``fused``: True runs the steps in fused launches (emd_k_train_fused_f32, up to 1 000 steps each, cut
        at every validation step; needs fused_allowed(batch_size, crop)), False (default) as sampler + step launches -- the
        fused form measured slower at the reference's [32,10,10], so it is opt-in.  Returns {"loss": [steps, configs], "val_step": [k], "val_loss": [k, configs]}."""
        import torch

        if steps < 0 or batch_size < 1 or chunk < 1:
            raise ValueError("bad steps / batch_size / chunk")
        if val_skip_n < 1:
            raise ValueError("val_skip_n must be >= 1")
        self._check_steps(steps)
        if fused and not self.fused_allowed(batch_size, crop):
            raise ValueError(f"a [{batch_size},{crop},{crop}] batch does not fit the fused launch's LDS budget")
        src = _as_batch(stack, self.device)
        val = _as_batch(val_stack, self.device) if val_stack is not None else None
        for s in (src, val):
            if s is not None and (s.shape[1] <= crop or s.shape[2] <= crop):
                raise ValueError(f"crop {crop} needs images larger than it, got {tuple(s.shape[1:])}")
        nf = len(self.filters)
        crops = torch.empty((batch_size, crop, crop), dtype=torch.float32, device=self.device)
        vcrops = torch.empty_like(crops) if val is not None else None
        losses, val_steps, val_losses = [], [], []

        def validate(vbuf, nval):
            sample_crops(val, batch_size, crop, self.seed ^ VAL_SEED_XOR, (self.step - 1) * batch_size, out=vcrops)
            for i, f in enumerate(self.filters):
                self._launch(f, vcrops, EMD_K_TRAIN_LOSS_ONLY, self._elem_ptr(vbuf, nval * nf + i))
            val_steps.append(self.step)

        done = 0
        while done < steps:
            n = min(chunk, steps - done)
            nval = 0
            vbuf = torch.empty((n // val_skip_n + 1, nf), dtype=torch.float32, device=self.device)
            if fused:
                buf = torch.empty((nf, n), dtype=torch.float32, device=self.device)
                k = 0
                while k < n:
                    seg = min(n - k, FUSED_MAX_STEPS)
                    if val is not None:   # stop at the next validation step
                        seg = min(seg, val_skip_n - self.step % val_skip_n)
                    self._fused(seg, buf[:, k:], batch_size, crop, src=src)
                    k += seg
                    if val is not None and self.step % val_skip_n == 0:
                        validate(vbuf, nval)
                        nval += 1
                losses.append(buf.t().cpu().numpy())
            else:
                buf = torch.empty((n, nf), dtype=torch.float32, device=self.device)
                for k in range(n):
                    sample_crops(src, batch_size, crop, self.seed, self.step * batch_size, out=crops)
                    for i, f in enumerate(self.filters):
                        self._launch(f, crops, EMD_K_TRAIN_UPDATE, self._elem_ptr(buf, k * nf + i))
                    self.step += 1
                    if val is not None and self.step % val_skip_n == 0:
                        validate(vbuf, nval)
                        nval += 1
                losses.append(buf.cpu().numpy())
            if nval:
                val_losses.append(vbuf[:nval].cpu().numpy())
            done += n
        return {"loss": np.concatenate(losses) if losses else np.zeros((0, nf), np.float32),
                "val_step": np.asarray(val_steps, np.int64),
                "val_loss": np.concatenate(val_losses) if val_losses else np.zeros((0, nf), np.float32)}

    # ---- parameters and checkpoints
    def _filter(self, config=None) -> _Filter:
        if config is None:
            return self.filters[0]
        c = tuple(config)
        for f in self.filters:
            if (f.depth, f.width) == c:
                return f
        raise KeyError(f"no filter {c}")

    def params(self, config=None) -> KernelParams:
        """The current maps of one filter (default: the first config) as KernelParams."""
        f = self._filter(config)
        return params_from_theta(f.theta.cpu().numpy(), f.depth, f.width)

    def packed_params(self, config=None):
        """The device block emd_kernel_denoise_f32 consumes, kept current by every update (no host round trip)."""
        return self._filter(config).packed

    def state_dict(self):
        """name -> numpy array with the names tf.train.Saver gives the reference's variables (kernel_state_dict)."""
        return kernel_state_dict([(f.depth, f.width, *(a.cpu().numpy() for a in (f.theta, f.m, f.v))) for f in self.filters],
                                 self.step, self.beta1, self.beta2)

    def save_checkpoint(self, directory, global_step=None):
        """saver.save(sess, directory + "/", global_step) (:717): the bundle <directory>/-<global_step>.{index,data-*} and
        the ``checkpoint`` state file.  ``global_step`` must be the trainer's step count (the Adam state saved beside it, the
        beta powers, belongs to that step).  Returns the prefix."""
        step = self.step if global_step is None else int(global_step)
        if step != self.step:
            raise ValueError(f"global_step {step} is not the trainer's step count {self.step}: its Adam state would not match")
        prefix = os.path.join(directory, "") + f"-{step}"
        tf_checkpoint.write_checkpoint(prefix, self.state_dict())
        return prefix

    def restore(self, directory):
        """Resume from tf_checkpoint.latest_checkpoint(directory): parameters, Adam slots and the step count.  The step is
        read from the saved beta powers (Adam's bias correction) and checked against the ``-<global_step>`` suffix of the
        checkpoint name when there is one."""
        import torch

        prefix = tf_checkpoint.latest_checkpoint(directory)
        if prefix is None:
            raise FileNotFoundError(f"{directory}: no checkpoint")
        z = tf_checkpoint.read_checkpoint(prefix)
        m = re.search(r"-(\d+)$", prefix)
        named = int(m.group(1)) if m else None
        step = None
        for i, f in enumerate(self.filters):
            b1, b2 = _beta_power_names(i)
            t = step_from_beta_powers(float(np.asarray(z[b1]).reshape(-1)[0]), float(np.asarray(z[b2]).reshape(-1)[0]),
                                      self.beta1, self.beta2)
            if t is None:
                t = named
            if t is None:
                raise ValueError(f"{prefix}: the step count is neither in the beta powers nor in the name")
            if (named is not None and t != named) or (step is not None and t != step):
                raise ValueError(f"{prefix}: beta powers say step {t}, the checkpoint name / other filters say {named if step is None else step}")
            step = t
        for f in self.filters:
            names = tf_names(f.depth, f.width)
            get = lambda sfx: np.array([np.asarray(z[n + sfx]).reshape(-1)[0] for n in names], np.float32)
            theta, mm, vv = get(""), get("/Adam"), get("/Adam_1")
            f.theta.copy_(torch.from_numpy(theta))
            f.m.copy_(torch.from_numpy(mm))
            f.v.copy_(torch.from_numpy(vv))
            f.step.fill_(step)
            f.packed.copy_(torch.from_numpy(params_from_theta(theta, f.depth, f.width).packed()))
        self.step = step
        return prefix
