"""Graph S training: the trainer of the separable autoencoder that ``autoencoder.Micrograph_Autoencoder`` applies.

The reference trains it in misc_py/autoencoder.py (:83-188, :339-506) and loads the checkpoints in misc_py/apply_autoencoders.py
(:312-344).  What is trained here is the graph the apply side reads (apply_autoencoders.py:91-187, ``AutoencoderEngine``):
4 separable blocks (depthwise 3x3, strides 2/2/2/1, pointwise without bias to 64/128/256/encoding_features, normalizer BN, a second
BN, relu), transposed convs k3 s2 + bias to 256 and 128 (BN + relu), a third to 64 (relu), a 3x3 conv 64 -> 1 without bias.  Per step
(autoencoder.py:177-188, :427-431):

  * every batch norm on the statistics of the WHOLE batch (is_training=True, biased variance, eps 1e-3);
  * loss = tf.losses.mean_squared_error(x, out): the target is the input crop, the mean runs over B*H*W;
  * AdamOptimizer(lr) with beta1 0.9, beta2 0.999, eps 1e-8 and TF's bias-corrected lr_t, where
    lr = lr0 (1 - (t // period) / (total_steps // period))^1.5 at the 1-based step t.

The forward pass is the graph-D kernels (depthwise, split-bf16 pointwise / transposed convs, batch statistics, the double-norm fold,
affine + relu); the reverse pass is the graph-D' training kernels (batch-form norm backward with the relu mask, pointwise and
transposed-conv weight and data gradients, depthwise backward) and csrc/s_train.hip for the loss and the last two layers
(emd_s_head_bwd_f32).  Python is plumbing: buffers, views, launch order and the captured graph.

Parameters, gradients and Adam's two slots are flat device vectors in one layout.  The one-channel input is carried as 4 channels and
encoding_features < 4 as 4: the padded entries are not parameters -- their gradients are exactly zero by construction (zero inputs,
zero weights, a relu mask that is off), they stay zero, and they never reach ``weights()`` or a checkpoint.

Exactly-zero gradients: the normalizer BN's beta of every separable block (the second BN removes any shift) and the biases of the
first two transposed convs (a batch-statistics BN follows them) have zero gradient in exact arithmetic.  They are never written
(the gradient vector is cleared every step), so Adam leaves them bitwise at their initial values; TF float32 would hand them noise
of ~1e-8 that its Adam normalises into steps of size ~lr.

Moving statistics are never updated (the reference collects ``update_ops`` before building the graph, autoencoder.py:357-358, so
the list is empty, and the apply graph never reads them): they stay as initialised (0 / 1), or as restored.
"""
from __future__ import annotations

import ctypes as C
import os
import re
from collections import OrderedDict

import numpy as np

from . import _lib, ops, tf_checkpoint
from . import train_ops as TO
from .autoencoder import BN_EPS, DEC_CHANNELS, ENC_CHANNELS, AutoencoderEngine, variable_specs
from .k_trainer import s_crop, s_record_parser, step_from_beta_powers  # noqa: F401

CROPSIZE = 160
LR0, TOTAL_STEPS, PERIOD = 0.01, 100000, 50000   # autoencoder.py:427-431
VAL_SEED_XOR = 0x76616C   # the validation crops' Philox key: the seed with this mixed in ("val")
HEAD_C = DEC_CHANNELS[-1]


def lr_schedule(t: int, lr0: float = LR0, total_steps: int = TOTAL_STEPS, period: int = PERIOD) -> float:
    """autoencoder.py:427-431: lr = lr0 (1 - (t // period) / (total_steps // period))^1.5 at the 1-based step t."""
    return lr0 * (1.0 - (t // period) / (total_steps // period)) ** 1.5


def adam_lr_t(lr: float, t: int, beta1: float = 0.9, beta2: float = 0.999) -> float:
    """TF AdamOptimizer's bias-corrected step size lr sqrt(1 - beta2^t) / (1 - beta1^t)."""
    return lr * (1.0 - beta2 ** t) ** 0.5 / (1.0 - beta1 ** t)


def _is_moving(name):
    return name.endswith(("/moving_mean", "/moving_variance"))


def trainable_specs(encoding_features: int = 16):
    return OrderedDict((n, s) for n, s in variable_specs(encoding_features).items() if not _is_moving(n))


def zero_gradient_names(encoding_features: int = 16):
    """The variables whose gradient is identically zero: every separable block's normalizer beta and the first two transposed
    convs' biases."""
    names = [f"SeparableConv2d{'' if k == 0 else f'_{k}'}/BatchNorm/beta" for k in range(4)]
    return names + ["Conv2d_transpose/biases", "Conv2d_transpose_1/biases"]


def initial_weights(encoding_features: int = 16, seed: int = 0):
    """Xavier-uniform kernels (the fan-in / fan-out of autoencoder.synthetic_weights), biases 0, gamma 1, beta 0, moving mean 0,
    moving variance 1, from numpy's generator seeded by ``seed``."""
    rng = np.random.default_rng(seed)
    w = OrderedDict()
    for name, shape in variable_specs(encoding_features).items():
        leaf = name.rsplit("/", 1)[1]
        if leaf in ("depthwise_weights", "pointwise_weights", "weights"):
            rf = shape[0] * shape[1]
            lim = np.sqrt(6.0 / (rf * shape[2] + rf * shape[3]))
            w[name] = rng.uniform(-lim, lim, shape).astype(np.float32)
        elif leaf in ("gamma", "moving_variance"):
            w[name] = np.ones(shape, np.float32)
        else:
            w[name] = np.zeros(shape, np.float32)
    return w


def _p4(c):
    return -(-c // 4) * 4


def _layout(name, shape):
    """(canonical shape of the TF array, padded device shape) -- the device shapes are what the kernels read: depthwise [9][Cin],
    pointwise [Cin][Cout], transposed conv [9][Cout][Cin], final conv [9][64], norm vectors [C]."""
    leaf = name.rsplit("/", 1)[1]
    if leaf == "depthwise_weights":
        return (9, shape[2]), (9, _p4(shape[2]))
    if leaf == "pointwise_weights":
        return (shape[2], shape[3]), (_p4(shape[2]), _p4(shape[3]))
    if name.startswith("Conv2d_transpose") and leaf == "weights":
        return (9, shape[2], shape[3]), (9, shape[2], _p4(shape[3]))
    if name == "Conv/weights":
        return (9, shape[2]), (9, shape[2])
    return (shape[0],), ((_p4(shape[0]),) if name.startswith(("SeparableConv2d", "BatchNorm")) else (shape[0],))


def state_dict_names(encoding_features: int = 16):
    """The names tf.train.Saver writes for the training graph: every variable of variable_specs, Adam's two slots of every
    trainable one, and the two beta powers."""
    names = list(variable_specs(encoding_features))
    for n in trainable_specs(encoding_features):
        names += [n + "/Adam", n + "/Adam_1"]
    return names + ["beta1_power", "beta2_power"]


def s_state_dict(weights, adam_m, adam_v, step: int, encoding_features: int = 16, beta1: float = 0.9, beta2: float = 0.999):
    """The checkpoint tensors after ``step`` Adam steps under state_dict_names: weights (variable_specs), Adam's slots (trainable
    names) and beta1_power / beta2_power = beta^step."""
    out = OrderedDict((n, np.asarray(weights[n], np.float32)) for n in variable_specs(encoding_features))
    for n in trainable_specs(encoding_features):
        out[n + "/Adam"] = np.asarray(adam_m[n], np.float32)
        out[n + "/Adam_1"] = np.asarray(adam_v[n], np.float32)
    out["beta1_power"] = np.float32(beta1 ** step)
    out["beta2_power"] = np.float32(beta2 ** step)
    return out


def _as_batch(batch, device):
    """host or device [B,S,S(,1)] -> contiguous float32 CUDA [B,S,S]."""
    import torch

    x = batch if isinstance(batch, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(batch, dtype=np.float32))
    if x.dim() == 4:
        if x.shape[3] != 1:
            raise ValueError("channel dimension must be 1")
        x = x[..., 0]
    if x.dim() != 3 or x.shape[1] != x.shape[2] or x.shape[1] % 8 or x.shape[1] < 8:
        raise ValueError("expected a [B,S,S] or [B,S,S,1] batch, S a multiple of 8")
    return x.to(device=device, dtype=torch.float32).contiguous()


def sample_crops(stack_dev, B: int, crop: int, seed: int, first_index: int, out=None, x4=None, draws=None, first_index_dev=None,
                 stream=None):
    """emd_s_sample_crops_f32: B preprocessed crop x crop crops of the device stack [N,H,W] into ``out`` [B,crop,crop] and, if given,
    channel 0 of ``x4`` [B,crop,crop,4]; draws (int32 [B,4] CUDA tensor or None) receives (image, x, y, D4 element) per crop."""
    import torch

    N, H, W = stack_dev.shape
    if out is None:
        out = torch.empty((B, crop, crop), dtype=torch.float32, device=stack_dev.device)
    if x4 is not None:
        assert x4.is_contiguous() and tuple(x4.shape) == (B, crop, crop, 4)
    rc = _lib.load().emd_s_sample_crops_f32(_lib.ptr(stack_dev), N, H, W, _lib.ptr(out), _lib.ptr(x4) if x4 is not None else None, B,
                                            crop, C.c_ulonglong(int(seed) & 0xFFFFFFFFFFFFFFFF), C.c_ulonglong(int(first_index)),
                                            _lib.ptr(first_index_dev) if first_index_dev is not None else None,
                                            _lib.ptr(draws) if draws is not None else None, _lib.stream_ptr(stream))
    _lib.check(rc, "emd_s_sample_crops_f32")
    return out


def head_backward(out, x, a: ops.Act, w9, dw9, dbias, loss, da: ops.Act | None = None, fused=True, stream=None):
    """The loss and the reverse pass of the last two layers (a = relu(transposed conv + bias), out = conv3x3(a, w9) to one
    channel): dw9 [9][C] and dbias [C] += their gradients, loss[0] = mean (out - x)^2, returns da = dL/d(pre-activation) (written
    over a unless ``da`` is given).  fused: emd_s_head_bwd_f32, one pass; else the composed route (emd_s_mse_loss_f32,
    emd_conv3x3_cout1_wgrad_f32, emd_conv3x3_cout1_bwd_data_f32, emd_relu_mask_bwd_f32, emd_bn_bwd_reduce_f32)."""
    import torch

    lib = _lib.load()
    B, H, W, Cc = a.B, a.H, a.W, a.C
    assert out.numel() == x.numel() == B * H * W and out.is_contiguous() and x.is_contiguous()
    if da is None:
        da = a
    if fused:
        nb = lib.emd_s_head_bwd_workspace_bytes(B, H, W, Cc)
        ws = torch.empty((nb + 3) // 4, dtype=torch.float32, device=out.device)
        _lib.check(lib.emd_s_head_bwd_f32(_lib.ptr(out), _lib.ptr(x), a.ptr, a.ld, _lib.ptr(w9), B, H, W, Cc, da.ptr, da.ld, _lib.ptr(dw9),
                                          _lib.ptr(dbias) if dbias is not None else None, _lib.ptr(loss), _lib.ptr(ws), nb,
                                          _lib.stream_ptr(stream)), "emd_s_head_bwd_f32")
        return da
    dout = torch.empty((B, H, W), dtype=torch.float32, device=out.device)
    ws = torch.empty(lib.emd_s_mse_loss_workspace_bytes() // 8, dtype=torch.float64, device=out.device)
    _lib.check(lib.emd_s_mse_loss_f32(_lib.ptr(out), _lib.ptr(x), C.c_long(out.numel()), _lib.ptr(loss), _lib.ptr(dout), _lib.ptr(ws),
                                      _lib.stream_ptr(stream)), "emd_s_mse_loss_f32")
    TO.conv3x3_cout1_wgrad(a, dout, dw9, stream=stream)
    g = da if da is not a else ops.Act.empty(B, H, W, Cc, out.device)
    TO.conv3x3_cout1_bwd_data(dout, w9, g, stream=stream)
    assert a.ld == Cc and g.ld == Cc and da.ld == Cc
    _lib.check(lib.emd_relu_mask_bwd_f32(a.ptr, g.ptr, da.ptr, C.c_long(B * H * W * Cc), _lib.stream_ptr(stream)), "emd_relu_mask_bwd_f32")
    if dbias is not None:
        TO.chan_reduce(da, dbias, accumulate_s1=True, stream=stream)
    return da


class AutoencoderTrainer:
    """Trains graph S (the apply graph of Micrograph_Autoencoder) on the GPU as misc_py/autoencoder.py trains it.

    encoding_features  channels of the code (1, 4 and 16 are the sizes apply_autoencoders.py loads).
    seed               seeds the initial weights (initial_weights) and keys the Philox stream of train()'s crop sampler.
    lr0, total_steps, period: lr = lr0 (1 - (t // period) / (total_steps // period))^1.5 at the 1-based step t.
    initial            optional weights (variable_specs(encoding_features)) to start from instead of initial_weights.
    fused_head         the loss and last two layers' reverse pass as one pass (emd_s_head_bwd_f32) or the composed route."""

    def __init__(self, encoding_features: int = 16, device=None, seed: int = 0, lr0: float = LR0, total_steps: int = TOTAL_STEPS,
                 period: int = PERIOD, initial=None, fused_head: bool = True, beta1: float = 0.9, beta2: float = 0.999,
                 eps: float = 1e-8):
        import torch

        if not (isinstance(encoding_features, (int, np.integer)) and 1 <= encoding_features <= 256):
            raise ValueError("encoding_features must be 1..256")
        if total_steps < 1 or period < 1 or total_steps // period < 1 or lr0 < 0:
            raise ValueError("bad learning-rate schedule")
        self.enc = int(encoding_features)
        self.lr0, self.total_steps, self.period = float(lr0), int(total_steps), int(period)
        self.beta1, self.beta2, self.eps = float(beta1), float(beta2), float(eps)
        self.seed = int(seed)
        self.fused_head = bool(fused_head)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.lib = _lib.load()
        w0 = initial_weights(self.enc, self.seed) if initial is None else initial
        specs = variable_specs(self.enc)
        if set(w0) != set(specs):
            raise ValueError("initial weights do not match variable_specs(encoding_features)")
        self.specs = specs
        self.trainable = trainable_specs(self.enc)
        self.moving = OrderedDict((n, np.asarray(w0[n], np.float32).copy()) for n in specs if _is_moving(n))

        # one layout for parameters, gradients and Adam's slots; every view starts on a 16-byte boundary
        self._offs, n = {}, 0
        for name, shape in self.trainable.items():
            canon, padded = _layout(name, shape)
            self._offs[name] = (n, canon, padded)
            n += -(-int(np.prod(padded)) // 4) * 4
        self.n = n
        z = lambda: torch.zeros(n, dtype=torch.float32, device=self.device)
        self.params, self.grads, self.m, self.v = z(), z(), z(), z()
        self.params.copy_(torch.from_numpy(self._flatten({k: w0[k] for k in self.trainable})))
        self.P = OrderedDict((k, self._view(self.params, k)) for k in self.trainable)
        self.G = OrderedDict((k, self._view(self.grads, k)) for k in self.trainable)
        self.ones = torch.ones(256, dtype=torch.float32, device=self.device)
        self.zeros = torch.zeros(256, dtype=torch.float32, device=self.device)
        self.loss_buf = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.lr_t_dev = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.index_dev = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.step = 0
        self._x4 = {}
        self._graphs = {}
        self._stacks = {}
        # test hooks (teacher forcing, as DenoiserTrainer.teacher): name -> CUDA float32 tensor in the device layout (padded
        # channels) that REPLACES the forward's tensor of that name ("sep{k}/d", "sep{k}/r", "dec{k}/r", "out") or the gradient
        # arriving at a layer in the reverse pass ("sep{k}/dy", "dec{k}/dy", "dec2/dr"); ``record`` (a dict) receives copies of
        # every layer's output and input gradient ("sep{k}/a", "dec{k}/a", "head/dr", "sep{k}/dx", "dec{k}/dx")
        self.teacher = None
        self.record = None

        # layers: packed bf16 planes of the pointwise and transposed-conv weights, forward and data-gradient orientation
        self.blocks, self.decs = [], []
        pb = TO.PackBatch(self.device)
        cin = 1
        for k, cout in enumerate(ENC_CHANNELS + (self.enc,)):
            s = "SeparableConv2d" if k == 0 else f"SeparableConv2d_{k}"
            o = "BatchNorm" if k == 0 else f"BatchNorm_{k}"
            ci, co = _p4(cin), _p4(cout)
            pw = self.P[s + "/pointwise_weights"].view(1, ci, co)
            L = {"s": s, "o": o, "stride": 2 if k < 3 else 1, "ci": ci, "co": co, "dw": self.P[s + "/depthwise_weights"],
                 "pk_f": TO.DevPackedWeights(1, ci, co, self.device), "pk_b": TO.DevPackedWeights(1, co, ci, self.device)}
            pb.add(L["pk_f"], pw, 1, cout_major=False)
            pb.add(L["pk_b"], pw, 1, cout_major=True, tap_sel=[0])
            self.blocks.append(L)
            cin = cout
        for k, cout in enumerate(DEC_CHANNELS):
            s = "Conv2d_transpose" if k == 0 else f"Conv2d_transpose_{k}"
            ci = _p4(cin)
            w = self.P[s + "/weights"].view(9, cout, ci)
            L = {"s": s, "o": f"BatchNorm_{4 + k}" if k < 2 else None, "ci": ci, "co": cout,
                 "pk_f": [TO.DevPackedWeights(len(ops.deconv_phase_taps(ph)), ci, cout, self.device) for ph in range(4)],
                 "pk_b": TO.DevPackedWeights(9, cout, ci, self.device)}
            for ph in range(4):
                pb.add(L["pk_f"][ph], w, 9, cout_major=True, tap_sel=[ky * 3 + kx for (ky, kx) in ops.deconv_phase_taps(ph)])
            pb.add(L["pk_b"], w, 9, cout_major=False)
            self.decs.append(L)
            cin = cout
        self.w_final = self.P["Conv/weights"]
        self._pack = pb
        self._pack.run()

    # ---- parameter layout
    def _view(self, flat, name):
        off, _, padded = self._offs[name]
        return flat[off: off + int(np.prod(padded))].view(padded)

    def _flatten(self, arrays):
        host = np.zeros(self.n, np.float32)
        for name, a in arrays.items():
            off, canon, padded = self._offs[name]
            buf = np.zeros(padded, np.float32)
            buf[tuple(slice(0, c) for c in canon)] = np.asarray(a, np.float32).reshape(canon)
            host[off: off + buf.size] = buf.reshape(-1)
        return host

    def _unflatten(self, flat_host):
        out = OrderedDict()
        for name, shape in self.trainable.items():
            off, canon, padded = self._offs[name]
            buf = flat_host[off: off + int(np.prod(padded))].reshape(padded)
            out[name] = np.ascontiguousarray(buf[tuple(slice(0, c) for c in canon)]).reshape(shape).astype(np.float32)
        return out

    # ---- one step
    def _input(self, B, S):
        import torch

        key = (B, S)
        if key not in self._x4:   # channels 1..3 stay zero: only channel 0 is ever written
            self._x4[key] = (torch.zeros((B, S, S, 4), dtype=torch.float32, device=self.device),
                             torch.empty((B, S, S), dtype=torch.float32, device=self.device))
        return self._x4[key]

    def _E(self, B, H, W, Cc):
        return ops.Act.empty(B, H, W, Cc, self.device)

    def _force(self, t, name):
        """Teacher forcing: overwrite t (an ops.Act or a tensor) with self.teacher[name] when there is one."""
        if self.teacher is not None and name in self.teacher:
            dst = t.torch() if isinstance(t, ops.Act) else t
            dst.copy_(self.teacher[name].reshape(dst.shape))
        return t

    def _rec(self, t, name):
        if self.record is not None:
            self.record[name] = (t.torch() if isinstance(t, ops.Act) else t).clone()

    def _forward(self, x4):
        """Forward on batch statistics -> (out [B,S,S], per-layer contexts)."""
        import torch

        a = ops.Act(x4)
        B = a.B
        ctx = []
        for L in self.blocks:
            Ho = -(-a.H // L["stride"])
            d = self._force(ops.dw3x3(a, L["dw"], self._E(B, Ho, Ho, L["ci"]), stride=L["stride"]), f"sep{len(ctx)}/d")
            r = self._force(ops.conv1x1(d, L["pk_f"], self.ones, self.zeros, self._E(B, Ho, Ho, L["co"]), act=ops.ACT_NONE),
                            f"sep{len(ctx)}/r")
            mean, var = ops.bn_batch_stats(r)
            s, o = L["s"], L["o"]
            fold = TO.bn_train_fold(mean, var, self.P[o + "/gamma"], self.P[o + "/beta"], B * Ho * Ho,
                                    gamma1=self.P[s + "/BatchNorm/gamma"], beta1=self.P[s + "/BatchNorm/beta"], eps=BN_EPS)
            out = ops.affine_act(r, fold["scale"], fold["shift"], self._E(B, Ho, Ho, L["co"]), act=ops.ACT_RELU)
            self._rec(out, f"sep{len(ctx)}/a")
            ctx.append({"x": a, "d": d, "r": r, "fold": fold})
            a = out
        for k, L in enumerate(self.decs):
            bias = self.P[L["s"] + "/biases"]
            r = ops.deconv3x3s2(a, L["pk_f"], self.ones, bias, self._E(B, 2 * a.H, 2 * a.W, L["co"]),
                                act=ops.ACT_NONE if k < 2 else ops.ACT_RELU)
            self._force(r, f"dec{k}/r")
            c = {"x": a, "r": r}
            if k < 2:
                mean, var = ops.bn_batch_stats(r)
                c["fold"] = TO.bn_train_fold(mean, var, self.P[L["o"] + "/gamma"], self.P[L["o"] + "/beta"], r.B * r.H * r.W, eps=BN_EPS)
                r = ops.affine_act(r, c["fold"]["scale"], c["fold"]["shift"], self._E(B, r.H, r.W, L["co"]), act=ops.ACT_RELU)
            self._rec(r, f"dec{k}/a")
            ctx.append(c)
            a = r
        out = torch.empty((B, a.H, a.W), dtype=torch.float32, device=self.device)
        ops.conv3x3_cout1(a, self.w_final, 1.0, 0.0, out, act=0)
        self._force(out, "out")
        return out, a, ctx

    def _backward(self, out, x, a, ctx, fused):
        """Clears the gradient vector and fills it; loss_buf[0] = the loss."""
        self.grads.zero_()
        dr = head_backward(out, x, a, self.w_final, self.G["Conv/weights"], self.G["Conv2d_transpose_2/biases"], self.loss_buf,
                           fused=fused)
        self._rec(dr, "head/dr")
        self._force(dr, "dec2/dr")
        nb = len(self.blocks)
        for k in (2, 1, 0):
            L, c = self.decs[k], ctx[nb + k]
            if k < 2:
                self._force(dr, f"dec{k}/dy")   # dy -> d loss / d r over r; the bias gradient is zero (the norm removes it) and is not written
                o = L["o"]
                dr = TO.bn_backward(dr, c["r"], c["fold"], self.P[o + "/gamma"], self.G[o + "/gamma"], self.G[o + "/beta"], c["r"],
                                    mask=TO.MASK_RELU)
            x_in = c["x"]
            tdy, tdx = TO.conv_taps(dr.H, dr.W, 2, 1)
            TO.conv_wgrad(dr, x_in, self.G[L["s"] + "/weights"].view(9, L["co"], L["ci"]), tdy, tdx, sa=2)
            dx = ops.conv3x3(dr, L["pk_b"], self.ones, self.zeros, self._E(x_in.B, x_in.H, x_in.W, L["ci"]), stride=2, act=False)
            self._rec(dx, f"dec{k}/dx")
            dr = dx
        for k in (3, 2, 1, 0):
            L, c = self.blocks[k], ctx[k]
            s, o = L["s"], L["o"]
            self._force(dr, f"sep{k}/dy")
            r = TO.bn_backward(dr, c["r"], c["fold"], self.P[o + "/gamma"], self.G[o + "/gamma"], self.G[o + "/beta"], c["r"],
                               mask=TO.MASK_RELU, gamma1=self.P[s + "/BatchNorm/gamma"], dgamma1=self.G[s + "/BatchNorm/gamma"])
            d, x_in = c["d"], c["x"]
            TO.conv_wgrad(d, r, self.G[s + "/pointwise_weights"].view(1, L["ci"], L["co"]))
            dd = ops.conv1x1(r, L["pk_b"], self.ones, self.zeros, d, act=False)
            TO.dw3x3_wgrad(x_in, dd, self.G[s + "/depthwise_weights"], stride=L["stride"])
            if k > 0:
                dr = TO.dw3x3_bwd_data(dd, L["dw"], self._E(x_in.B, x_in.H, x_in.W, x_in.C), stride=L["stride"])
                self._rec(dr, f"sep{k}/dx")

    def _apply(self, t=None):
        """Adam at the 1-based step t on the device rate lr_t_dev, then the re-pack of the weights."""
        TO.adam_step(self.params, self.grads, self.m, self.v, t, None, beta1=self.beta1, beta2=self.beta2, eps=self.eps,
                     lr_t_dev=self.lr_t_dev)
        self._pack.run()

    def _body(self, x4, x, update, fused=None):
        out, a, ctx = self._forward(x4)
        self._backward(out, x, a, ctx, self.fused_head if fused is None else fused)
        if update:
            self._apply()
        return out

    def _set_rate(self, t):
        self.lr_t_dev.fill_(adam_lr_t(lr_schedule(t, self.lr0, self.total_steps, self.period), t, self.beta1, self.beta2))

    def _check_steps(self, steps):
        if self.step + steps > self.total_steps:
            raise ValueError(f"{self.step} + {steps} steps run past total_steps={self.total_steps}: the learning-rate schedule ends there")

    def _load(self, batch):
        x = _as_batch(batch, self.device)
        B, S = x.shape[0], x.shape[1]
        x4, tgt = self._input(B, S)
        x4[..., 0].copy_(x)
        tgt.copy_(x)
        return x4, tgt

    def train_step(self, batch, graph: bool = False):
        """One Adam step on ``batch`` (host or device [B,S,S(,1)], S a multiple of 8; the target is the batch itself).  Returns
        the loss (computed with the parameters before the update, as the reference's sess.run) as a device scalar.
        graph=True: the step (copy-in excluded) is captured once per shape into a hipGraph and replayed."""
        self._check_steps(1)
        x4, tgt = self._load(batch)
        t = self.step + 1
        self._set_rate(t)
        if graph:
            self._replay(("batch", tuple(x4.shape)), lambda: self._body(x4, tgt, True))
        else:
            self._body(x4, tgt, True)
        self.step = t
        return self.loss_buf[0].clone()

    def loss_and_grad(self, batch, fused=None):
        """(loss, {TF variable name: gradient}) on ``batch`` with the current parameters, no update."""
        x4, tgt = self._load(batch)
        self._body(x4, tgt, False, fused)
        g = self._unflatten(self.grads.cpu().numpy())
        return float(self.loss_buf[0].item()), g

    def evaluate(self, batch):
        """The loss on ``batch`` with the current parameters."""
        import torch

        x4, tgt = self._load(batch)
        out, _, _ = self._forward(x4)
        ws = torch.empty(self.lib.emd_s_mse_loss_workspace_bytes() // 8, dtype=torch.float64, device=self.device)
        loss = torch.empty(1, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.emd_s_mse_loss_f32(_lib.ptr(out), _lib.ptr(tgt), C.c_long(out.numel()), _lib.ptr(loss), None, _lib.ptr(ws),
                                               _lib.stream_ptr()), "emd_s_mse_loss_f32")
        return float(loss.item())

    def _replay(self, key, fn):
        """Run ``fn`` (one whole step on fixed buffers) as a captured graph on one stream: captured on first use, replayed after."""
        import torch

        g = self._graphs.get(key)
        if g is None:
            # code objects load on first use: one launch of every kernel outside of capture, with the state put back afterwards
            keep = [t.clone() for t in (self.params, self.m, self.v, self.loss_buf)]
            fn()
            for dst, src in zip((self.params, self.m, self.v, self.loss_buf), keep):
                dst.copy_(src)
            self._pack.run()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                fn()
            self._graphs[key] = g
        g.replay()

    def train(self, stack, steps: int, batch_size: int = 32, val_stack=None, val_skip_n: int = 10, crop: int = CROPSIZE,
              graph: bool = True, chunk: int = 1000):
        """``steps`` steps on crops sampled on the device from ``stack`` ([N,H,W(,1)], host or device; H, W > crop).  The i-th step
        this trainer takes (i = 0, 1, ..., i.e. 1-based step t = i + 1) draws crops b = 0..batch_size-1 from Philox(seed, i*B + b).
        The stack is copied into one device buffer per stack shape, which the captured graph reads.  Every
        ``val_skip_n``-th step a batch from ``val_stack`` is evaluated after the update.  graph=True: sampler, forward, reverse pass
        and Adam as one captured graph, replayed with the crop index and lr_t on the device.  The device is read once per ``chunk``
        steps.  Returns {"loss": [steps], "val_step": [k], "val_loss": [k]}."""
        import torch

        if steps < 0 or batch_size < 1 or chunk < 1 or val_skip_n < 1:
            raise ValueError("bad steps / batch_size / chunk / val_skip_n")
        if crop % 8:
            raise ValueError("crop must be a multiple of 8")
        self._check_steps(steps)
        src = self._stack(stack, crop)
        val = self._stack(val_stack, crop) if val_stack is not None else None
        dst = self._stacks.get(tuple(src.shape))   # one device buffer per stack shape: the captured graph reads it
        if dst is None:
            dst = self._stacks[tuple(src.shape)] = torch.empty_like(src)
        if dst.data_ptr() != src.data_ptr():
            dst.copy_(src)
        src = dst
        x4, tgt = self._input(batch_size, crop)
        key = ("sample", batch_size, crop, tuple(src.shape))

        def body():
            sample_crops(src, batch_size, crop, self.seed, 0, out=tgt, x4=x4, first_index_dev=self.index_dev)
            self._body(x4, tgt, True)

        losses, val_steps, val_losses = [], [], []
        done = 0
        while done < steps:
            n = min(chunk, steps - done)
            buf = torch.empty(n, dtype=torch.float32, device=self.device)
            for k in range(n):
                t = self.step + 1
                self._set_rate(t)
                self.index_dev.fill_(self.step * batch_size)
                if graph:
                    self._replay(key, body)
                else:
                    body()
                buf[k: k + 1].copy_(self.loss_buf)
                self.step = t
                if val is not None and self.step % val_skip_n == 0:
                    vx4, vt = self._input(batch_size, crop)
                    sample_crops(val, batch_size, crop, self.seed ^ VAL_SEED_XOR, (self.step - 1) * batch_size, out=vt, x4=vx4)
                    val_losses.append(self.evaluate(vt))
                    val_steps.append(self.step)
            losses.append(buf.cpu().numpy())
            done += n
        return {"loss": np.concatenate(losses) if losses else np.zeros(0, np.float32), "val_step": np.asarray(val_steps, np.int64),
                "val_loss": np.asarray(val_losses, np.float32)}

    def _stack(self, stack, crop):
        import torch

        s = stack if isinstance(stack, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(stack, dtype=np.float32))
        if s.dim() == 4 and s.shape[3] == 1:
            s = s[..., 0]
        if s.dim() != 3 or s.shape[1] <= crop or s.shape[2] <= crop:
            raise ValueError(f"expected an [N,H,W] stack with H, W > {crop}")
        return s.to(device=self.device, dtype=torch.float32).contiguous()

    # ---- weights and checkpoints
    def weights(self):
        """OrderedDict matching variable_specs(encoding_features): the trained variables and the (never updated) moving statistics."""
        tr = self._unflatten(self.params.cpu().numpy())
        return OrderedDict((n, tr[n] if n in tr else self.moving[n].copy()) for n in self.specs)

    def engine(self):
        """An AutoencoderEngine (the apply graph, per-image statistics) built from weights()."""
        return AutoencoderEngine(self.weights(), self.device, self.enc)

    def state_dict(self):
        """name -> numpy array under the names tf.train.Saver gives the training graph's variables (state_dict_names)."""
        return s_state_dict(self.weights(), self._unflatten(self.m.cpu().numpy()), self._unflatten(self.v.cpu().numpy()), self.step,
                            self.enc, self.beta1, self.beta2)

    def save_checkpoint(self, directory, global_step=None):
        """saver.save(sess, directory + "/", global_step): the bundle <directory>/-<global_step>.{index,data-*} and the
        ``checkpoint`` state file; Micrograph_Autoencoder(checkpoint_loc=directory) reads it.  Returns the prefix."""
        step = self.step if global_step is None else int(global_step)
        if step != self.step:
            raise ValueError(f"global_step {step} is not the trainer's step count {self.step}: its Adam state would not match")
        os.makedirs(directory, exist_ok=True)
        prefix = os.path.join(directory, "") + f"-{step}"
        tf_checkpoint.write_checkpoint(prefix, self.state_dict())
        return prefix

    def restore(self, directory):
        """Resume from tf_checkpoint.latest_checkpoint(directory): variables, Adam slots, moving statistics and the step count
        (read from the beta powers and checked against the ``-<global_step>`` suffix of the name when there is one)."""
        import torch

        prefix = tf_checkpoint.latest_checkpoint(directory)
        if prefix is None:
            raise FileNotFoundError(f"{directory}: no checkpoint")
        z = tf_checkpoint.read_checkpoint(prefix)
        m = re.search(r"-(\d+)$", prefix)
        named = int(m.group(1)) if m else None
        t = step_from_beta_powers(float(np.asarray(z["beta1_power"]).reshape(-1)[0]), float(np.asarray(z["beta2_power"]).reshape(-1)[0]),
                                  self.beta1, self.beta2)
        if t is None:
            t = named
        if t is None:
            raise ValueError(f"{prefix}: the step count is neither in the beta powers nor in the name")
        if named is not None and t != named:
            raise ValueError(f"{prefix}: beta powers say step {t}, the checkpoint name says {named}")
        if t > self.total_steps:
            raise ValueError(f"{prefix}: step {t} is past total_steps={self.total_steps}")
        for n, shape in self.specs.items():
            if tuple(np.asarray(z[n]).shape) != tuple(shape):
                raise ValueError(f"{n}: shape {np.asarray(z[n]).shape} != {shape}")
        self.params.copy_(torch.from_numpy(self._flatten({n: z[n] for n in self.trainable})))
        self.m.copy_(torch.from_numpy(self._flatten({n: z[n + "/Adam"] for n in self.trainable})))
        self.v.copy_(torch.from_numpy(self._flatten({n: z[n + "/Adam_1"] for n in self.trainable})))
        for n in self.moving:
            self.moving[n] = np.asarray(z[n], np.float32).copy()
        self._pack.run()
        self.step = t
        return prefix
