"""Float64 restatement of graph S's training objective for the tests of emdenoise.autoencoder_trainer: the apply graph of
misc_py/apply_autoencoders.py:91-187 with every batch norm on the statistics of the WHOLE batch (the training graph,
misc_py/autoencoder.py:339-506; oracle.autoencoder_graph runs one image at a time, as the apply side does), the loss
tf.losses.mean_squared_error(x, out) (:177-188), gradients by autograd, and TF's Adam."""
from collections import OrderedDict

import numpy as np
import torch

from oracle import tf_ops as T
from oracle.autoencoder_graph import BN_EPS, variable_specs


def _bn(x, gamma, beta):
    mean = x.mean(dim=(0, 1, 2), keepdim=True)
    var = ((x - mean) ** 2).mean(dim=(0, 1, 2), keepdim=True)
    return (x - mean) / torch.sqrt(var + BN_EPS) * gamma + beta


def forward(x, w, trace=None):
    """x [B,S,S,1] tensor, w {name: tensor} -> out [B,S,S,1]; trace (list) receives every layer's output."""
    a = x
    for k, stride in enumerate((2, 2, 2, 1)):
        s = "SeparableConv2d" if k == 0 else f"SeparableConv2d_{k}"
        o = "BatchNorm" if k == 0 else f"BatchNorm_{k}"
        a = T.depthwise_conv2d_t(a, w[s + "/depthwise_weights"], stride=stride)
        a = T.conv2d_t(a, w[s + "/pointwise_weights"], None)
        a = _bn(a, w[s + "/BatchNorm/gamma"], w[s + "/BatchNorm/beta"])
        a = torch.relu(_bn(a, w[o + "/gamma"], w[o + "/beta"]))
        if trace is not None:
            trace.append(a)
    for k in range(3):
        s = "Conv2d_transpose" if k == 0 else f"Conv2d_transpose_{k}"
        a = T.conv2d_transpose_s2_t(a, w[s + "/weights"], w[s + "/biases"])
        if k < 2:
            a = _bn(a, w[f"BatchNorm_{4 + k}/gamma"], w[f"BatchNorm_{4 + k}/beta"])
        a = torch.relu(a)
        if trace is not None:
            trace.append(a)
    return T.conv2d_t(a, w["Conv/weights"], None)


def trainable(encoding_features):
    return [n for n in variable_specs(encoding_features) if not n.endswith(("/moving_mean", "/moving_variance"))]


def loss_and_grads(batch, weights, encoding_features, dtype=np.float64):
    """batch [B,S,S] numpy, weights {name: array} -> (loss, {trainable name: gradient}), in float64 (or ``dtype``: float32 shows
    how far a float32 evaluation of the same graph lands from float64)."""
    x = torch.from_numpy(np.asarray(batch, dtype))[..., None]
    w = {n: torch.tensor(np.asarray(weights[n], dtype), requires_grad=n in trainable(encoding_features))
         for n in variable_specs(encoding_features)}
    out = forward(x, w)
    loss = ((out - x) ** 2).mean()
    names = trainable(encoding_features)
    grads = torch.autograd.grad(loss, [w[n] for n in names])
    return float(loss.detach()), OrderedDict((n, g.numpy()) for n, g in zip(names, grads))


def adam_trajectory(batches, weights, encoding_features, lr_fn, steps, beta1=0.9, beta2=0.999, eps=1e-8, zero=()):
    """``steps`` float64 TF-Adam steps (m, v, lr_t = lr sqrt(1-beta2^t)/(1-beta1^t), var -= lr_t m / (sqrt(v) + eps)) on
    batches[t % len]; the gradients of ``zero`` are taken as exactly 0 (their exact value).  Returns the trainable weights."""
    w = {n: np.asarray(v, np.float64).copy() for n, v in weights.items()}
    names = trainable(encoding_features)
    m = {n: np.zeros_like(w[n]) for n in names}
    v = {n: np.zeros_like(w[n]) for n in names}
    for t in range(1, steps + 1):
        _, g = loss_and_grads(batches[(t - 1) % len(batches)], w, encoding_features)
        lr_t = lr_fn(t) * np.sqrt(1 - beta2 ** t) / (1 - beta1 ** t)
        for n in names:
            gn = np.zeros_like(g[n]) if n in zero else g[n]
            m[n] = beta1 * m[n] + (1 - beta1) * gn
            v[n] = beta2 * v[n] + (1 - beta2) * gn * gn
            w[n] = w[n] - lr_t * m[n] / (np.sqrt(v[n]) + eps)
    return {n: w[n] for n in names}


def trace_grads(batch, weights, encoding_features):
    """The float64 forward with every layer's tensors and their loss gradients, for teacher forcing: returns (loss, values,
    grads, param_grads).  values: "sep{k}/d", "sep{k}/r" (pointwise output), "sep{k}/a"; "dec{k}/r" (transposed conv + bias),
    "dec{k}/a"; "out".  grads: d loss / d of every "*/a" and of "dec2/r"."""
    x = torch.from_numpy(np.asarray(batch, np.float64))[..., None]
    names = trainable(encoding_features)
    w = {n: torch.tensor(np.asarray(weights[n], np.float64), requires_grad=n in names) for n in variable_specs(encoding_features)}
    v = OrderedDict()
    a = x
    for k, stride in enumerate((2, 2, 2, 1)):
        s = "SeparableConv2d" if k == 0 else f"SeparableConv2d_{k}"
        o = "BatchNorm" if k == 0 else f"BatchNorm_{k}"
        v[f"sep{k}/d"] = d = T.depthwise_conv2d_t(a, w[s + "/depthwise_weights"], stride=stride)
        v[f"sep{k}/r"] = r = T.conv2d_t(d, w[s + "/pointwise_weights"], None)
        a = torch.relu(_bn(_bn(r, w[s + "/BatchNorm/gamma"], w[s + "/BatchNorm/beta"]), w[o + "/gamma"], w[o + "/beta"]))
        v[f"sep{k}/a"] = a
    for k in range(3):
        s = "Conv2d_transpose" if k == 0 else f"Conv2d_transpose_{k}"
        v[f"dec{k}/r"] = r = T.conv2d_transpose_s2_t(a, w[s + "/weights"], w[s + "/biases"])
        a = torch.relu(_bn(r, w[f"BatchNorm_{4 + k}/gamma"], w[f"BatchNorm_{4 + k}/beta"]) if k < 2 else r)
        v[f"dec{k}/a"] = a
    v["out"] = out = T.conv2d_t(a, w["Conv/weights"], None)
    loss = ((out - x) ** 2).mean()
    gk = [n for n in v if n.endswith("/a")] + ["dec2/r"]
    res = torch.autograd.grad(loss, [v[n] for n in gk] + [w[n] for n in names])
    grads = OrderedDict((n, g.numpy()) for n, g in zip(gk, res[:len(gk)]))
    pgrads = OrderedDict((n, g.numpy()) for n, g in zip(names, res[len(gk):]))
    return float(loss.detach()), OrderedDict((n, t.detach().numpy()) for n, t in v.items()), grads, pgrads
