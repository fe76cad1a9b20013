"""Float64 restatement of graph K's training objective (misc_py/noise-removal-kernels.py:378-438) in torch, for the tests
of emdenoise.k_trainer: filter_fn over the REFLECT-padded image (:99-105, :378-399), both losses, and the gradient with
respect to the make_layer scalars ``theta`` (layout of emd_k_train_step_f32: w [depth][nsym] | b1.. | s1..) by autograd."""
import numpy as np
import torch
import torch.nn.functional as F


def sym_pairs(width):
    o = width // 2
    return [(x, y) for x in range(o + 1) for y in range(x + 1)]


def tap_classes(width):
    """[w*w] class (creation index of the shared scalar) of every tap."""
    o = width // 2
    lut = {p: k for k, p in enumerate(sym_pairs(width))}
    return [lut[(max(abs(i - o), abs(j - o)), min(abs(i - o), abs(j - o)))] for i in range(width) for j in range(width)]


def _maps(theta, depth, width):
    n = len(sym_pairs(width))
    cls = torch.tensor(tap_classes(width), device=theta.device)
    Wm = [theta[l * n:(l + 1) * n][cls] for l in range(depth)]
    Bm = [None] + [theta[depth * n + (l - 1) * n: depth * n + l * n][cls] for l in range(1, depth)]
    S = [None] + [theta[(2 * depth - 1) * n + l - 1] for l in range(1, depth)]
    return Wm, Bm, S


def _tap(xp, Wm, Bm, S, depth, width, i, j, H, W):
    k = i * width + j
    f = Wm[0][k] * xp[:, i:i + H, j:j + W]
    for l in range(1, depth):
        f = Wm[l][k] * (S[l] * torch.sigmoid(f + Bm[l][k]))
    return f


def _pad(x, width):
    o = width // 2
    return F.pad(x[:, None], (o, o, o, o), mode="reflect")[:, 0]


def ref_forward(x, theta, depth, width):
    """x [B,H,W] float64 tensor, theta float64 tensor -> F(x) [B,H,W] (the image the filter returns, un-transposed)."""
    B, H, W = x.shape
    xp = _pad(x, width)
    Wm, Bm, S = _maps(theta, depth, width)
    out = torch.zeros_like(x)
    for i in range(width):
        for j in range(width):
            out = out + _tap(xp, Wm, Bm, S, depth, width, i, j, H, W)
    return out


def ref_target(x, loss):
    """The reference assembles its output transposed (stack axis=1, then axis=2, :421-424) and compares it with the input
    (:438): output[b,j,i] = F(x)[b,i,j], so F(x)[b,i,j] is held against x[b,j,i]."""
    return x.transpose(1, 2) if loss == "reference" else x


def ref_loss(out, x, loss):
    return torch.mean((out - ref_target(x, loss)) ** 2)


def ref_loss_and_grad(x, theta, depth, width, loss):
    """(loss, dloss/dtheta) in float64 by autograd, one tap at a time (dL/dF is computed first, then every tap's sub-graph is
    back-propagated with it), so that a 512 x 512 batch with 225 taps fits in memory.  x: torch float64 [B,H,W] (any
    device); theta: numpy or torch."""
    x = x.to(torch.float64)
    th = torch.as_tensor(np.asarray(theta, np.float64) if not isinstance(theta, torch.Tensor) else theta,
                         dtype=torch.float64, device=x.device).detach().clone().requires_grad_(True)
    B, H, W = x.shape
    xp = _pad(x, width)
    with torch.no_grad():
        out = ref_forward(x, th, depth, width)
        r = out - ref_target(x, loss)
        L = float(torch.mean(r * r))
        dout = 2.0 * r / r.numel()
    for i in range(width):
        for j in range(width):
            Wm, Bm, S = _maps(th, depth, width)
            f = _tap(xp, Wm, Bm, S, depth, width, i, j, H, W)
            f.backward(dout)
    return L, th.grad.detach().cpu().numpy()
