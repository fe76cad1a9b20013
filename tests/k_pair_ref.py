"""Float64 restatement of graph K's PAIRED training objective (misc_py/noise_removal_kernels_duplicate.py:406-434) and of the
pair maker (misc_py/autoencoder_train-val-test.py:35-55), for the tests of emdenoise.k_trainer's paired surface.

pair_forward      filter_fn over the unpadded image ("valid": the (H-w+1) x (W-w+1) interior) or the REFLECT-padded one.
pair_loss         mean((F(x) - truth interior)^2), and sqrt of it when it exceeds 1 and the rule is on (:433).
pair_loss_and_grad  the loss and d loss / d theta by float64 autograd through all of the above.
pair_adam         TF's AdamOptimizer in float64 on a list of pair batches (lr = lr0 (1 - t/(T+1)), lr_t = lr sqrt(1-b2^t)/(1-b1^t),
                  m / (sqrt(v) + eps)), the arithmetic tests/test_k_train_gpu.py restates for the unpaired trainer.
pair_loss_loop    the same loss by a literal per-pixel, per-tap double loop (pins pair_forward / pair_loss a second time).
make_pairs_ref    the pair maker in float64 numpy, given the draws.
theta's layout is emd_k_train_step_f32's: w [depth][nsym] | b1.. | s1.. (tests/k_train_ref.py)."""
import math

import numpy as np
import torch

from .k_train_ref import _maps, _pad, _tap, sym_pairs, tap_classes  # noqa: F401


def pair_forward(x, theta, depth, width, pad):
    """x [B,H,W] float64 tensor -> F(x): [B,H-w+1,W-w+1] for pad "valid", [B,H,W] for "reflect"."""
    B, H, W = x.shape
    if pad == "valid":
        xp, Ho, Wo = x, H - width + 1, W - width + 1
    else:
        xp, Ho, Wo = _pad(x, width), H, W
    Wm, Bm, S = _maps(theta, depth, width)
    out = torch.zeros((B, Ho, Wo), dtype=x.dtype, device=x.device)
    for i in range(width):
        for j in range(width):
            out = out + _tap(xp, Wm, Bm, S, depth, width, i, j, Ho, Wo)
    return out


def pair_target(truth, width, pad):
    """What F(x) is compared with (:431-432): the interior of truth for "valid", truth itself for "reflect"."""
    o = width // 2
    H, W = truth.shape[1], truth.shape[2]
    return truth[:, o:H - o, o:W - o] if pad == "valid" else truth


def pair_loss(out, truth, width, pad, sqrt_above_1):
    L = torch.mean((out - pair_target(truth, width, pad)) ** 2)
    if sqrt_above_1 and float(L.detach()) > 1.0:   # tf.cond(loss > 1., sqrt(loss), loss)
        L = torch.sqrt(L)
    return L


def pair_loss_and_grad(x, truth, theta, depth, width, pad="valid", sqrt_above_1=True, dtype=torch.float64):
    """(loss, d loss / d theta, plain MSE) by autograd.  x, truth: numpy or torch [B,H,W]; theta: numpy."""
    x = torch.as_tensor(np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x), dtype=dtype)
    truth = torch.as_tensor(np.asarray(truth.cpu() if isinstance(truth, torch.Tensor) else truth), dtype=dtype)
    th = torch.tensor(np.asarray(theta, np.float64), dtype=dtype, requires_grad=True)
    out = pair_forward(x, th, depth, width, pad)
    mse = float(torch.mean((out.detach() - pair_target(truth, width, pad)) ** 2))
    L = pair_loss(out, truth, width, pad, sqrt_above_1)
    L.backward()
    return float(L.detach()), th.grad.detach().numpy().astype(np.float64), mse


def pair_adam(theta0, batches, steps, depth, width, pad="valid", sqrt_above_1=True, lr0=0.01, total_steps=10000, beta1=0.5,
              beta2=0.999, eps=1e-8, dtype=torch.float64):
    """``steps`` steps of TF's Adam from theta0 on batches[(t-1) % len(batches)] = (x, truth).  Returns (theta, losses, mses)
    with the loss of every step taken before its update.  dtype float32 keeps theta / m / v and the objective in float32 (an
    emulation of a float32 trainer; the schedule stays in double, as on the device)."""
    np_t = np.float64 if dtype == torch.float64 else np.float32
    th = np.asarray(theta0, np_t).copy()
    m, v = np.zeros_like(th), np.zeros_like(th)
    losses, mses = [], []
    for t in range(1, steps + 1):
        x, truth = batches[(t - 1) % len(batches)]
        L, g, mse = pair_loss_and_grad(x, truth, th, depth, width, pad, sqrt_above_1, dtype)
        g = g.astype(np_t)
        losses.append(L)
        mses.append(mse)
        lr = np_t(lr0 * (1.0 - t / (total_steps + 1)))
        lr_t = np_t(float(lr) * math.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t))
        m = np_t(beta1) * m + np_t(1.0 - np_t(beta1)) * g
        v = np_t(beta2) * v + np_t(1.0 - np_t(beta2)) * g * g
        th = th - lr_t * m / (np.sqrt(v) + np_t(eps))
    return th, np.asarray(losses), np.asarray(mses)


def pair_loss_loop(x, truth, theta, depth, width, pad="valid", sqrt_above_1=True):
    """The paired loss by a literal loop over images, output pixels and taps in Python floats (doubles)."""
    x, truth, theta = np.asarray(x, np.float64), np.asarray(truth, np.float64), np.asarray(theta, np.float64)
    B, H, W = x.shape
    o, n = width // 2, len(sym_pairs(width))
    cls = tap_classes(width)
    sig = lambda z: 1.0 / (1.0 + math.exp(-z))

    def refl(i, size):
        i = -i if i < 0 else i
        return 2 * size - 2 - i if i >= size else i

    rows = range(H - width + 1) if pad == "valid" else range(H)
    cols = range(W - width + 1) if pad == "valid" else range(W)
    total, count = 0.0, 0
    for b in range(B):
        for r in rows:
            for c in cols:
                out = 0.0
                for i in range(width):
                    for j in range(width):
                        k = cls[i * width + j]
                        if pad == "valid":
                            v = x[b, r + i, c + j]
                            tr, tc = r + o, c + o
                        else:
                            v = x[b, refl(r + i - o, H), refl(c + j - o, W)]
                            tr, tc = r, c
                        f = theta[k] * v
                        for l in range(1, depth):
                            f = theta[l * n + k] * (theta[(2 * depth - 1) * n + l - 1] * sig(f + theta[depth * n + (l - 1) * n + k]))
                        out += f
                total += (out - truth[b, tr, tc]) ** 2
                count += 1
    L = total / count
    return math.sqrt(L) if (sqrt_above_1 and L > 1.0) else L


def make_pairs_ref(a, b, draws, patch=20):
    """autoencoder_train-val-test.py:35-55 in float64 for stacks a, b [N,H,W] and draws [N,2] = (i, j): each image rescaled by
    (img - min) / (mean - min), the patch at (i, j) of both, and 0.5 in both where either holds a non-finite value (the paired
    trainer's record_parser).  Returns (x, t) float64 [N,patch,patch]."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    N = a.shape[0]
    x, t = np.empty((N, patch, patch)), np.empty((N, patch, patch))
    with np.errstate(all="ignore"):
        for n in range(N):
            i, j = int(draws[n][0]), int(draws[n][1])
            pats = []
            for img in (a[n], b[n]):
                c = np.min(img)
                m = np.mean(img) - c
                pats.append(((img - c) / m)[i:i + patch, j:j + patch])
            if not (np.isfinite(pats[0]).all() and np.isfinite(pats[1]).all()):
                pats = [np.full((patch, patch), 0.5), np.full((patch, patch), 0.5)]
            x[n], t[n] = pats
    return x, t


def d4_kernel(centre, edge, corner):
    """A D4-symmetric 3 x 3 kernel from its three make_layer scalars (theta of a (1, 3) filter: classes (0,0), (1,0), (1,1))."""
    return np.array([[corner, edge, corner], [edge, centre, edge], [corner, edge, corner]], np.float64)


def apply_valid_3x3(x, k):
    """[B,H,W] float64 -> [B,H-2,W-2], correlation with k (what pair_forward computes for a depth-1 width-3 filter)."""
    x = np.asarray(x, np.float64)
    H, W = x.shape[1], x.shape[2]
    return sum(k[i, j] * x[:, i:i + H - 2, j:j + W - 2] for i in range(3) for j in range(3))
