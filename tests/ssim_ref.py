"""Restatement of the reference's structural-similarity functions for the tests (misc_py/denoiser-multi-gpu.py:124-139
_tf_fspecial_gauss, :142-167 tf_ssim, :170-192 tf_ms_ssim, and the loss term of :775), with torch-CPU conv2d / autograd, written
from those lines.  dtype=torch.float64 is the reference the device results are checked against; dtype=torch.float32 is used only
as a yardstick: its own distance from the float64 result sets the tolerances."""
import numpy as np
import torch
import torch.nn.functional as F

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)   # :171
K1, K2, L = 0.01, 0.03, 1                             # :144-146


def fspecial_gauss(size=11, sigma=1.5, dtype=torch.float64):
    """:124-139: np.mgrid[-size//2 + 1:size//2 + 1, ...] -> exp(-(x^2 + y^2) / (2 sigma^2)) / sum, [size, size]."""
    x_data, y_data = np.mgrid[-size // 2 + 1:size // 2 + 1, -size // 2 + 1:size // 2 + 1]
    x = torch.tensor(x_data, dtype=dtype)
    y = torch.tensor(y_data, dtype=dtype)
    g = torch.exp(-((x ** 2 + y ** 2) / (2.0 * sigma ** 2)))
    return g / g.sum()


def _nchw(a, dtype):
    """[B,H,W,1] / [B,H,W] / [H,W] (numpy or torch) -> torch [B,1,H,W] of dtype."""
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))
    t = t.to(dtype)
    if t.dim() == 4:
        t = t[..., 0]
    elif t.dim() == 2:
        t = t[None]
    return t[:, None]


def ssim_t(img1, img2, cs_map=False, mean_metric=True, size=11, sigma=1.5):
    """tf_ssim (:142-167) on torch [B,1,H,W] tensors (differentiable); maps come back as [B,1,H-size+1,W-size+1]."""
    window = fspecial_gauss(size, sigma, img1.dtype)[None, None]
    C1 = (K1 * L) ** 2
    C2 = (K2 * L) ** 2
    mu1 = F.conv2d(img1, window)
    mu2 = F.conv2d(img2, window)
    mu1_sq = mu1 * mu1
    mu2_sq = mu2 * mu2
    mu1_mu2 = mu1 * mu2
    sigma1_sq = F.conv2d(img1 * img1, window) - mu1_sq
    sigma2_sq = F.conv2d(img2 * img2, window) - mu2_sq
    sigma12 = F.conv2d(img1 * img2, window) - mu1_mu2
    ssim_map = ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))
    if cs_map:
        value = (ssim_map, (2.0 * sigma12 + C2) / (sigma1_sq + sigma2_sq + C2))
    else:
        value = ssim_map
    if mean_metric:
        value = tuple(v.mean() for v in value) if cs_map else value.mean()
    return value


def avg_pool_same_t(x):
    """tf.nn.avg_pool(x, [1,2,2,1], [1,2,2,1], 'SAME') on [B,1,H,W]: windows that hang over the end hold the valid elements only
    and are divided by their number."""
    return F.avg_pool2d(x, 2, 2, ceil_mode=True, count_include_pad=False)


def ms_ssim_t(img1, img2, level=5, per_image=False):
    """tf_ms_ssim (:170-192).  -> (value, mssim [level], mcs [level]); per_image: the same formula on each image's own means
    (value [B], mssim / mcs [level, B])."""
    weight = torch.tensor(WEIGHTS, dtype=img1.dtype)
    mssim, mcs = [], []
    for _ in range(level):
        ssim_map, cs_map = ssim_t(img1, img2, cs_map=True, mean_metric=False)
        if per_image:
            mssim.append(ssim_map.mean(dim=(1, 2, 3)))
            mcs.append(cs_map.mean(dim=(1, 2, 3)))
        else:
            mssim.append(ssim_map.mean())
            mcs.append(cs_map.mean())
        img1 = avg_pool_same_t(img1)
        img2 = avg_pool_same_t(img2)
    mssim = torch.stack(mssim, 0)
    mcs = torch.stack(mcs, 0)
    w = weight.view(-1, *([1] * (mcs.dim() - 1)))
    value = torch.prod(mcs[0:level - 1] ** w[0:level - 1], dim=0) * (mssim[level - 1] ** w[level - 1])
    return value, mssim, mcs


def ssim(a, b, dtype=torch.float64, size=11, sigma=1.5):
    """numpy in, numpy out: {"ssim_map", "cs_map" [B,Hm,Wm], "means" [B,2] (ssim, cs per image), "batch" [2]}."""
    s, c = ssim_t(_nchw(a, dtype), _nchw(b, dtype), cs_map=True, mean_metric=False, size=size, sigma=sigma)
    means = torch.stack([s.mean(dim=(1, 2, 3)), c.mean(dim=(1, 2, 3))], 1)
    return {"ssim_map": s[:, 0].numpy(), "cs_map": c[:, 0].numpy(), "means": means.numpy(),
            "batch": np.array([float(s.mean()), float(c.mean())])}


def ssim_loss(x, y, dtype=torch.float64, per_image=False, size=11, sigma=1.5):
    """L = 1 - tf_ssim(x, y) (:775) and dL/dx by autograd.  per_image: every image its own loss, -> (loss [B], grad [B,H,W]) with
    grad[b] = dL_b/dx[b]; else (loss scalar of the batch mean, grad [B,H,W])."""
    xt = _nchw(x, dtype).clone().requires_grad_(True)
    yt = _nchw(y, dtype)
    m = ssim_t(xt, yt, mean_metric=False, size=size, sigma=sigma)
    loss = 1.0 - (m.mean(dim=(1, 2, 3)) if per_image else m.mean())
    loss.sum().backward()
    return loss.detach().numpy(), xt.grad[:, 0].numpy()


def ms_ssim(a, b, dtype=torch.float64, level=5, per_image=False):
    v, mssim, mcs = ms_ssim_t(_nchw(a, dtype), _nchw(b, dtype), level, per_image)
    return v.numpy(), mssim.numpy(), mcs.numpy()


def psnr(a, b, data_range=1.0, per_image=False):
    a64 = np.asarray(a, np.float64).reshape(np.shape(a)[0], -1)
    b64 = np.asarray(b, np.float64).reshape(np.shape(b)[0], -1)
    mse = ((a64 - b64) ** 2).mean(axis=1)
    if not per_image:
        mse = mse.mean()
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(data_range ** 2 / mse)
