#!/usr/bin/env python3
"""Times emdenoise.focus (csrc/focus.hip) on one GPU:

    python tools/focus_bench.py [--steps K] [--warmup W] [--out profiles/focus_bench.json]

With HIP events after warm-up, the median, the minimum and the maximum of K calls: ``fresnel_quantifier`` (rectified, ksize 3) and
``image_entropy`` (plain and normalize=True) at [15,2048,2048] (the reference's ``stack_size``) and [32,512,512], and ``autofocus`` of
15 x 2048^2.  Beside each, in the same process: (i) a device-to-device copy that moves the same number of bytes as the call must
read, and the call's rate as a fraction of that copy's; (ii) the same result composed from torch on the same GPU -- for the focus
measure ``F.pad(reflect)`` + ``conv2d``, the mean, the mask and the masked moments in float64, batched (no gather: the stronger
baseline of the two); for the entropy ``torch.histc`` per image (it is not batched) and the entropy formula.

Bytes the calls must read, per pixel: the rectified focus measure 12 (three passes over the float32 stack: the mean, the set's mean,
the moments), the plain entropy 4, the normalized entropy 12 (mean, std, histogram).  What they write is a handful of doubles."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn, steps, warmup):
    """(median, min, max) microseconds of fn() over `steps` calls, each between its own pair of HIP events."""
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "focus_bench.json"))
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F

    from emdenoise import focus

    dev = torch.device("cuda", 0)
    rows = []
    k3 = torch.tensor([[2.0, 0.0, 2.0], [0.0, -8.0, 0.0], [2.0, 0.0, 2.0]], device=dev).reshape(1, 1, 3, 3)

    def images(B, H, W, seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        return torch.poisson(torch.rand((B, H, W), device=dev, generator=g) * 300.0 + 20.0, generator=g) / 400.0

    def copy_us(nbytes):
        n = int(nbytes // 8)
        src, dst = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
        us = timed(lambda: dst.copy_(src), a.steps, a.warmup)[0]
        del src, dst
        return us

    def torch_fresnel(x):
        L = F.conv2d(F.pad(x[:, None], (1, 1, 1, 1), mode="reflect"), k3)[:, 0].double()
        mask = L >= L.mean((1, 2), keepdim=True)
        n = mask.sum((1, 2))
        mean = torch.where(mask, L, 0.0).sum((1, 2)) / n
        d2 = torch.where(mask, L - mean[:, None, None], 0.0) ** 2
        m2, m4 = d2.sum((1, 2)) / n, (d2 * d2).sum((1, 2)) / n
        return m4 / (m2 * m2) - 3.0

    def torch_entropy(x, normalize, bins=256, eps=1e-6):
        out = []
        for img in x:
            if normalize:
                img = 0.15 * (img.double() - img.double().mean()) / img.double().std(unbiased=False) + 0.5
                img = img.float()
            p = torch.histc(img, bins=bins, min=0.0, max=1.0).double() + eps
            p = p / p.sum()
            out.append(-(p * torch.log2(p)).sum())
        return torch.stack(out)

    def row(name, shape, ours, composed, bytes_per_px):
        B, H, W = shape
        nbytes = float(bytes_per_px) * B * H * W
        us, us_min, us_max = timed(ours, a.steps, a.warmup)
        tus, tus_min, tus_max = timed(composed, a.steps, a.warmup)
        us2 = timed(ours, a.steps, 1)[0]                                     # again after the other: the spread between two runs
        cus = copy_us(nbytes)
        r = {"what": name, "shape": list(shape), "us": round(us, 1), "us_min": round(us_min, 1), "us_max": round(us_max, 1),
             "us_second_run": round(us2, 1), "bytes_read_by_design": int(nbytes), "TB_per_s": round(nbytes / (us * 1e-6) / 1e12, 3),
             "same_bytes_copy_us": round(cus, 1), "fraction_of_copy_rate": round(cus / us, 3), "torch_composed_us": round(tus, 1),
             "torch_composed_us_min": round(tus_min, 1), "torch_composed_us_max": round(tus_max, 1),
             "torch_composed_over_ours": round(tus / us, 2)}
        rows.append(r)
        print(json.dumps(r), flush=True)

    for shape in ((15, 2048, 2048), (32, 512, 512)):
        x = images(*shape, seed=shape[1])
        k_ours, k_torch = focus.fresnel_quantifier(x).cpu().numpy(), torch_fresnel(x).cpu().numpy()
        print(f"fresnel_quantifier {shape}: largest relative distance from the torch composition {np.abs(k_ours / k_torch - 1).max():.2e}", flush=True)
        row("fresnel_quantifier (rectified, ksize 3)", shape, lambda: focus.fresnel_quantifier(x), lambda: torch_fresnel(x), 12)
        row("image_entropy", shape, lambda: focus.image_entropy(x), lambda: torch_entropy(x, False), 4)
        row("image_entropy (normalize)", shape, lambda: focus.image_entropy(x, normalize=True), lambda: torch_entropy(x, True), 12)
        if shape[0] == 15:
            z = torch.linspace(-7.0, 7.0, 15, dtype=torch.float64, device=dev)
            row("autofocus", shape, lambda: focus.autofocus(x, z), lambda: torch_fresnel(x), 12)
        del x
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""),
                   "steps": a.steps, "warmup": a.warmup, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
