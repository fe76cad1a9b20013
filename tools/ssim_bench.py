#!/usr/bin/env python3
"""Times the image-quality metrics (csrc/ssim.hip) on one GPU:

    python tools/ssim_bench.py [--steps K] [--warmup W] [--out profiles/ssim_bench.json] [--no-trainer]

At [32,512,512,1] and [8,2048,2048,1], with HIP events after warm-up: ``ssim`` (means only), ``ssim_loss`` with its gradient,
``ms_ssim`` and ``psnr``; beside them, in the same process, (i) a device-to-device copy of the same number of bytes -- the
bandwidth yardstick of DESIGN.md 5 -- and (ii) the same quantities through torch.nn.functional.conv2d / autograd on the GPU, "what
a user would otherwise write" (in this tool only, never in the package).  Reported: microseconds, the fraction of the copy rate
on the algorithmic bytes (8 B/px forward; the gradient 8 B/px more for the read-modify-write of dout plus 24 B/px for the three
derivative planes written and read back), and the ratio to (ii).  One more row times DenoiserTrainer.train_step at [8,512,512,1]
in bench.py's form (batched per-image towers, captured graph) with the SSIM term off and on, alternating in one process."""
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
    """Median and minimum microseconds of fn() over `steps` calls, each between its own pair of HIP events."""
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
    return float(np.median(ts)), float(np.min(ts))


def torch_ssim_map(x, y, win):
    import torch.nn.functional as F

    C1, C2 = 0.01 ** 2, 0.03 ** 2
    mu1, mu2 = F.conv2d(x, win), F.conv2d(y, win)
    s1 = F.conv2d(x * x, win) - mu1 * mu1
    s2 = F.conv2d(y * y, win) - mu2 * mu2
    s12 = F.conv2d(x * y, win) - mu1 * mu2
    cs = (2 * s12 + C2) / (s1 + s2 + C2)
    return (2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1) * cs, cs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssim_bench.json"))
    ap.add_argument("--no-trainer", action="store_true")
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F

    import emdenoise
    from emdenoise import metrics
    from tests.synth_inputs import synthetic_pair

    dev = torch.device("cuda", 0)
    rows = []
    for (B, S) in ((32, 512), (8, 2048)):
        lq, hq = synthetic_pair(1, S, S, seed=3)
        x = torch.from_numpy(lq).to(dev).repeat(B, 1, 1, 1).contiguous()
        y = torch.from_numpy(hq).to(dev).repeat(B, 1, 1, 1).contiguous()
        x += 0.01 * torch.rand_like(x)
        npx = B * S * S
        dout = torch.zeros_like(x)
        src, dst = torch.empty(npx * 2, dtype=torch.float32, device=dev), torch.empty(npx * 2, dtype=torch.float32, device=dev)
        copy_us, _ = timed(lambda: dst.copy_(src), a.steps, a.warmup)          # 8 B/px read + 8 B/px written
        copy_rate = 16.0 * npx / (copy_us * 1e-6)
        xn, yn = x.permute(0, 3, 1, 2).contiguous(), y.permute(0, 3, 1, 2).contiguous()
        g = torch.from_numpy(metrics.gaussian_taps()).to(dev)
        win = torch.outer(g, g)[None, None]
        pool = lambda t: F.avg_pool2d(t, 2, 2, ceil_mode=True, count_include_pad=False)

        def t_ssim():
            return torch_ssim_map(xn, yn, win)[0].mean()

        def t_loss():
            xr = xn.detach().requires_grad_(True)
            (1.0 - torch_ssim_map(xr, yn, win)[0].mean()).backward()
            dout.view_as(xr).add_(xr.grad)

        def t_ms():
            p, q, mcs = xn, yn, []
            for l in range(5):
                m, cs = torch_ssim_map(p, q, win)
                mcs.append(cs.mean())
                p, q = pool(p), pool(q)
            w = torch.tensor(metrics.MS_SSIM_WEIGHTS, device=dev)
            return torch.prod(torch.stack(mcs[:4]) ** w[:4]) * m.mean() ** w[4]

        def t_psnr():
            return 10.0 * torch.log10(1.0 / ((xn - yn) ** 2).mean())

        cases = [("ssim", lambda: emdenoise.ssim(x, y), t_ssim, 8.0),
                 ("ssim_loss", lambda: emdenoise.ssim_loss(x, y, dout, scale=0.0), t_loss, 8.0 + 8.0 + 24.0),
                 ("ms_ssim", lambda: emdenoise.ms_ssim(x, y), t_ms, 8.0 * (1 + 4.0 / 3.0 * (1 - 0.25 ** 4)) + 8.0 / 3.0 * (1 - 0.25 ** 4)),
                 ("psnr", lambda: emdenoise.psnr(x, y), t_psnr, 8.0)]
        for name, ours, theirs, bpp in cases:
            us, us_min = timed(ours, a.steps, a.warmup)
            tus, _ = timed(theirs, max(3, a.steps // 3), 2)
            r = {"what": name, "shape": [B, S, S, 1], "us": round(us, 1), "us_min": round(us_min, 1), "bytes_per_px": round(bpp, 2),
                 "copy_us_same_px": round(copy_us, 1), "copy_TB_per_s": round(copy_rate / 1e12, 3),
                 "fraction_of_copy_rate": round(bpp * npx / (us * 1e-6) / copy_rate, 3), "torch_conv2d_us": round(tus, 1),
                 "speedup_over_torch": round(tus / us, 2)}
            rows.append(r)
            print(json.dumps(r), flush=True)
        del x, y, xn, yn, dout, src, dst
        torch.cuda.empty_cache()

    if not a.no_trainer:
        from emdenoise import denoiser as D
        from emdenoise import trainer as TR

        lq, hq = synthetic_pair(8, 512, 512, seed=11)
        x, t = torch.from_numpy(lq).to(dev), torch.from_numpy(hq).to(dev)
        tr = TR.DenoiserTrainer(D.synthetic_weights(variant="Dprime"), dev)
        step = lambda w: tr.train_step(x, t, tower_batch=1, streams=8, graph=True, batched=True, ssim_weight=w)
        for w in (0.0, 1.0):
            for _ in range(2):
                step(w)
        torch.cuda.synchronize()
        ts = {0.0: [], 1.0: []}
        for _ in range(max(4, a.steps // 3)):
            for w in (0.0, 1.0):          # alternating: both legs see the same clocks
                us, _ = timed(lambda: step(w), 1, 0)
                ts[w].append(us)
        r = {"what": "train_step", "shape": [8, 512, 512, 1], "ssim_off_us": round(float(np.median(ts[0.0])), 1),
             "ssim_on_us": round(float(np.median(ts[1.0])), 1),
             "term_us": round(float(np.median(ts[1.0]) - np.median(ts[0.0])), 1)}
        rows.append(r)
        print(json.dumps(r), flush=True)

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
