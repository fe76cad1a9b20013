#!/usr/bin/env python3
"""Times emdenoise.dose (csrc/dose.hip) on one GPU:

    python tools/dose_bench.py [--steps K] [--warmup W] [--out profiles/dose_bench.json]

With HIP events after warm-up, the median, the minimum and the maximum of K calls of ``cdf``, ``sample_counts`` (at 2, 16 and 64
electrons a pixel) and ``dose_series`` (the reference's levels 2 .. 64, counts and 16-bit rescale) at [1,2048,2048] (2.7e8 draws at
64 a pixel) and [32,512,512], and of the draw launch alone on a CDF that is already there.  Beside each, in the same process: (i) a
device-to-device copy that moves the bytes the call must move at the least, and the call's rate as a fraction of that copy's; (ii)
the same kind of result composed from torch on the same GPU, image by image: ``cumsum`` in float64, ``rand`` in float64 scaled by
the total, ``searchsorted(right=True)``, ``bincount`` (for the series one such round per level on the level's own draws, and a
``cumsum`` over the levels).  Draws per microsecond are reported for both.

Bytes a call must move, per pixel: the CDF 20 (three reads of the float32 image: the maximum, the tiles' sums, the scan; one int64
written); the counts 4 more for every plane zeroed; the series 8 more per plane for the cumulation and 8 per plane for a rescale.
Per draw 12 are added (the last CDF entry read, one int32 added to): a floor, since the search reads more than one entry."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LEVELS = (2, 4, 8, 16, 32, 64)


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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dose_bench.json"))
    a = ap.parse_args()
    import torch

    from emdenoise import dose

    dev = torch.device("cuda", 0)
    rows = []

    def images(B, H, W, seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        return torch.rand((B, H, W), device=dev, generator=g) * 300.0 + 20.0

    def copy_us(nbytes):
        n = int(nbytes // 8)
        src, dst = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
        us = timed(lambda: dst.copy_(src), a.steps, a.warmup)[0]
        del src, dst
        return us

    def torch_cdf(x):
        w = torch.where(torch.isfinite(x) & (x > 0), x, 0.0).double().flatten(1)
        return torch.cumsum(w / w.amax(1, keepdim=True), 1)

    def torch_counts(c, draws):
        """One image's float64 CDF [n] -> int64 counts [n] of `draws` uniform draws."""
        u = torch.rand(draws, dtype=torch.float64, device=dev) * c[-1]
        return torch.bincount(torch.searchsorted(c, u, right=True).clamp_(max=c.numel() - 1), minlength=c.numel())

    def torch_sample(x, draws):
        return torch.stack([torch_counts(c, draws) for c in torch_cdf(x)])

    def torch_series(x, bounds):
        return torch.stack([torch.cumsum(torch.stack([torch_counts(c, bounds[k + 1] - bounds[k]) for k in range(len(bounds) - 1)]), 0)
                            for c in torch_cdf(x)])

    def row(name, shape, draws, ours, composed, nbytes):
        us, us_min, us_max = timed(ours, a.steps, a.warmup)
        tus, tus_min, tus_max = timed(composed, a.steps, a.warmup) if composed else (None, None, None)
        us2 = timed(ours, a.steps, 1)[0]                                     # again after the other: the spread between two runs
        cus = copy_us(nbytes)
        r = {"what": name, "shape": list(shape), "draws": int(draws), "us": round(us, 1), "us_min": round(us_min, 1), "us_max": round(us_max, 1),
             "us_second_run": round(us2, 1), "bytes_moved_by_design": int(nbytes), "same_bytes_copy_us": round(cus, 1),
             "fraction_of_copy_rate": round(cus / us, 4), "draws_per_us": round(draws / us, 1) if draws else None}
        if composed:
            r.update({"torch_composed_us": round(tus, 1), "torch_composed_us_min": round(tus_min, 1), "torch_composed_us_max": round(tus_max, 1),
                      "torch_draws_per_us": round(draws / tus, 1) if draws else None, "torch_composed_over_ours": round(tus / us, 2)})
        rows.append(r)
        print(json.dumps(r), flush=True)

    for shape in ((1, 2048, 2048), (32, 512, 512)):
        B, H, W = shape
        n, px = H * W, B * H * W
        x = images(*shape, seed=H)
        row("cdf", shape, 0, lambda: dose.cdf(x), lambda: torch_cdf(x), 20 * px)
        c = dose.cdf(x)
        for avg in (2, 16, 64):
            D = avg * n
            row(f"sample_counts ({avg} a pixel)", shape, B * D, lambda: dose.sample_counts(x, D), lambda: torch_sample(x, D), 24 * px + 12 * B * D)
            planes = torch.zeros((B, 1, H, W), dtype=torch.int32, device=dev)
            row(f"the draw launch alone ({avg} a pixel)", shape, B * D, lambda: dose._draw_device(c, 0, 0, [0, D], planes), None, 12 * B * D)
            del planes
        bounds = [0] + [v * n for v in LEVELS]
        L = len(LEVELS)
        row("dose_series (2 .. 64, counts)", shape, B * bounds[-1], lambda: dose.dose_series(x, LEVELS), lambda: torch_series(x, bounds),
            (20 + 12 * L) * px + 12 * B * bounds[-1])
        row("dose_series (2 .. 64, uint16)", shape, B * bounds[-1], lambda: dose.dose_series(x, LEVELS, rescale="uint16"), None,
            (20 + 20 * L) * px + 12 * B * bounds[-1])
        del x, c
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""),
                   "steps": a.steps, "warmup": a.warmup, "tile": dose.TILE, "coarse": dose.COARSE, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
