#!/usr/bin/env python3
"""Times the classical baseline filters (csrc/filters.hip) on one GPU:

    python tools/filter_bench.py [--steps K] [--warmup W] [--out profiles/filter_bench.json] [--no-host]

At [32,512,512] and [8,2048,2048], with HIP events after warm-up: ``gaussian`` (3 / 1.5 and 11 / 1.5), ``median`` (3, 5),
``bilateral`` (d 5, 9), ``wiener`` (5: given and estimated noise) and ``tv_chambolle`` (50 iterations; also per iteration).  Beside
each, in the same process: (i) a device-to-device copy that moves the same number of bytes as the filter's algorithmic traffic --
the bandwidth yardstick of DESIGN.md 5 -- and, for the rows the bytes can bind (Gaussian 3, median 3, Wiener), the filter's rate as a
fraction of that copy's; Chambolle's iteration is set against a measured copy of an inner iteration's 20 B/px; (ii) scipy (or, for bilateral and
Chambolle, the numpy restatement of tests/filters_ref.py) on the host for ONE image of that size, "what a user would otherwise
run".  One more row times the whole ``baseline_table`` of the batch.  Algorithmic bytes per pixel: 8 (read x, write out) for the
one-launch filters; 12 for Wiener with the estimate (x is read twice); Chambolle 20 per inner iteration (x, two dual planes read,
two written), 12 for the first (nothing read but x) and 16 for the last (out instead of the planes)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

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


def host_us(fn, reps=1):
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e6


def tv_bytes_per_px(n_iter):
    if n_iter == 1:
        return 8.0
    return 12.0 + 16.0 + 20.0 * (n_iter - 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter_bench.json"))
    ap.add_argument("--no-host", action="store_true", help="skip the host (scipy / numpy) column")
    a = ap.parse_args()
    import torch

    import emdenoise
    from emdenoise import filters
    from tests import filters_ref as R
    from tests.synth_inputs import synthetic_pair

    dev = torch.device("cuda", 0)
    n_tv = 50
    rows = []
    for (B, S) in ((32, 512), (8, 2048)):
        lq, hq = synthetic_pair(1, S, S, seed=3)
        x = torch.from_numpy(lq[..., 0]).to(dev).repeat(B, 1, 1).contiguous()
        t = torch.from_numpy(hq[..., 0]).to(dev).repeat(B, 1, 1).contiguous()
        x += 0.01 * torch.rand_like(x)
        npx = B * S * S
        one = lq[0, :, :, 0].astype(np.float64)
        copies = {}

        def copy_us(bpp):
            """a device-to-device copy that moves bpp bytes per pixel of the batch in all (half read, half written)"""
            if bpp not in copies:
                n = int(npx * bpp / 8)
                src, dst = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
                copies[bpp] = timed(lambda: dst.copy_(src), a.steps, a.warmup)[0]
                del src, dst
            return copies[bpp]

        cases = [("gaussian 3/1.5", lambda: filters.gaussian(x, 1.5, 3), lambda: R.gaussian(one, 1.5, 3), 8.0),
                 ("gaussian 11/1.5", lambda: filters.gaussian(x, 1.5, 11), lambda: R.gaussian(one, 1.5, 11), 8.0),
                 ("median 3", lambda: filters.median(x, 3), lambda: R.median(one, 3), 8.0),
                 ("median 5", lambda: filters.median(x, 5), lambda: R.median(one, 5), 8.0),
                 ("bilateral 5", lambda: filters.bilateral(x, 5, 0.1, 1.5), lambda: R.bilateral(one, 5, 0.1, 1.5), 8.0),
                 ("bilateral 9", lambda: filters.bilateral(x, 9, 0.1, 1.5), lambda: R.bilateral(one, 9, 0.1, 1.5), 8.0),
                 ("wiener 5 given noise", lambda: filters.wiener(x, 5, 0.004), lambda: R.wiener(one, 5, 0.004), 8.0),
                 ("wiener 5 estimated noise", lambda: filters.wiener(x, 5), lambda: R.wiener(one, 5), 12.0),
                 (f"tv_chambolle {n_tv} iterations", lambda: filters.tv_chambolle(x, 0.1, n_tv), lambda: R.tv_chambolle(one, 0.1, n_tv),
                  tv_bytes_per_px(n_tv))]
        # the rows whose instruction count leaves the bytes as the bound: only they get a fraction of the copy rate
        byte_bound = ("gaussian 3/1.5", "median 3", "wiener 5 given noise", "wiener 5 estimated noise")
        for name, ours, host, bpp in cases:
            us, us_min = timed(ours, a.steps, a.warmup)
            r = {"what": name, "shape": [B, S, S], "us": round(us, 1), "us_min": round(us_min, 1), "bytes_per_px": round(bpp, 2),
                 "TB_per_s": round(bpp * npx / (us * 1e-6) / 1e12, 3)}
            if name.startswith("tv_chambolle"):
                # one inner iteration against a measured copy of its 20 B/px (the whole call's bytes do not fit one copy)
                cus = copy_us(20.0)
                r.update({"us_per_iteration": round(us / n_tv, 1), "copy_us_20_bytes_per_px": round(cus, 1),
                          "iteration_fraction_of_copy_rate": round(cus / (us / n_tv) * (bpp / n_tv) / 20.0, 3)})
            else:
                r["same_bytes_copy_us"] = round(copy_us(bpp), 1)
                if name in byte_bound:
                    r["fraction_of_copy_rate"] = round(copy_us(bpp) / us, 3)
            if not a.no_host:
                hus = host_us(host)
                r["host_one_image_us"] = round(hus, 1)
                r["host_per_image_over_ours"] = round(hus / (us / B), 1)
            rows.append(r)
            print(json.dumps(r), flush=True)
        us, us_min = timed(lambda: emdenoise.baseline_table(x, t), max(3, a.steps // 4), 1)
        r = {"what": "baseline_table (6 methods, mse + ssim each)", "shape": [B, S, S], "us": round(us, 1), "us_min": round(us_min, 1)}
        rows.append(r)
        print(json.dumps(r), flush=True)
        del x, t
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        # torch names an MI355X "AMD Radeon Graphics"; the architecture string says which chip it was
        json.dump({"device": torch.cuda.get_device_name(0), "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""),
                   "steps": a.steps, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
