#!/usr/bin/env python3
"""Times emdenoise.diversity (csrc/diversity.hip) on one GPU:

    python tools/diversity_bench.py [--steps K] [--warmup W] [--out profiles/diversity_bench.json]

With HIP events after warm-up, the median, the minimum and the maximum of K calls: ``gram_ssd_pairs`` for 8 pairs over 9 images of
2048 x 2048 (the reference's micrographs) and for 32 pairs over 33 images of 512 x 512, and ``row_distances`` of [4,2048,2048].  Beside
each, in the same process on the same GPU, alternating: (i) the same result composed from torch in float32 -- ``x @ x.T``, the three
elementwise steps of the script's ``gram``, and for a pair the difference, its square and ``mean`` -- once as the script does it (two
products a pair) and once with every image's matrix formed a single time and kept (the stronger baseline: 9 products instead of 16);
(ii) a device-to-device copy of the bytes the call must move (the stack once; for ``row_distances`` also the matrices it writes).

The rate is quoted on the triangular count, the products the symmetric result needs: images x H (H + 1) / 2 x W multiply-adds, two
images a pair, against the 157.3 TF float32 matrix peak.  It is the whole call over its operations, launches included, not a
kernel's share of peak.  At 2048 x 2048 the distance of both float32 routes from the torch composition in float64 is recorded (not
asserted)."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_TF = 157.3


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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diversity_bench.json"))
    a = ap.parse_args()
    import torch

    from emdenoise import diversity

    assert torch.cuda.is_available(), "diversity_bench needs a GPU"
    dev = torch.device("cuda", 0)
    rows = []

    def images(B, H, W, seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        return torch.poisson(torch.rand((B, H, W), device=dev, generator=g) * 300.0 + 20.0, generator=g) / 400.0

    def gram(x):                                                   # the script's gram, in x's dtype; [H,W] or batched [B,H,W]
        n = (x * x).sum(dim=-1)
        d = x @ x.transpose(-1, -2)
        d *= -2
        d += n.unsqueeze(-1)
        d += n.unsqueeze(-2)
        return d

    def torch_pairs(x, pairs):                                     # as the script: two products a pair
        return torch.stack([((gram(x[i]) - gram(x[j])) ** 2).mean() for i, j in pairs])

    def torch_pairs_kept(x, pairs):                                # every image's matrix once
        used = sorted({int(k) for p in pairs for k in p})
        D = {k: gram(x[k]) for k in used}
        return torch.stack([((D[i] - D[j]) ** 2).mean() for i, j in pairs])

    def copy_us(nbytes):
        n = int(nbytes // 8)
        src, dst = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
        us = timed(lambda: dst.copy_(src), a.steps, a.warmup)[0]
        del src, dst
        return us

    def row(name, shape, products, ours, composed, nbytes, extra=None):
        B, H, W = shape
        flop = 2.0 * products * (H * (H + 1) // 2) * W
        us, us_min, us_max = timed(ours, a.steps, a.warmup)
        r = {"what": name, "shape": list(shape), "us": round(us, 1), "us_min": round(us_min, 1), "us_max": round(us_max, 1)}
        for label, fn in composed:
            tus, tus_min, tus_max = timed(fn, a.steps, a.warmup)
            r[f"{label}_us"], r[f"{label}_us_min"], r[f"{label}_us_max"] = round(tus, 1), round(tus_min, 1), round(tus_max, 1)
            r[f"{label}_over_ours"] = round(tus / us, 2)
        us2 = timed(ours, a.steps, 1)[0]                            # again after the others: the spread between two runs
        cus = copy_us(nbytes)
        r.update({"us_second_run": round(us2, 1), "triangular_flop": flop, "TF_per_s": round(flop / (us * 1e-6) / 1e12, 1),
                  "fraction_of_f32_matrix_peak": round(flop / (us * 1e-6) / 1e12 / PEAK_TF, 3), "bytes_moved_by_design": int(nbytes),
                  "same_bytes_copy_us": round(cus, 1)})
        r.update(extra or {})
        rows.append(r)
        print(json.dumps(r), flush=True)

    for (B, H, W), P in (((9, 2048, 2048), 8), ((33, 512, 512), 32)):
        x = images(B, H, W, seed=H)
        pairs = diversity.pair_schedule(B, P)
        pd = torch.from_numpy(pairs).to(dev)
        plist = [tuple(int(k) for k in p) for p in pairs]
        extra = {}
        if H == 2048:
            want = torch_pairs_kept(x.double(), plist).cpu().numpy()
            got = diversity.gram_ssd_pairs(x, pd)[0].cpu().numpy()
            comp = torch_pairs(x, plist).double().cpu().numpy()
            extra = {"largest_relative_distance_from_float64": float(np.abs(got / want - 1).max()),
                     "torch_float32_largest_relative_distance_from_float64": float(np.abs(comp / want - 1).max())}
        row(f"gram_ssd_pairs, {P} pairs", (B, H, W), 2 * P, lambda: diversity.gram_ssd_pairs(x, pd),
            [("torch_two_products_a_pair", lambda: torch_pairs(x, plist)), ("torch_matrices_kept", lambda: torch_pairs_kept(x, plist))],
            4.0 * B * H * W, extra)
        del x
        torch.cuda.empty_cache()

    B, H, W = 4, 2048, 2048
    x = images(B, H, W, seed=7)
    want = gram(x.double())
    rel = lambda d: float(torch.linalg.norm(d.double() - want) / torch.linalg.norm(want))
    extra = {"rel_l2_from_float64": rel(diversity.row_distances(x)),
             "torch_float32_rel_l2_from_float64": rel(gram(x))}
    del want
    row("row_distances", (B, H, W), B, lambda: diversity.row_distances(x),
        [("torch_composed", lambda: gram(x))], 4.0 * B * H * W + 4.0 * B * H * H, extra)

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""),
                   "steps": a.steps, "warmup": a.warmup, "f32_matrix_peak_TF": PEAK_TF, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
