#!/usr/bin/env python3
"""Times the harvester (csrc/harvest.hip) on one GPU:

    python tools/harvest_bench.py [--steps K] [--warmup W] [--out profiles/harvest_bench.json] [--no-host]

With HIP events after warm-up: ``box_resize`` 4096 x 4096 -> 2048 and 2672 x 4008 -> 2048 (batches of 4), ``image_stats`` at
[8,2048,2048], and ``img_params`` of one 2672 x 4008 image (which ends in its one read-back of three rows of statistics).  Beside
each, in the same process: (i) a device-to-device copy that moves the same number of bytes as the call's traffic by design, and
the call's rate as a fraction of that copy's; (ii) the numpy restatement of tests/harvest_ref.py on the host for ONE image.

Bytes by design: the resize reads the d x d crop and writes S x S (4 B each); the statistics read the image four times (the tile
pass; the centred moments with the selection's second pass; two more selection passes), 16 B per pixel; scale01 8 B per pixel;
img_params is statistics of the raw image, the resize, statistics, scale01 and statistics of the S x S image."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.filter_bench import host_us, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "harvest_bench.json"))
    ap.add_argument("--no-host", action="store_true", help="skip the host (numpy restatement) column")
    a = ap.parse_args()
    import torch

    from emdenoise import harvest
    from tests import harvest_ref as R

    dev = torch.device("cuda", 0)
    S = 2048
    rows = []

    def images(B, H, W, seed):
        """count-valued micrographs with an offset: negatives, zeros and duplicates, as a detector gives them"""
        g = torch.Generator(device=dev).manual_seed(seed)
        return torch.poisson(torch.rand((B, H, W), device=dev, generator=g) * 300.0 + 20.0, generator=g) - 25.0

    def copy_us(nbytes):
        n = int(nbytes // 8)
        src, dst = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
        us = timed(lambda: dst.copy_(src), a.steps, a.warmup)[0]
        del src, dst
        return us

    def row(name, shape, ours, host, nbytes, per_image):
        us, us_min = timed(ours, a.steps, a.warmup)
        cus = copy_us(nbytes)
        r = {"what": name, "shape": list(shape), "us": round(us, 1), "us_min": round(us_min, 1), "bytes": int(nbytes),
             "TB_per_s": round(nbytes / (us * 1e-6) / 1e12, 3), "same_bytes_copy_us": round(cus, 1), "fraction_of_copy_rate": round(cus / us, 3)}
        if not a.no_host:
            hus = host_us(host)
            r["host_one_image_us"] = round(hus, 1)
            r["host_per_image_over_ours"] = round(hus / (us / per_image), 1)
        rows.append(r)
        print(json.dumps(r), flush=True)

    for (B, H, W) in ((4, 4096, 4096), (4, 2672, 4008)):
        x = images(B, H, W, 1)
        d = min(H, W)
        one = x[0].cpu().numpy()
        row(f"box_resize {H} x {W} -> {S}", (B, H, W), lambda: harvest.box_resize(x, S), lambda: R.box_resize(one, S),
            4.0 * B * (d * d + S * S), B)
        del x
        torch.cuda.empty_cache()

    x = images(8, S, S, 2)
    one = x[0].cpu().numpy()
    row("image_stats", (8, S, S), lambda: harvest.image_stats(x), lambda: R.image_stats(one), 16.0 * 8 * S * S, 8)
    row("scale01 (statistics, then the rescale)", (8, S, S), lambda: harvest.scale01(x), lambda: R.scale01(one), 24.0 * 8 * S * S, 8)
    del x
    torch.cuda.empty_cache()

    H, W = 2672, 4008
    img = images(1, H, W, 3)[0]
    one = img.cpu().numpy()

    def host_img_params():
        small = R.box_resize(one, S)
        R.image_stats(one), R.image_stats(small), R.image_stats(R.scale01(small))

    row("img_params (one image, with its read-back)", (H, W), lambda: harvest.img_params(img, S), host_img_params,
        16.0 * H * W + 4.0 * (H * H + S * S) + (16.0 + 8.0 + 16.0) * S * S, 1)

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""),
                   "steps": a.steps, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
