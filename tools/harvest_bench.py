#!/usr/bin/env python3
"""Times the harvester (csrc/harvest.hip) on one GPU:

    python tools/harvest_bench.py [--steps K] [--warmup W] [--out profiles/harvest_bench.json] [--no-host]

With HIP events after warm-up: ``box_resize`` 4096 x 4096 -> 2048 and 2672 x 4008 -> 2048 (batches of 4), ``image_stats`` at
[8,2048,2048], and ``img_params`` of one 2672 x 4008 image (which ends in its one read-back of three rows of statistics).  Beside
each, in the same process: (i) a device-to-device copy that moves the same number of bytes as the call's traffic by design, and
the call's rate as a fraction of that copy's; (ii) the numpy restatement of tests/harvest_ref.py on the host for ONE image.

Bytes by design: the resize reads the d x d crop and writes S x S (4 B each); the statistics read the image four times (the tile
pass; the centred moments with the selection's second pass; two more selection passes), 16 B per pixel; scale01 8 B per pixel;
img_params is statistics of the raw image, the resize, statistics, scale01 and statistics of the S x S image.

The frequency fields (csrc/fft.hip): ``rfft2`` and ``freq_stats`` at [8,2048,2048] and ``img_params(freq=True)`` of
the 2672 x 4008 image, each also beside ``torch.fft.rfft2`` in float64 on the same GPU (``torch_rfft2_f64_us``; for freq_stats and
img_params it is the transform alone, which they contain).  Bytes by design per pixel: the row pass reads 4 and writes 8 (the half
spectrum, complex double), the column pass reads 8 and writes 8 (rfft2) or 4 (|F|), the profile reads 4."""
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
    from tests import fft_ref as FR
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

    def row(name, shape, ours, host, nbytes, per_image, torch_fft=None):
        us, us_min = timed(ours, a.steps, a.warmup)
        cus = copy_us(nbytes)
        r = {"what": name, "shape": list(shape), "us": round(us, 1), "us_min": round(us_min, 1), "bytes": int(nbytes),
             "TB_per_s": round(nbytes / (us * 1e-6) / 1e12, 3), "same_bytes_copy_us": round(cus, 1), "fraction_of_copy_rate": round(cus / us, 3)}
        if torch_fft is not None:
            r["torch_rfft2_f64_us"] = round(timed(torch_fft, a.steps, a.warmup)[0], 1)
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
    x64 = x.double()
    torch_fft = lambda: torch.fft.rfft2(x64)
    row("rfft2", (8, S, S), lambda: harvest.rfft2(x), lambda: np.fft.rfft2(one.astype(np.float64)), 28.0 * 8 * S * S, 8, torch_fft)
    row("freq_stats", (8, S, S), lambda: harvest.freq_stats(x), lambda: FR.freq_stats(one), 28.0 * 8 * S * S, 8, torch_fft)
    del x, x64
    torch.cuda.empty_cache()

    H, W = 2672, 4008
    img = images(1, H, W, 3)[0]
    one = img.cpu().numpy()

    def host_img_params():
        small = R.box_resize(one, S)
        R.image_stats(one), R.image_stats(small), R.image_stats(R.scale01(small))

    row("img_params (one image, with its read-back)", (H, W), lambda: harvest.img_params(img, S), host_img_params,
        16.0 * H * W + 4.0 * (H * H + S * S) + (16.0 + 8.0 + 16.0) * S * S, 1)

    def host_img_params_freq():
        host_img_params()
        FR.freq_stats(R.box_resize(one, S))

    small64 = harvest.box_resize(img, S).double()
    row("img_params(freq=True) (one image, with its read-back)", (H, W), lambda: harvest.img_params(img, S, freq=True),
        host_img_params_freq, 16.0 * H * W + 4.0 * (H * H + S * S) + (16.0 + 8.0 + 16.0 + 28.0) * S * S, 1,
        lambda: torch.fft.rfft2(small64))

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""),
                   "steps": a.steps, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
