#!/usr/bin/env python3
"""Times the wavelet transform and wavelet shrinkage (csrc/wavelet.hip) on one GPU:

    python tools/wavelet_bench.py [--steps K] [--warmup W] [--out profiles/wavelet_bench.json] [--no-host]

At [32,512,512] and [8,2048,2048], with HIP events after warm-up, for "db1" and "db2" at the default number of levels:
``wavedec2`` + ``waverec2``, ``denoise_wavelet`` with a given sigma and with the estimated one.  Beside each, in the same process:
(i) a device-to-device copy that moves the same number of bytes as the call's algorithmic traffic and the call's rate as a
fraction of that copy's; (ii) the numpy restatement of tests/wavelet_ref.py on the host for ONE image of that size.  One more row
times the seven-column ``baseline_table(reference_columns=True)`` of the batch.

Algorithmic bytes per pixel, with g = 1 + 1/4 + ... + 1/4^(levels-1) (a level reads its input once and writes four bands of a quarter
each, 8 B per input pixel; synthesis the reverse): transform pair 16 g; denoiser 16 g, plus 4 for the four selection passes over
dd_1 (a quarter of the pixels, 4 B each, four times) when sigma is estimated."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wavelet_bench.json"))
    ap.add_argument("--no-host", action="store_true", help="skip the host (numpy restatement) column")
    a = ap.parse_args()
    import torch

    import emdenoise
    from emdenoise import filters
    from tests import wavelet_ref as R
    from tests.synth_inputs import synthetic_pair

    dev = torch.device("cuda", 0)
    rows = []
    for (B, S) in ((32, 512), (8, 2048)):
        lq, hq = synthetic_pair(1, S, S, seed=3)
        x = torch.from_numpy(lq[..., 0]).to(dev).repeat(B, 1, 1).contiguous()
        t = torch.from_numpy(hq[..., 0]).to(dev).repeat(B, 1, 1).contiguous()
        x += 0.01 * torch.rand_like(x)
        npx = B * S * S
        one = x[0].cpu().numpy().astype(np.float64)
        copies = {}

        def copy_us(bpp):
            """a device-to-device copy that moves bpp bytes per pixel of the batch in all (half read, half written)"""
            key = round(bpp, 3)
            if key not in copies:
                n = int(npx * bpp / 8)
                src, dst = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
                copies[key] = timed(lambda: dst.copy_(src), a.steps, a.warmup)[0]
                del src, dst
            return copies[key]

        for wv in ("db1", "db2"):
            levels = R.default_levels(S, S, len(R.rec_lo_of(wv)))
            g = sum(0.25 ** i for i in range(levels))
            cases = [(f"wavedec2 + waverec2 {wv}", lambda: filters.waverec2(filters.wavedec2(x, wv), wv, x.shape),
                      lambda: R.waverec2(R.wavedec2(one, wv), wv, one.shape), 16.0 * g),
                     (f"denoise_wavelet {wv} given sigma", lambda: filters.denoise_wavelet(x, wv, sigma=0.02),
                      lambda: R.denoise_wavelet(one, wv, sigma=0.02), 16.0 * g),
                     (f"denoise_wavelet {wv} estimated sigma", lambda: filters.denoise_wavelet(x, wv),
                      lambda: R.denoise_wavelet(one, wv), 16.0 * g + 4.0)]
            for name, ours, host, bpp in cases:
                us, us_min = timed(ours, a.steps, a.warmup)
                cus = copy_us(bpp)
                r = {"what": name, "shape": [B, S, S], "levels": levels, "us": round(us, 1), "us_min": round(us_min, 1),
                     "bytes_per_px": round(bpp, 2), "TB_per_s": round(bpp * npx / (us * 1e-6) / 1e12, 3), "same_bytes_copy_us": round(cus, 1),
                     "fraction_of_copy_rate": round(cus / us, 3)}
                if not a.no_host:
                    hus = host_us(host)
                    r["host_one_image_us"] = round(hus, 1)
                    r["host_per_image_over_ours"] = round(hus / (us / B), 1)
                rows.append(r)
                print(json.dumps(r), flush=True)
        us, us_min = timed(lambda: emdenoise.baseline_table(x, t, reference_columns=True), max(3, a.steps // 4), 1)
        r = {"what": "baseline_table (7 methods, mse + ssim each)", "shape": [B, S, S], "us": round(us, 1), "us_min": round(us_min, 1)}
        rows.append(r)
        print(json.dumps(r), flush=True)
        del x, t
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""),
                   "steps": a.steps, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
