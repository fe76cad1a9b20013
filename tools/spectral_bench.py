#!/usr/bin/env python3
"""Times the 2-D FFT of any side (csrc/fft_any.hip) on one GPU:

    python tools/spectral_bench.py [--steps K] [--warmup W] [--out profiles/spectral_bench.json]

Medians of K calls, each between its own pair of HIP events, after warm-up, in one process: ``spectral.fft2`` of one complex128 image
of 1000 x 1000, 1228 x 1228 and 2047 x 2047, beside ``torch.fft.fft2`` of the same tensor and beside this library's own plain
transform (``exitwave.fft2``) at the enclosing power of two (1024, 2048, 2048); and ``spectral.propagate`` at 1228 x 1228 beside the
same operation composed from ``torch.fft`` with the transfer function precomputed.  Recorded, not gated."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.filter_bench import timed  # noqa: E402

LAM, PX, DEFOCUS = 2.51e-12, 1e-10, 1.2e-7
FFT_ROWS = [(1000, 1024), (1228, 2048), (2047, 2048)]   # (side, the enclosing power of two)
PROP_SIDE = 1228


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectral_bench.json"))
    a = ap.parse_args()
    import torch

    from emdenoise import exitwave, spectral
    from tests import spectral_ref as R

    dev = torch.device("cuda", 0)
    rows = []

    def wave(n, seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        return torch.complex(torch.randn((1, n, n), device=dev, generator=g, dtype=torch.float64),
                             torch.randn((1, n, n), device=dev, generator=g, dtype=torch.float64))

    def us(fn):
        return round(timed(fn, a.steps, a.warmup)[0], 1)

    for n, p in FFT_ROWS:
        z, zp = wave(n, n), wave(p, p)
        r = {"what": "fft2", "shape": [1, n, n], "line": spectral.line_length(n), "us": us(lambda: spectral.fft2(z)),
             "torch_fft_c128_us": us(lambda: torch.fft.fft2(z)), "plain_side": p, "plain_us": us(lambda: exitwave.fft2(zp)),
             "torch_fft_c128_plain_us": us(lambda: torch.fft.fft2(zp)),
             "rel_l2_against_torch": float(torch.linalg.norm(spectral.fft2(z) - torch.fft.fft2(z)) / torch.linalg.norm(torch.fft.fft2(z)))}
        r["ours_over_torch"] = round(r["us"] / r["torch_fft_c128_us"], 2)
        r["ours_over_plain"] = round(r["us"] / r["plain_us"], 2)
        rows.append(r)
        print(json.dumps(r), flush=True)
        del z, zp
        torch.cuda.empty_cache()

    n = PROP_SIDE
    z = wave(n, 7)
    d = torch.full((1,), DEFOCUS, dtype=torch.float64, device=dev)
    Hf = torch.from_numpy(R.transfer_function(n, n, LAM, DEFOCUS, PX)).to(dev)
    r = {"what": "propagate", "shape": [1, n, n], "line": spectral.line_length(n), "us": us(lambda: spectral.propagate(z, d, LAM, px=PX)),
         "torch_fft_c128_us": us(lambda: torch.fft.ifft2(torch.fft.fft2(z) * Hf)),
         "rel_l2_against_torch": float(torch.linalg.norm(spectral.propagate(z, d, LAM, px=PX) - torch.fft.ifft2(torch.fft.fft2(z) * Hf))
                                       / torch.linalg.norm(z))}
    r["ours_over_torch"] = round(r["us"] / r["torch_fft_c128_us"], 2)
    rows.append(r)
    print(json.dumps(r), flush=True)

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""),
                   "steps": a.steps, "warmup": a.warmup, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
