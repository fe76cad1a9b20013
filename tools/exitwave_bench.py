#!/usr/bin/env python3
"""Times the focal-series reconstruction (csrc/exitwave.hip) on one GPU:

    python tools/exitwave_bench.py [--steps K] [--warmup W] [--out profiles/exitwave_bench.json]

Medians of K calls, each between its own pair of HIP events, after warm-up: ``fft2`` at [8,1024,1024] and [1,4096,4096],
``propagate`` at [8,1024,1024], and 10 iterations of ``reconstruct`` for N = 8 and 20 images at 512 x 512 and 1024 x 1024 -- the
fused path (two launches per iteration) and the composed path (``pad_periods = 0`` through the launches of ``propagate``).  Beside
each row, in the same process on the same GPU: the same operation composed from ``torch.fft`` in complex128 with the transfer
functions precomputed (the stand-in for the ArrayFire original), and a device-to-device copy of the row's bytes by design.

Bytes by design per element of S x S (complex double = 16 B, image = 4 B): fft2 64 (two passes, each reads and writes); propagate 96
(three passes); the fused reconstruction per image 20 for the first row launch, 32 per column launch, 36 per row launch between two
column launches, plus 48 for the exit wave; the composed reconstruction per image and iteration 2 x 96 for the two propagations, 16
for the mean and 36 for the modulus constraint."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.filter_bench import timed  # noqa: E402

LAM, PX, ITERS = 2.51e-12, 1e-10, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exitwave_bench.json"))
    a = ap.parse_args()
    import torch

    from emdenoise import exitwave

    dev = torch.device("cuda", 0)
    rows = []

    def copy_us(nbytes):
        n = int(nbytes // 8)
        src, dst = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
        us = timed(lambda: dst.copy_(src), a.steps, a.warmup)[0]
        del src, dst
        torch.cuda.empty_cache()
        return us

    def row(name, shape, ours, composed_torch, nbytes, **more):
        us, us_min = timed(ours, a.steps, a.warmup)
        tus = timed(composed_torch, a.steps, a.warmup)[0]
        cus = copy_us(nbytes)
        r = {"what": name, "shape": list(shape), "us": round(us, 1), "us_min": round(us_min, 1), "bytes": int(nbytes),
             "TB_per_s": round(nbytes / (us * 1e-6) / 1e12, 3), "same_bytes_copy_us": round(cus, 1), "fraction_of_copy_rate": round(cus / us, 3),
             "torch_fft_c128_us": round(tus, 1), "torch_over_ours": round(tus / us, 2)}
        r.update(more)
        rows.append(r)
        print(json.dumps(r), flush=True)
        return us

    def waves(B, S, seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        return torch.complex(torch.rand((B, S, S), device=dev, generator=g, dtype=torch.float64) - 0.5,
                             torch.rand((B, S, S), device=dev, generator=g, dtype=torch.float64) - 0.5)

    for B, S in ((8, 1024), (1, 4096)):
        z = waves(B, S, 1)
        row("fft2", (B, S, S), lambda: exitwave.fft2(z), lambda: torch.fft.fft2(z), 64.0 * B * S * S)
        del z
        torch.cuda.empty_cache()

    B, S = 8, 1024
    z = waves(B, S, 2)
    d = torch.linspace(-8e-8, 9e-8, B, dtype=torch.float64, device=dev)
    H = exitwave.transfer_function(S, LAM, d, px=PX)
    row("propagate", (B, S, S), lambda: exitwave.propagate(z, d, LAM, px=PX), lambda: torch.fft.ifft2(torch.fft.fft2(z) * H),
        96.0 * B * S * S)
    del z, H
    torch.cuda.empty_cache()

    for N, S in ((8, 512), (20, 512), (8, 1024), (20, 1024)):
        g = torch.Generator(device=dev).manual_seed(3)
        images = (1.0 + 0.1 * (torch.rand((N, S, S), device=dev, generator=g) - 0.5)).to(torch.float32)
        k = torch.arange(N, dtype=torch.float64, device=dev) - N // 2
        d = 2e-9 * torch.sign(k) * k * k + 1e-8
        Hp, Hm = exitwave.transfer_function(S, LAM, d, px=PX), exitwave.transfer_function(S, LAM, -d, px=PX)
        amp = images.double().abs()

        def torch_reconstruct():
            psi = images.to(torch.complex128)
            for _ in range(ITERS):
                E = torch.fft.ifft2(torch.fft.fft2(psi) * Hm).sum(0) / N
                b = torch.fft.ifft2(torch.fft.fft2(E)[None] * Hp)
                psi = amp * b / b.abs()
            return E

        px2 = float(S * S)
        fused = row(f"reconstruct, {ITERS} iterations, fused", (N, S, S),
                    lambda: exitwave.reconstruct(images, d, LAM, px=PX, iterations=ITERS), torch_reconstruct,
                    px2 * (N * (20.0 + 32.0 * ITERS + 36.0 * (ITERS - 1)) + 48.0), launches=1 + 1 + 2 * ITERS - 1 + 1)
        rows[-1]["us_per_iteration"] = round(fused / ITERS, 1)
        comp = row(f"reconstruct, {ITERS} iterations, composed", (N, S, S),
                   lambda: exitwave.reconstruct(images, d, LAM, px=PX, iterations=ITERS, _composed=True), torch_reconstruct,
                   px2 * N * ITERS * (192.0 + 16.0 + 36.0), launches=1 + 8 * ITERS - 1)
        rows[-1]["us_per_iteration"] = round(comp / ITERS, 1)
        rows[-1]["composed_over_fused"] = round(comp / fused, 2)
        del images, Hp, Hm, amp
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""),
                   "steps": a.steps, "iterations": ITERS, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
