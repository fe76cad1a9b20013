#!/usr/bin/env python3
"""Times the candidate-batched reconstruction and the defocus search (csrc/exitwave.hip) on one GPU:

    python tools/exitwave_search_bench.py [--steps K] [--warmup W] [--out profiles/exitwave_search_bench.json]

Medians of K calls, each between its own pair of HIP events, after warm-up, all in one process.  A defocus sweep of C = 10 increments
over N = 8 images, 10 iterations, at 128, 256, 512 and 1024 pixels a side: the one candidate-batched call (``_sequential=False``)
against the loop of C reconstructions (``_sequential=True``, what ``defocus_sweep`` was before the batched call existed) and against
the same sweep composed from ``torch.fft`` in complex128 with the transfer functions precomputed.  Then ``defocus_search`` at 256 and
512: "section" with 8 candidates and 4 rounds, "plateau" with 8 steps from a given seed."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.filter_bench import timed  # noqa: E402

LAM, PX, ITERS, N, C = 2.51e-12, 1e-10, 10, 8, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exitwave_search_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch

    from emdenoise import exitwave

    dev = torch.device("cuda", 0)
    rows = []
    k = np.arange(N, dtype=np.float64) - N // 2
    ramp = 0.2 * np.sign(k) * k * k + 1.0
    incs = np.linspace(0.5e-8, 1.5e-8, C)
    kw = dict(px=PX, iterations=ITERS)

    def note(r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    for S in (128, 256, 512, 1024):
        g = torch.Generator(device=dev).manual_seed(3)
        images = (1.0 + 0.1 * (torch.rand((N, S, S), device=dev, generator=g) - 0.5)).to(torch.float32)
        table = torch.from_numpy(np.outer(incs, ramp)).to(dev)
        Hp = torch.stack([exitwave.transfer_function(S, LAM, table[c], px=PX) for c in range(C)])
        Hm = torch.stack([exitwave.transfer_function(S, LAM, -table[c], px=PX) for c in range(C)])
        amp = images.double().abs()

        def torch_sweep():
            out = []
            for c in range(C):
                psi = images.to(torch.complex128)
                for _ in range(ITERS):
                    E = torch.fft.ifft2(torch.fft.fft2(psi) * Hm[c]).sum(0) / N
                    b = torch.fft.ifft2(torch.fft.fft2(E)[None] * Hp[c])
                    psi = amp * b / b.abs()
                inten = b.real * b.real + b.imag * b.imag
                cc = images.double().mean((1, 2)) / inten.mean((1, 2))
                out.append(((images.double() - cc[:, None, None] * inten) ** 2).mean((1, 2)).max())
            return torch.stack(out)

        batched = timed(lambda: exitwave.defocus_sweep(images, LAM, incs, ramp, _sequential=False, **kw), a.steps, a.warmup)
        seq = timed(lambda: exitwave.defocus_sweep(images, LAM, incs, ramp, _sequential=True, **kw), a.steps, a.warmup)
        tus = timed(torch_sweep, a.steps, a.warmup)[0]
        note({"what": f"defocus sweep, {C} increments, {ITERS} iterations", "shape": [N, S, S], "batched_us": round(batched[0], 1),
              "batched_us_min": round(batched[1], 1), "sequential_us": round(seq[0], 1), "sequential_us_min": round(seq[1], 1),
              "sequential_over_batched": round(seq[0] / batched[0], 2), "torch_fft_c128_us": round(tus, 1),
              "torch_over_batched": round(tus / batched[0], 2), "launches_batched": 2 * ITERS + 6, "launches_sequential": C * (2 * ITERS + 6)})
        if S in (256, 512):
            r, b2 = torch.from_numpy(ramp).to(dev), torch.tensor([0.3e-8, 1.9e-8], dtype=torch.float64, device=dev)
            b3 = torch.tensor([0.6e-8, 1.2e-8, 1e30], dtype=torch.float64, device=dev)
            sec = timed(lambda: exitwave.defocus_search(images, LAM, r, bracket=b2, candidates=8, rounds=4, **kw), a.steps, a.warmup)
            pla = timed(lambda: exitwave.defocus_search(images, LAM, r, method="plateau", bracket=b3, max_steps=8, **kw), a.steps, a.warmup)
            note({"what": "defocus_search section, 8 candidates, 4 rounds", "shape": [N, S, S], "us": round(sec[0], 1),
                  "us_min": round(sec[1], 1), "reconstructions": 32, "us_per_reconstruction": round(sec[0] / 32, 1)})
            note({"what": "defocus_search plateau, 8 steps", "shape": [N, S, S], "us": round(pla[0], 1), "us_min": round(pla[1], 1),
                  "reconstructions": 8, "us_per_reconstruction": round(pla[0] / 8, 1)})
        del images, Hp, Hm, amp
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""),
                   "steps": a.steps, "iterations": ITERS, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
