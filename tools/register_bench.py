#!/usr/bin/env python3
"""Times the registration of a focal series (csrc/register.hip) on one GPU:

    python tools/register_bench.py [--steps K] [--warmup W] [--out profiles/register_bench.json]

Medians of K calls, each between its own pair of HIP events, after warm-up: ``phase_correlate`` in chain mode (``rel_pos_estimate``
without the centres) at [8,1024,1024] and [2,4096,4096], ``crop_stack`` at [8,2048,2048] -> 1024 x 1024, and ``reconstruct_series``
for N = 8 at 1024 x 1024 -> 512 x 512 with 10 iterations.  Beside each row, in the same process on the same GPU: the same
computation composed from ``torch.fft`` in float64 / complex128 and torch indexing (everything on the device, no read-back), and a
device-to-device copy of the row's bytes by design.

Bytes by design per pixel of S x S (complex double = 16 B, double = 8 B, image = 4 B): the rows of every image 4 + 16, the columns 16
per image read and 16 per pair written, the surface 16 + 8 per pair; the crop 4 read and 4 written per output pixel;
``reconstruct_series`` the sum of the three and the fused reconstruction's of tools/exitwave_bench.py."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.filter_bench import timed  # noqa: E402

LAM, PX, ITERS = 2.51e-12, 1e-10, 10


def correlate_bytes(N, S):
    return float(S * S) * (N * (4.0 + 16.0 + 16.0) + (N - 1) * (16.0 + 16.0 + 8.0))


def crop_bytes(N, side):
    return float(N * side * side) * 8.0


def recon_bytes(N, s):
    return float(s * s) * (N * (20.0 + 32.0 * ITERS + 36.0 * (ITERS - 1)) + 48.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "register_bench.json"))
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
             "torch_composition_us": round(tus, 1), "torch_over_ours": round(tus / us, 2)}
        r.update(more)
        rows.append(r)
        print(json.dumps(r), flush=True)

    def stack(N, S, seed):
        """A random field rolled by a few pixels per image: the correlation has a sharp peak."""
        g = torch.Generator(device=dev).manual_seed(seed)
        x = torch.rand((S, S), device=dev, generator=g)
        return torch.stack([torch.roll(x, (3 * k - 5, 7 - 2 * k), (0, 1)) for k in range(N)]).contiguous()

    def torch_shifts(x):
        """[N-1,2]: the restated phase correlation of consecutive images, on the device."""
        S = x.shape[-1]
        F = torch.fft.fft2(x.double())
        P = F[:-1] * F[1:].conj()
        m = P.abs()
        R = torch.where(m > 0, P / m, torch.zeros_like(P))
        c = torch.fft.fftshift(torch.fft.ifft2(R).real, dim=(-2, -1))
        idx = c.flatten(1).argmax(1)
        py, px = idx // S, idx % S
        off = torch.arange(-2, 3, device=dev)
        ys, xs = py[:, None] + off[None], px[:, None] + off[None]
        ok = ((ys >= 0) & (ys < S))[:, :, None] & ((xs >= 0) & (xs < S))[:, None, :]
        v = c[torch.arange(c.shape[0], device=dev)[:, None, None], ys.clamp(0, S - 1)[:, :, None], xs.clamp(0, S - 1)[:, None, :]] * ok
        sv = v.sum((1, 2))
        cx, cy = (v * xs[:, None, :]).sum((1, 2)) / sv, (v * ys[:, :, None]).sum((1, 2)) / sv
        return torch.stack([S / 2 - cx, S / 2 - cy], 1)

    def torch_centres(shifts, S):
        pos = torch.cat([torch.zeros((1, 2), dtype=torch.float64, device=dev), shifts.cumsum(0)])
        return S / 2 + pos - pos.mean(0)

    def torch_crop(x, centres, side):
        N, S = x.shape[0], x.shape[-1]
        x0 = centres - side / 2
        i0 = torch.floor(x0)
        f = (x0 - i0)[:, :, None]                                           # [N,2,1]
        t = i0.long()[:, :, None] + torch.arange(side, device=dev)[None, None]   # [N,2,side]: x taps, y taps
        n = torch.arange(N, device=dev)[:, None, None]

        def tap(dy, dx):
            ys, xs = t[:, 1, :, None] + dy, t[:, 0, None, :] + dx
            ok = (ys >= 0) & (ys < S) & (xs >= 0) & (xs < S)
            return x[n, ys.clamp(0, S - 1), xs.clamp(0, S - 1)].double() * ok

        fx, fy = f[:, 0, None, :], f[:, 1, :, None]
        return ((1 - fy) * ((1 - fx) * tap(0, 0) + fx * tap(0, 1)) + fy * ((1 - fx) * tap(1, 0) + fx * tap(1, 1))).float()

    for N, S in ((8, 1024), (2, 4096)):
        x = stack(N, S, 1)
        ours = exitwave.rel_pos_estimate(x, as_cropping_centres=False)
        theirs = torch_shifts(x)
        row("phase_correlate, chain mode", (N, S, S), lambda: exitwave.rel_pos_estimate(x, as_cropping_centres=False), lambda: torch_shifts(x),
            correlate_bytes(N, S), launches=5, largest_distance_from_torch=float((ours - theirs).abs().max()))
        del x
        torch.cuda.empty_cache()

    N, S, side = 8, 2048, 1024
    x = stack(N, S, 2)
    centres = S / 2 + 40.0 * (torch.rand((N, 2), device=dev, dtype=torch.float64) - 0.5)
    same = bool(torch.equal(exitwave.crop_stack(x, centres, side), torch_crop(x, centres, side)))
    row("crop_stack", (N, S, S, side), lambda: exitwave.crop_stack(x, centres, side), lambda: torch_crop(x, centres, side),
        crop_bytes(N, side), launches=1, same_bits_as_torch=same)
    del x
    torch.cuda.empty_cache()

    N, S, side = 8, 1024, 512
    x = 1.0 + 0.1 * (stack(N, S, 3) - 0.5)
    k = torch.arange(N, dtype=torch.float64, device=dev) - N // 2
    d = 2e-9 * torch.sign(k) * k * k + 1e-8
    Hp, Hm = exitwave.transfer_function(side, LAM, d, px=PX), exitwave.transfer_function(side, LAM, -d, px=PX)

    def torch_series():
        images = torch_crop(x, torch_centres(torch_shifts(x), S), side)
        amp = images.double().abs()
        psi = images.to(torch.complex128)
        for _ in range(ITERS):
            E = torch.fft.ifft2(torch.fft.fft2(psi) * Hm).sum(0) / N
            b = torch.fft.ifft2(torch.fft.fft2(E)[None] * Hp)
            psi = amp * b / b.abs()
        return E

    ours, theirs = exitwave.reconstruct_series(x, d, LAM, side, px=PX, iterations=ITERS), torch_series()
    row(f"reconstruct_series, {ITERS} iterations", (N, S, S, side),
        lambda: exitwave.reconstruct_series(x, d, LAM, side, px=PX, iterations=ITERS), torch_series,
        correlate_bytes(N, S) + crop_bytes(N, side) + recon_bytes(N, side), launches=5 + 1 + 1 + 2 * ITERS + 2,
        rel_l2_from_torch=float(torch.linalg.norm(ours - theirs) / torch.linalg.norm(theirs)))

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""),
                   "steps": a.steps, "iterations": ITERS, "rows": rows,
                   "not_measured": "no rocprofv3 trace, no per-kernel split, no hardware counters; pair mode and the window are not timed"},
                  fh, indent=1)


if __name__ == "__main__":
    main()
