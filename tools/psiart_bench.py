#!/usr/bin/env python3
"""Times one step of the gradient-descent exit-wave and aberration fit (csrc/psiart.hip) on one GPU:

    python tools/psiart_bench.py [--steps K] [--warmup W] [--out profiles/psiart_bench.json]

Medians of K calls of ``PsiArtFit.step()``, each between its own pair of HIP events, after warm-up, for N = 8 and 16 images at
512 x 512 and 1024 x 1024, every one of the 29 rates non-zero.  Beside each row, in the same process on the same GPU: the same step
composed from ``torch.fft`` in complex128 with autograd and ``torch.optim.Adam`` (the stand-in for the TensorFlow original), a
device-to-device copy of the row's bytes by design, and the number of launches per step.  Beside those, the step with trainable
per-image shifts (every shift rate non-zero, shifts of +-0.3 px) and the same composition with the shifts as a
trainable phase ramp: ``shift_us``, ``shift_over_plain`` and ``torch_shift_us``.

Bytes by design per pixel (complex double = 16 B, double = 8 B, image = 4 B): rows of psi 32; forward columns 48 + 16 N (psi^ and
(chi_base / pi, T) are written for the reverse pass); inverse rows with the row sums 36 N; the loss pass 20 N; rows of G_b 36 N;
reverse columns 48 + 16 N; inverse rows with the field gradients and Adam 112.  240 + 124 N in all."""
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

SAMPLING, SCALE, LAUNCHES = 0.5, 5.0, 10
TERMS = ((2, 2, 0, 1), (2, 0, 2, None), (3, 3, 3, 4), (3, 1, 5, 6), (4, 4, 7, 8), (4, 2, 9, 10), (4, 0, 11, None), (5, 5, 12, 13),
         (5, 3, 14, 15), (5, 1, 16, 17), (6, 6, 18, 19), (6, 4, 20, 21), (6, 2, 22, 23), (6, 0, 24, None))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "psiart_bench.json"))
    a = ap.parse_args()
    import torch

    from emdenoise import psiart

    dev = torch.device("cuda", 0)
    lam = float(psiart.energy2wavelength(200))
    rows = []
    for N, S in ((8, 512), (16, 512), (8, 1024), (16, 1024)):
        g = torch.Generator(device=dev).manual_seed(5)
        images = (1.0 + 0.1 * (torch.rand((N, S, S), device=dev, generator=g) - 0.5)).to(torch.float32)
        th_np, phi_np = psiart.polar_grid(S, SAMPLING, lam)
        p0 = np.zeros(psiart.NPARAM)
        for n, m, ia, ip in TERMS:                    # every coefficient non-zero: 1 rad at the largest theta
            p0[ia] = n * lam / (2.0 * np.pi * th_np.max() ** n) / (3.0 * (N // 2) if ia == 2 else 1.0)
            if ip is not None:
                p0[ip] = 0.3
        p0[25], p0[26] = 15.0, 0.2
        ramp = psiart.defocus_ramp(N)
        fit = psiart.PsiArtFit(images, lam, SAMPLING, rates=np.full(29, 1e-6), offset_scale=SCALE)
        fit._params.copy_(torch.from_numpy(p0))
        us, us_min = timed(lambda: fit.step(), a.steps, a.warmup)
        d0 = 0.3 * np.cos(np.arange(2 * N, dtype=np.float64)).reshape(N, 2)
        sfit = psiart.PsiArtFit(images, lam, SAMPLING, rates=np.full(29, 1e-6), offset_scale=SCALE, shifts=d0)
        sfit._params.copy_(torch.from_numpy(p0))
        sfit.set_shift_rates(np.full(N, 1e-6))
        sus, sus_min = timed(lambda: sfit.step(), a.steps, a.warmup)
        us2 = timed(lambda: fit.step(), a.steps, a.warmup)[0]      # the step without shifts again, after the one with them

        th, phi = torch.from_numpy(th_np.copy()).to(dev), torch.from_numpy(phi_np.copy()).to(dev)
        root = images.double().clamp_min(0).sqrt()
        rmean = root.mean((1, 2))
        A = root[N // 2].clone().requires_grad_(True)
        P = torch.zeros((S, S), dtype=torch.float64, device=dev, requires_grad=True)
        par = torch.from_numpy(p0).to(dev).requires_grad_(True)
        rk = torch.from_numpy(ramp).to(dev)
        opt = torch.optim.Adam([A, P, par], lr=1e-6, betas=(0.99, 0.999), eps=0.1)

        f = torch.from_numpy(np.fft.fftfreq(S)).to(dev)
        dsh = torch.from_numpy(d0).to(dev).requires_grad_(True)
        opt_s = torch.optim.Adam([A, P, par, dsh], lr=1e-6, betas=(0.99, 0.999), eps=0.1)

        def torch_step(shifted=False):
            (opt_s if shifted else opt).zero_grad(set_to_none=True)
            ph = torch.fft.fft2(torch.polar(A, P))
            off = SCALE * torch.tanh(par[26] / SCALE)
            base = 0
            for n, m, ia, ip in TERMS:
                if ia != 2:
                    base = base + par[ia] * (torch.cos(m * (phi - par[ip])) if ip is not None else 1.0) * th ** n / n
            chi = (2 * np.pi / lam) * (base[None] + (par[2] * rk + off)[:, None, None] * (th ** 2 / 2)[None])
            if shifted:
                chi = chi + 2 * np.pi * (f[None, :, None] * dsh[:, 0, None, None] + f[None, None, :] * dsh[:, 1, None, None])
            T = torch.exp(-torch.sign(par[25]) * (0.5 * np.pi / lam * par[25] * th ** 2) ** 2)
            m_ = torch.fft.ifft2(torch.polar(T[None].expand_as(chi), -chi) * ph[None]).abs()
            c = rmean / m_.mean((1, 2))
            loss = ((c[:, None, None] * m_ - root) ** 2).mean((1, 2)).sum() / N
            loss.backward()
            (opt_s if shifted else opt).step()

        tus = timed(torch_step, a.steps, a.warmup)[0]
        tsus = timed(lambda: torch_step(True), a.steps, a.warmup)[0]
        nbytes = float(S * S) * (240.0 + 124.0 * N)
        n8 = int(nbytes // 8)
        src, dst = torch.empty(n8, dtype=torch.float32, device=dev), torch.empty(n8, dtype=torch.float32, device=dev)
        cus = timed(lambda: dst.copy_(src), a.steps, a.warmup)[0]
        r = {"what": "step", "shape": [N, S, S], "us": round(us, 1), "us_min": round(us_min, 1), "launches": LAUNCHES, "bytes": int(nbytes),
             "TB_per_s": round(nbytes / (us * 1e-6) / 1e12, 3), "same_bytes_copy_us": round(cus, 1), "fraction_of_copy_rate": round(cus / us, 3),
             "torch_fft_c128_autograd_adam_us": round(tus, 1), "torch_over_ours": round(tus / us, 2), "us_again": round(us2, 1),
             "shift_us": round(sus, 1), "shift_us_min": round(sus_min, 1), "shift_over_plain": round(sus / us, 3),
             "torch_shift_us": round(tsus, 1), "torch_shift_over_ours": round(tsus / sus, 2)}
        rows.append(r)
        print(json.dumps(r), flush=True)
        del fit, sfit, images, src, dst, A, P, par, dsh, opt, opt_s, root
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""),
                   "steps": a.steps, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
