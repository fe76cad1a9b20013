#!/usr/bin/env python3
"""Times the affine registration by mutual information and the warp (csrc/affine.hip) on one GPU:

    python tools/affine_bench.py [--steps K] [--warmup W] [--out profiles/affine_bench.json]
    python tools/affine_bench.py --iterations-only 200        # nothing but optimizer iterations at the bench shape, for a kernel trace

Medians of K calls, each between its own pair of HIP events, after warm-up: ``warp`` at [8,2048,2048]; the metric
(``mutual_information``) and one optimizer iteration (the difference of 150 and 50 iterations in one call, over 100) at P = 7 pairs of
2048 x 2048 with 250 000 samples and 50 bins; ``register_series`` of 8 images for 1000 iterations on three levels.  Beside each row, in
the same process on the same GPU: a device-to-device copy of the row's bytes by design, and for the warp and the metric the same
computation composed from torch in float64 (a gather, and for the histogram ``index_add_``).

Bytes by design: the warp reads and writes 4 bytes per pixel; the metric reads per pair and sample the index (4), the fixed pixel (4)
and four moving taps (16), writes and reads G = 64 partial histograms of bins^2 x 8 bytes per pair, and reads both images once for
the extrema (8 per pixel and pair); an iteration is the metric without the extrema; ``register_series`` is 1000 iterations at their
levels' sizes plus the extrema once per level."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.filter_bench import timed  # noqa: E402

P, S, NSAMPLES, BINS, NSERIES, ITERS = 7, 2048, 250000, 50, 8, 1000


def metric_bytes(pairs, n, extrema_pixels):
    G = min(64, -(-n // 1024))
    return float(pairs) * (n * 24.0 + 2.0 * G * BINS * BINS * 8.0 + extrema_pixels * 8.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "affine_bench.json"))
    ap.add_argument("--iterations-only", type=int, default=0)
    a = ap.parse_args()
    import numpy as np
    import torch

    from emdenoise import affine

    dev = torch.device("cuda", 0)
    rows = []

    def series(N, side, seed):
        """A smooth random field with noise, image k rotated, scaled and shifted a little more than image k - 1, then inverted for odd k."""
        g = torch.Generator(device=dev).manual_seed(seed)
        coarse = torch.rand((1, 1, side // 32 + 1, side // 32 + 1), device=dev, generator=g)
        field = torch.nn.functional.interpolate(coarse, size=(side, side), mode="bicubic", align_corners=True)[0, 0].clamp(0, 1)
        field = (field + 0.05 * torch.rand((side, side), device=dev, generator=g)).float().contiguous()
        T = torch.from_numpy(np.stack([affine.from_similarity(0.3 * k, 1.0 + 0.002 * k, (1.5 * k, -1.0 * k), side, side) for k in range(N)])).to(dev)
        x = affine.warp(field[None].expand(N, side, side).contiguous(), T, fill=0.5)
        x[1::2] = (1.0 - x[1::2] / 1.06) ** 1.5
        return x.contiguous()

    if a.iterations_only:
        x = series(P + 1, S, 1)
        smp = affine.draw_samples(NSAMPLES, S, S, 0)
        state = affine.iterate(x[:-1], x[1:], None, a.iterations_only, smp, BINS, reset=True)
        torch.cuda.synchronize()
        print(json.dumps({"iterations": a.iterations_only, "accepted": affine.state_fields(state)["accepted"].tolist()}))
        return

    def copy_us(nbytes):
        n = max(int(nbytes // 8), 1)
        src, dst = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
        us = timed(lambda: dst.copy_(src), a.steps, a.warmup)[0]
        del src, dst
        torch.cuda.empty_cache()
        return us

    def row(name, shape, us, us_min, nbytes, torch_us=None, **more):
        cus = copy_us(nbytes)
        r = {"what": name, "shape": list(shape), "us": round(us, 1), "us_min": round(us_min, 1), "bytes": int(nbytes),
             "TB_per_s": round(nbytes / (us * 1e-6) / 1e12, 4), "same_bytes_copy_us": round(cus, 1), "fraction_of_copy_rate": round(cus / us, 3)}
        if torch_us is not None:
            r.update(torch_composition_us=round(torch_us, 1), torch_over_ours=round(torch_us / us, 2))
        r.update(more)
        rows.append(r)
        print(json.dumps(r), flush=True)

    def pull(T, H, W, x, y):
        cx, cy, h = affine.geometry(H, W)
        u, v = (x.double() - cx) / h, (y.double() - cy) / h
        return ((T[..., 0, 0, None] * u + T[..., 0, 1, None] * v) + T[..., 0, 2, None]) * h + cx, \
               ((T[..., 1, 0, None] * u + T[..., 1, 1, None] * v) + T[..., 1, 2, None]) * h + cy

    def taps(img, xs, ys, fill):
        """Bilinear values [N,n] of img [N,H,W] at float64 coordinates [N,n]."""
        N, H, W = img.shape
        flat = img.reshape(N, H * W)
        ix, iy = torch.floor(xs), torch.floor(ys)
        fx, fy = xs - ix, ys - iy
        ix, iy = ix.long(), iy.long()

        def tap(j, k):
            yy, xx = iy + j, ix + k
            ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            return torch.where(ok, flat.gather(1, yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).double(), fill)

        return (1 - fy) * ((1 - fx) * tap(0, 0) + fx * tap(0, 1)) + fy * ((1 - fx) * tap(1, 0) + fx * tap(1, 1))

    def torch_warp(img, T, fill):
        N, H, W = img.shape
        idx = torch.arange(H * W, device=dev)
        xs, ys = pull(T, H, W, (idx % W)[None], (idx // W)[None])
        return taps(img, xs, ys, torch.tensor(fill, dtype=torch.float64, device=dev)).float().reshape(N, H, W)

    def torch_mi(fixed, moving, T, smp):
        """The same metric from a gather and index_add_ in float64 (weights as doubles, not fixed point)."""
        Pn, H, W = fixed.shape
        s = smp.long()
        xs, ys = pull(T, H, W, (s % W)[None], (s // W)[None])
        ok = (xs >= 0) & (xs <= W - 1) & (ys >= 0) & (ys <= H - 1)
        zero = torch.zeros((), dtype=torch.float64, device=dev)
        m = taps(moving, torch.where(ok, xs, zero), torch.where(ok, ys, zero), zero)
        f = fixed.reshape(Pn, H * W)[:, s].double()
        fmin, fmax = fixed.amin((1, 2)).double()[:, None], fixed.amax((1, 2)).double()[:, None]
        mmin, mmax = moving.amin((1, 2)).double()[:, None], moving.amax((1, 2)).double()[:, None]
        tf = (f - fmin) / ((fmax - fmin) / (BINS - 4)) + 2
        tm = (m - mmin) / ((mmax - mmin) / (BINS - 4)) + 2
        jf, jm = torch.floor(tf).clamp(2, BINS - 3).long(), torch.floor(tm).clamp(2, BINS - 3).long()
        hist = torch.zeros((Pn, BINS * BINS), dtype=torch.float64, device=dev)
        base = (torch.arange(Pn, device=dev) * BINS * BINS)[:, None]
        for d in (-1, 0, 1, 2):
            aa = ((jm + d).double() - tm).abs()
            w = torch.where(aa < 1, (4 - 6 * aa * aa + 3 * aa * aa * aa) / 6, torch.where(aa < 2, (2 - aa) ** 3 / 6, zero)) * ok
            hist.view(-1).index_add_(0, (base + jf * BINS + jm + d).reshape(-1), w.reshape(-1))
        Pj = (hist / hist.sum(1, keepdim=True)).reshape(Pn, BINS, BINS)
        pf, pm = Pj.sum(2, keepdim=True), Pj.sum(1, keepdim=True)
        return torch.where(Pj > 0, Pj * torch.log(Pj / (pf * pm)), zero).sum((1, 2))

    # the warp
    x = series(8, S, 2)
    T = torch.from_numpy(np.stack([affine.from_similarity(0.5 * k - 2.0, 1.0 + 0.004 * k, (3.0 * k, -2.0 * k), S, S) for k in range(8)])).to(dev)
    same = bool(torch.equal(affine.warp(x, T, 0.25), torch_warp(x, T, 0.25)))
    us, us_min = timed(lambda: affine.warp(x, T, 0.25), a.steps, a.warmup)
    row("warp", (8, S, S), us, us_min, 8.0 * 8 * S * S, timed(lambda: torch_warp(x, T, 0.25), a.steps, a.warmup)[0], launches=1,
        same_bits_as_torch=same)
    del x
    torch.cuda.empty_cache()

    # the metric and one iteration
    x = series(P + 1, S, 1)
    fixed, moving = x[:-1], x[1:]
    smp = affine.draw_samples(NSAMPLES, S, S, 0)
    Tc = torch.from_numpy(np.stack([affine.from_similarity(0.3, 1.002, (1.5, -1.0), S, S)] * P)).to(dev)
    ours, theirs = affine.mutual_information(fixed, moving, Tc, smp, BINS), torch_mi(fixed, moving, Tc, smp)
    us, us_min = timed(lambda: affine.mutual_information(fixed, moving, Tc, smp, BINS), a.steps, a.warmup)
    row("mutual_information", (P, S, S, NSAMPLES, BINS), us, us_min, metric_bytes(P, NSAMPLES, S * S),
        timed(lambda: torch_mi(fixed, moving, Tc, smp), a.steps, a.warmup)[0], launches=4,
        largest_distance_from_torch=float((ours - theirs).abs().max()))
    ws = torch.empty(affine._lib.load().emd_mattes_mi_workspace_bytes(P, S, S, NSAMPLES, BINS) // 8 + 1, dtype=torch.float64, device=dev)
    state = affine.iterate(fixed, moving, None, 0, smp, BINS, reset=True)
    start = state.clone()

    def block(k):
        state.copy_(start)
        affine.iterate(fixed, moving, state, k, smp, BINS, workspace=ws)

    t150, t50 = timed(lambda: block(150), a.steps, a.warmup), timed(lambda: block(50), a.steps, a.warmup)
    per = (t150[0] - t50[0]) / 100.0
    row("one optimizer iteration (histogram launch + step launch)", (P, S, S, NSAMPLES, BINS), per, (t150[1] - t50[1]) / 100.0,
        metric_bytes(P, NSAMPLES, 0), launches=2, block_of_150_us=round(t150[0], 1), block_of_50_us=round(t50[0], 1))
    del x, fixed, moving
    torch.cuda.empty_cache()

    # the series
    x = series(NSERIES, S, 3)
    kw = dict(iterations=ITERS, samples=NSAMPLES, bins=BINS, levels=3, seed=0)
    pairs, st = affine.register_series(x, return_state=True, **kw)
    f = affine.state_fields(st)
    us, us_min = timed(lambda: affine.register_series(x, **kw), a.steps, a.warmup)
    per_level = [ITERS // 3, ITERS // 3, ITERS - 2 * (ITERS // 3)]
    nbytes = sum(metric_bytes(NSERIES - 1, NSAMPLES, 0) * k + (NSERIES - 1) * 8.0 * (S >> (2 - lv)) ** 2 for lv, k in enumerate(per_level))
    row(f"register_series, {ITERS} iterations on 3 levels", (NSERIES, S, S, NSAMPLES, BINS), us, us_min, nbytes,
        launches=2 * ITERS + 3 * 3 + 4 + 2, accepted=f["accepted"].tolist(), status=f["status"].tolist(),
        largest_parameter=float((pairs - torch.tensor([[1.0, 0, 0], [0, 1.0, 0]], dtype=torch.float64, device=dev)).abs().max()))

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""),
                   "steps": a.steps, "rows": rows,
                   "not_measured": "no hardware counters; the per-kernel split of an iteration comes from a separate kernel trace of "
                                   "--iterations-only (DESIGN.md 3.22)"}, fh, indent=1)


if __name__ == "__main__":
    main()
