"""Graph K training speed: microseconds per training step (bench.py measures the flagship inference workload and stays as it is).

    python tools/k_train_bench.py [--steps K] [--warmup W] [--out profiles/k_train_bench.json]

Rows (filter (depth, width) = (2, 3) unless stated; one step = every filter's forward + backward + reduce + Adam launches):
  sampler+step  [32,10,10]     emd_k_sample_crops_f32 + emd_k_train_step_f32, eager (the reference's configuration, :52/:81).
                               Compare with the kernels' device time from a trace (rocprofv3 --kernel-trace --stats -- python
                               tools/k_train_bench.py): measured 16.5 + 6.6 + 4.3 us, i.e. these rows are device-bound, not host-bound
  step          [32,10,10]     emd_k_train_step_f32 alone on a fixed batch
  fused n       [32,10,10]     emd_k_train_fused_f32: n whole steps per launch (n = 1000, and n = 10, the validation cadence)
  step          [32,171,171]   the reference's other crop size (:81, commented)
  step          [32,512,512]   a full frame; printed beside the VALU bound computed for this kernel's instruction mix
  sweep 5x5     [32,10,10]     depths 1..5 x widths 3,5,7,9,13 (the commented sweep of :360-361 without the width 17 this
                               library refuses), 25 filters on one sampled batch per step: eager, and fused (n = 1000)
Timing: torch.cuda events around K back-to-back steps after W warm-up steps, median of 5 repeats."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# MI355X: 256 CUs x 4 SIMD-32 at 2.4 GHz; a wave's VALU instruction occupies its SIMD 4 cycles (64 lanes), a transcendental
# (v_exp_f32, v_rcp_f32) 8 (MI355X_MICROARCH constants table)
CUS, SIMDS, CLOCK = 256, 4, 2.4e9


def valu_bound_us(npix, width, depth):
    """Lower bound of k_grad_kernel from its per-tap instruction count: forward (w0*v, then per layer l >= 1 add b, exp,
    add 1, rcp, mul s, mul w; accumulate) once in the forward pass and again in the backward pass, plus the backward
    (per layer: 3 mul/fma for dw, ds and dz, the 1-g, the dz product, the db add; the dw0 fma)."""
    taps = width * width
    plain_fwd = 2 + 4 * (depth - 1)            # w0*v, accumulate; per layer: add b, add 1, mul s, mul w
    trans_fwd = 2 * (depth - 1)                # exp, rcp
    plain_bwd = 1 + 6 * (depth - 1)
    plain = taps * (2 * plain_fwd + plain_bwd)
    trans = taps * 2 * trans_fwd
    cycles_per_wave = 4 * plain + 8 * trans    # per 64 pixels on one SIMD
    waves = npix / 64
    return waves * cycles_per_wave / (CUS * SIMDS * CLOCK) * 1e6, plain, trans


def problem_bound_us(npix, width, depth):
    """Lower bound of the PROBLEM (not of this kernel's form), (2,3)-style D4-symmetric maps: the class trick evaluates each
    input pixel's chain once per tap class (nsym classes: `depth-1` sigmoids of 2 transcendentals + 4 plain ops each) and
    keeps g and g(1-g) for the backward; the forward sums w^2 class terms per output pixel (1 add each); the backward does,
    per tap, one FMA per gradient kind (dw per layer, db and ds per layer >= 1) on the output residual, plus per class the
    chain-rule products (3 per layer >= 1).  Same chip rate as valu_bound_us."""
    nsym = (width // 2 + 1) * (width // 2 + 2) // 2
    taps = width * width
    trans = nsym * 2 * (depth - 1)
    plain = nsym * (1 + 4 * (depth - 1)) + taps + taps * (depth + 2 * (depth - 1)) + nsym * 3 * (depth - 1)
    cycles_per_wave = 4 * plain + 8 * trans
    return (npix / 64) * cycles_per_wave / (CUS * SIMDS * CLOCK) * 1e6, plain, trans


def timed(fn, steps, warmup, reps=5):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / steps)
    return float(np.median(out)), [round(v, 2) for v in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import emdenoise
    from emdenoise import k_trainer as KT
    from tests.synth_inputs import synthetic_lq

    dev = torch.device("cuda", 0)
    rows = []

    def row(name, shape, configs, us, reps, **kw):
        r = {"row": name, "shape": list(shape), "configs": [list(c) for c in configs], "us_per_step": round(us, 2), "reps_us": reps}
        r.update(kw)
        rows.append(r)
        print(json.dumps(r), flush=True)

    stack = torch.from_numpy(synthetic_lq(16, 96, 96, seed=1)[..., 0]).to(dev)
    crops = torch.empty((32, 10, 10), dtype=torch.float32, device=dev)
    big = 10 ** 9   # timing only: keep lr0 (1 - t / (T + 1)) positive however many steps run
    tr = emdenoise.KernelDenoiserTrainer([(2, 3)], device=dev, seed=0, total_steps=big)
    f = tr.filters[0]
    t = [0]

    def sample_and_step():
        KT.sample_crops(stack, 32, 10, 0, t[0] * 32, out=crops)
        tr._launch(f, crops, KT.EMD_K_TRAIN_UPDATE, tr._elem_ptr(tr._loss_buf, 0))
        t[0] += 1

    us, reps = timed(sample_and_step, a.steps, a.warmup)
    row("sampler+step eager", (32, 10, 10), [(2, 3)], us, reps)
    us, reps = timed(lambda: tr._launch(f, crops, KT.EMD_K_TRAIN_UPDATE, tr._elem_ptr(tr._loss_buf, 0)), a.steps, a.warmup)
    row("step", (32, 10, 10), [(2, 3)], us, reps)
    trf = emdenoise.KernelDenoiserTrainer([(2, 3)], device=dev, seed=0, total_steps=big)
    for n in (1000, 10):
        buf = torch.empty((1, n), dtype=torch.float32, device=dev)
        calls = max(2, (a.steps * 5) // n)
        us, reps = timed(lambda: trf._fused(n, buf, 32, 10, src=stack), calls, 1)
        row(f"fused n={n}", (32, 10, 10), [(2, 3)], us / n, [round(v / n, 3) for v in reps])
    for S in (171, 512):
        x = torch.from_numpy(synthetic_lq(32, S, S, seed=2)[..., 0]).to(dev)
        steps = max(10, a.steps // (10 if S == 512 else 2))
        us, reps = timed(lambda: tr._launch(f, x, KT.EMD_K_TRAIN_UPDATE, tr._elem_ptr(tr._loss_buf, 0)), steps, a.warmup // 2)
        extra = {}
        if S == 512:
            bound, plain, trans = valu_bound_us(32 * S * S, 3, 2)
            pbound, pplain, ptrans = problem_bound_us(32 * S * S, 3, 2)
            extra = {"valu_bound_us": round(bound, 2), "valu_per_pixel": plain, "transcendental_per_pixel": trans,
                     "problem_bound_us": round(pbound, 2), "problem_valu_per_pixel": pplain,
                     "problem_transcendental_per_pixel": ptrans, "hbm_read_MB": round(32 * S * S * 4 / 1e6, 1)}
        row("step", (32, S, S), [(2, 3)], us, reps, **extra)
    sweep = [(d, w) for d in range(1, 6) for w in (3, 5, 7, 9, 13)]
    trs = emdenoise.KernelDenoiserTrainer(sweep, device=dev, seed=0, total_steps=big)

    def sweep_step():
        KT.sample_crops(stack, 32, 10, 0, t[0] * 32, out=crops)
        for i, ff in enumerate(trs.filters):
            trs._launch(ff, crops, KT.EMD_K_TRAIN_UPDATE, trs._elem_ptr(trs._loss_buf, i))
        t[0] += 1

    us, reps = timed(sweep_step, max(10, a.steps // 4), a.warmup // 2)
    row("sweep 5x5 sampler+steps eager", (32, 10, 10), sweep, us, reps)
    trs2 = emdenoise.KernelDenoiserTrainer(sweep, device=dev, seed=0, total_steps=big)
    buf = torch.empty((len(sweep), 1000), dtype=torch.float32, device=dev)
    us, reps = timed(lambda: trs2._fused(1000, buf, 32, 10, src=stack), 2, 1, reps=3)
    row("sweep 5x5 fused n=1000", (32, 10, 10), sweep, us / 1000, [round(v / 1000, 2) for v in reps])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
