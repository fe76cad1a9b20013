"""Graph S training speed (bench.py measures the flagship inference workload and stays as it is).

    python tools/s_train_bench.py [--steps K] [--warmup W] [--out profiles/s_train_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -o s -- python tools/s_train_bench.py --trace-run
    python tools/s_train_bench.py --merge-stats DIR/.../s_kernel_stats.csv [--out ...]

Rows, at [32,160,160] (the reference's batch and crop, autoencoder.py:41-45), one step = forward on batch statistics, reverse
pass, Adam and the weight re-pack on a fixed batch:
  step eager / captured       encoding_features 16, 4 and 1; captured = one torch.cuda.graph replay per step (single stream)
  head fused / composed       the loss + last two layers' reverse pass alone: emd_s_head_bwd_f32 against emd_s_mse_loss_f32 +
                              emd_conv3x3_cout1_wgrad_f32 + emd_conv3x3_cout1_bwd_data_f32 + emd_relu_mask_bwd_f32 + the bias reduce
Algorithmic HBM bytes of a step: every tensor the step keeps (each layer's depthwise output d, conv output r and activation a,
the input and the output) is written once and read once in the forward pass, and its gradient is written once and read once
in the reverse pass: bytes = 4 * 4 * sum(elements).  The bound is bytes / HBM_PEAK; the ratio is measured time / bound.
Timing: torch.cuda events around K back-to-back steps after W warm-up steps, median of 5 repeats."""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12   # MI355X HBM3E, bytes/s (nominal)
B, S = 32, 160


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


def step_elements(enc, B=B, S=S):
    p4 = lambda c: -(-c // 4) * 4
    n = B * S * S * 4 + B * S * S            # input (4 channels) and output
    h, ci = S, 4
    for co, st in ((64, 2), (128, 2), (256, 2), (p4(enc), 1)):
        h = -(-h // st)
        n += B * h * h * (ci + 2 * co)       # d, r, a
        ci = co
    for co in (256, 128, 64):
        h *= 2
        n += B * h * h * co * (2 if co != 64 else 1)   # r and a (the last transposed conv writes a only)
    return n


def batch():
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:S, 0:S] / S
    return (1.0 + 0.5 * np.sin(6 * yy[None] + 4 * xx[None] + rng.random((B, 1, 1)) * 6)
            + 0.3 * rng.standard_normal((B, S, S))).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "s_train_bench.json"))
    ap.add_argument("--trace-run", action="store_true", help="only 20 captured steps (for a kernel trace)")
    ap.add_argument("--merge-stats", default=None, help="a rocprofv3 kernel_stats.csv to summarise into --out")
    a = ap.parse_args()
    if a.merge_stats:
        with open(a.merge_stats) as f:
            rows = list(csv.DictReader(f))
        rows.sort(key=lambda r: -float(r["TotalDurationNs"]))
        total = sum(float(r["TotalDurationNs"]) for r in rows)
        # steps in the trace = launches of a once-per-step kernel (the run also holds the warm-up and the capturing step)
        steps = int(next(r for r in rows if "s_head_bwd_kernel" in r["Name"])["Calls"])
        d = json.load(open(a.out))
        d["kernel_trace"] = {"run": "tools/s_train_bench.py --trace-run: encoding_features 16, [32,160,160]; one eager warm-up step, "
                                    "the capturing step and 20 replays", "steps": steps,
                             "device_us_per_step": round(total / 1e3 / steps, 1),
                             "top": [{"kernel": r["Name"][:120], "calls": int(r["Calls"]), "us_per_step": round(float(r["TotalDurationNs"]) / 1e3 / steps, 1),
                                      "percent": round(100 * float(r["TotalDurationNs"]) / total, 1)} for r in rows[:15]]}
        json.dump(d, open(a.out, "w"), indent=1)
        print(json.dumps(d["kernel_trace"], indent=1))
        return

    import torch

    import emdenoise
    from emdenoise import autoencoder_trainer as AT
    from emdenoise import ops

    dev = torch.device("cuda", 0)
    x = torch.from_numpy(batch()).to(dev)
    if a.trace_run:
        tr = AT.AutoencoderTrainer(16, device=dev)
        tr.train_step(x, graph=True)
        torch.cuda.synchronize()
        for _ in range(20):
            tr.train_step(x, graph=True)
        torch.cuda.synchronize()
        return
    rows = []
    for enc in (16, 4, 1):
        tr = AT.AutoencoderTrainer(enc, device=dev, total_steps=10 ** 9, period=10 ** 9)
        byts = 16 * step_elements(enc)
        bound = byts / HBM_PEAK * 1e6
        for graph in (False, True):
            us, reps = timed(lambda: tr.train_step(x, graph=graph), a.steps, a.warmup)
            rows.append({"name": "step captured" if graph else "step eager", "encoding_features": enc, "shape": [B, S, S],
                         "us_per_step": round(us, 1), "reps": reps, "algorithmic_bytes": byts, "hbm_bound_us": round(bound, 1),
                         "ratio_to_bound": round(us / bound, 2)})
            print(rows[-1])
    rng = np.random.default_rng(1)
    act = torch.from_numpy(np.maximum(rng.standard_normal((B, S, S, 64)), 0).astype(np.float32)).to(dev)
    out = torch.from_numpy(rng.standard_normal((B, S, S)).astype(np.float32)).to(dev)
    w9 = torch.from_numpy((rng.standard_normal((9, 64)) * 0.1).astype(np.float32)).to(dev)
    dw, db, loss = torch.zeros(9, 64, device=dev), torch.zeros(64, device=dev), torch.zeros(1, device=dev)
    da = ops.Act.empty(B, S, S, 64, dev)
    for fused in (True, False):
        us, reps = timed(lambda: AT.head_backward(out, x, ops.Act(act), w9, dw, db, loss, da=da, fused=fused), a.steps, a.warmup)
        byts = 4 * (2 * B * S * S + 2 * B * S * S * 64)   # out, x; a read, da written
        rows.append({"name": "head fused" if fused else "head composed", "shape": [B, S, S, 64], "us": round(us, 1), "reps": reps,
                     "algorithmic_bytes": byts, "hbm_bound_us": round(byts / HBM_PEAK * 1e6, 1),
                     "ratio_to_bound": round(us / (byts / HBM_PEAK * 1e6), 2)})
        print(rows[-1])
    d = {"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK,
         "bytes_formula": "4 bytes * 4 passes * sum of the elements of every kept tensor (input, d/r/a per layer, output)", "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(d, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
