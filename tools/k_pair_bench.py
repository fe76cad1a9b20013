"""Graph K paired training speed (bench.py measures the flagship inference workload and stays as it is).

    python tools/k_pair_bench.py [--steps K] [--warmup W] [--out profiles/k_pair_bench.json]

Rows (one step = the filter's forward + backward launch and its reduce + Adam launch, on a fixed device batch):
  pair step  [1,20,20]  VALID   (1,3) (1,5) (1,7)   the reference's setting: one 20 x 20 pair per step
  pair step  [32,20,20] VALID   (1,3) (1,5) (1,7)
  pair step  [32,512,512] REFLECT (2,3)             paired training at full size
Beside every paired time: the unpaired emd_k_train_step_f32 at the same shape measured in this same process (boxes differ by a few
percent, so only a ratio taken in one process means anything), the ratio paired / unpaired, and the algorithmic-bytes bound of
the paired step (x and truth read once, 8 B H W bytes, plus the partial slabs written and read back) at the HBM rate below.
  make_pairs  1024 x [160,160]                      emd_k_make_pairs_f32, with its bytes bound (both stacks read twice)
  distill     1024 x [171,171], encoding_features 16   teacher crops + make_pairs, end to end on the device
Timing as tools/k_train_bench.py: torch.cuda events around K back-to-back calls after W warm-up calls, median of 5 repeats."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.k_train_bench import timed  # noqa: E402

HBM_BYTES_PER_S = 8.0e12   # MI355X peak HBM3E rate; the bound below is bytes / this


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import emdenoise
    from emdenoise import autoencoder
    from emdenoise import k_trainer as KT
    from tests.synth_inputs import synthetic_lq

    dev = torch.device("cuda", 0)
    lib = emdenoise._lib.load()
    rows = []

    def row(name, shape, **kw):
        r = {"row": name, "shape": list(shape)}
        r.update(kw)
        rows.append(r)
        print(json.dumps(r), flush=True)

    big = 10 ** 9   # timing only: keep lr0 (1 - t / (T + 1)) positive however many steps run
    cases = [((1, 20, 20), "valid", c) for c in KT.PAIR_PRESET["configs"]]
    cases += [((32, 20, 20), "valid", c) for c in KT.PAIR_PRESET["configs"]]
    cases += [((32, 512, 512), "reflect", (2, 3))]
    for shape, pad, cfg in cases:
        B, H, W = shape
        x = torch.from_numpy(np.ascontiguousarray(synthetic_lq(B, H, W, seed=2)[..., 0])).to(dev)
        t = torch.from_numpy(np.ascontiguousarray(synthetic_lq(B, H, W, seed=3)[..., 0])).to(dev)
        tr = emdenoise.KernelDenoiserTrainer([cfg], device=dev, seed=0, lr0=0.01, total_steps=big, beta1=0.5, loss="image")
        f = tr.filters[0]
        loss = tr._elem_ptr(tr._loss_buf, 0)
        flags = KT.EMD_K_TRAIN_UPDATE | KT.EMD_K_TRAIN_SQRT_ABOVE_1
        steps = max(10, a.steps // 10) if H == 512 else a.steps
        warm = max(2, a.warmup // 2) if H == 512 else a.warmup
        us_p, reps_p = timed(lambda: tr._launch_pair(f, x, t, KT.PADS[pad], flags, loss), steps, warm)
        us_u, reps_u = timed(lambda: tr._launch(f, x, KT.EMD_K_TRAIN_UPDATE, loss), steps, warm)
        partial = lib.emd_k_train_workspace_bytes(B, H, W, cfg[1], cfg[0])
        nbytes = 8 * B * H * W + 2 * partial
        row("pair step", shape, pad=pad, config=list(cfg), us_per_step=round(us_p, 2), reps_us=reps_p,
            unpaired_us_per_step=round(us_u, 2), unpaired_reps_us=reps_u, ratio_paired_over_unpaired=round(us_p / us_u, 3),
            algorithmic_bytes=int(nbytes), bytes_bound_us=round(nbytes / HBM_BYTES_PER_S * 1e6, 3))

    N = 1024
    rng = np.random.default_rng(0)
    src = torch.from_numpy(synthetic_lq(64, 171, 171, seed=5)[..., 0].astype(np.float32)).to(dev)
    stack = src[torch.from_numpy(rng.integers(0, 64, N)).to(dev)].contiguous()   # 1024 images from 64 distinct ones
    pa = stack[:, :160, :160].contiguous()
    pb = (pa * 0.5 + 0.25).contiguous()
    calls = max(5, a.steps // 10)
    us, reps = timed(lambda: KT.make_pairs(pa, pb, seed=1), calls, 2)
    nbytes = 2 * 2 * N * 160 * 160 * 4   # two stacks, a statistics pass and (in the window only) a second read; the bound counts both whole
    row("make_pairs", (N, 160, 160), us_per_call=round(us, 1), reps_us=reps, algorithmic_bytes=nbytes,
        bytes_bound_us=round(nbytes / HBM_BYTES_PER_S * 1e6, 2))
    teacher = autoencoder.Micrograph_Autoencoder(encoding_features=16)
    us, reps = timed(lambda: KT.distill(teacher, stack, seed=1), 3, 1, reps=3)
    row("distill", (N, 171, 171), encoding_features=16, max_batch=64, us_per_call=round(us, 1), reps_us=reps,
        us_per_crop=round(us / N, 2))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "hbm_bytes_per_s": HBM_BYTES_PER_S, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
