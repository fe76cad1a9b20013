#!/usr/bin/env python3
"""Times the refinement of crop centres and defocuses (csrc/exitwave.hip) on one GPU:

    python tools/exitwave_refine_bench.py [--steps K] [--warmup W] [--out profiles/exitwave_refine_bench.json]

Medians of K calls, each between its own pair of HIP events, after warm-up, all in one process.  A series of N = 8 frames of 1024
pixels a side, crops of 256 and of 512, 10 iterations: ``refine_params`` with one round and with eight, beside the loop a user runs
without it -- ``crop_stack`` + ``reconstruction_loss`` for each of the 6 (N - 1) = 42 polls of a round, the loss read back after every
call, the decision on the host.  Both make the same decisions on the same bits, which the tool checks.

Then one refinement with 50 iterations at 256: whether the centres and the relative defocuses end nearer to the truth than the seed
is recorded as numbers, with no pass / fail attached (at small sizes they do not: DESIGN.md 3.30)."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.filter_bench import timed  # noqa: E402

LAM, PX, ITERS, N, S0 = 2.51e-12, 1e-10, 10, 8, 1024
STEPS = (1.0, 4e-9)


def series(side, np, torch, exitwave, dev):
    """Frames |P(wave, df_k)| of a smooth object confined to the middle (a Gaussian envelope of width side / 5), drifted by whole
    pixels; the true centres and defocuses; the seed (the truth perturbed by -1..1 px and up to 4e-9); the anchor."""
    rng = np.random.default_rng(11)
    anchor = N // 2
    k = np.arange(N, dtype=np.float64) - anchor
    df = 2e-8 * np.sign(k) * k * k + 1e-8
    g = torch.Generator(device=dev).manual_seed(5)
    noise = torch.randn((2, S0, S0), device=dev, generator=g, dtype=torch.float64)
    f = torch.fft.fftfreq(S0, device=dev, dtype=torch.float64)
    low = torch.exp(-(f[:, None] ** 2 + f[None, :] ** 2) / (2 * 0.02 ** 2))
    u, v = torch.fft.ifft2(torch.fft.fft2(noise) * low).real
    u, v = (u - u.mean()) / u.std(), (v - v.mean()) / v.std()
    y = torch.arange(S0, device=dev, dtype=torch.float64) - S0 / 2
    env = torch.exp(-(y[:, None] ** 2 + y[None, :] ** 2) / (2.0 * (side / 5.0) ** 2))
    wave = 1.0 + ((1.0 + 0.1 * u) * torch.exp(0.3j * v) - 1.0) * env
    drift = rng.integers(-2, 3, size=(N, 2))
    drift[anchor] = 0
    frames = exitwave.propagate(wave[None].expand(N, S0, S0).contiguous(), df, LAM, px=PX).abs().to(torch.float32)
    frames = torch.stack([torch.roll(frames[i], (int(drift[i][1]), int(drift[i][0])), (0, 1)) for i in range(N)]).contiguous()
    centres = S0 / 2.0 + drift.astype(np.float64)
    c0 = centres + rng.uniform(-1.0, 1.0, size=(N, 2))
    d0 = df + rng.uniform(-4e-9, 4e-9, size=N)
    c0[anchor], d0[anchor] = centres[anchor], df[anchor]
    return frames, centres, df, c0, d0, anchor


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exitwave_refine_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch

    from emdenoise import exitwave

    dev = torch.device("cuda", 0)
    rows = []
    polls = exitwave.refine_polls(N, N // 2)
    Q = 2 * len(polls)

    def note(r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    for side in (256, 512):
        frames, centres, df, c0, d0, anchor = series(side, np, torch, exitwave, dev)
        kw = dict(px=PX, iterations=ITERS)
        up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)

        def loop(rounds):
            """The compass search with one crop and one reconstruction per poll and the decisions on the host."""
            c, d, steps = c0.copy(), d0.copy(), np.array(STEPS)
            loss = lambda cc, dd: float(exitwave.reconstruction_loss(exitwave.crop_stack(frames, up(cc), side), up(dd), LAM, **kw))
            best, choices = loss(c, d), []
            for _ in range(rounds):
                cands = []
                for q in range(Q):
                    axis, k = polls[q // 2]
                    cc, dd = c.copy(), d.copy()
                    if axis == 2:
                        dd[k] = dd[k] - steps[1] if q & 1 else dd[k] + steps[1]
                    else:
                        cc[k, axis] = cc[k, axis] - steps[0] if q & 1 else cc[k, axis] + steps[0]
                    cands.append((loss(cc, dd), cc, dd))
                i = int(np.argmin([l for l, _, _ in cands]))
                if cands[i][0] < best:
                    best, c, d = cands[i]
                    choices.append(i)
                else:
                    steps = steps * 0.5
                    choices.append(-1)
            return best, choices

        seed = (up(c0), up(d0), up(np.array(STEPS)))

        def batched(rounds):   # the seed is on the device: launches only
            return exitwave.refine_params(frames, seed[0], seed[1], LAM, side, step_xy=seed[2], rounds=rounds, **kw)

        got, (best, choices) = batched(8), loop(8)
        same = got.history_choice.tolist() == choices and float(got.loss) == best
        for rounds in (1, 8):
            tb = timed(lambda: batched(rounds), a.steps, a.warmup)
            tl = timed(lambda: loop(rounds), a.steps, a.warmup)
            chunks = -(-Q // min(Q, exitwave.MAX_CANDIDATES))
            note({"what": f"refine_params, {rounds} round(s) of {Q} polls, {ITERS} iterations", "frames": [N, S0, S0], "side": side,
                  "batched_us": round(tb[0], 1), "batched_us_min": round(tb[1], 1), "loop_us": round(tl[0], 1), "loop_us_min": round(tl[1], 1),
                  "loop_over_batched": round(tl[0] / tb[0], 2), "same_decisions_and_loss_bits": bool(same),
                  "launches_batched": 2 * ITERS + 11 + rounds * (chunks * (2 * ITERS + 8) + 1),
                  "launches_loop": (1 + rounds * Q) * (2 * ITERS + 7)})
        if side == 256:
            r = exitwave.refine_params(frames, c0, d0, LAM, side, step_xy=STEPS[0], step_defocus=STEPS[1], rounds=8, px=PX, iterations=50)
            cerr = lambda c: float(np.abs(np.asarray(c) - centres).max())
            derr = lambda d: float(np.abs((np.asarray(d) - df) / df).max())
            rc, rd = r.centres.cpu().numpy(), r.defocuses.cpu().numpy()
            note({"what": "refine_params, 8 rounds, 50 iterations: distance from the true parameters", "frames": [N, S0, S0], "side": side,
                  "loss_seed": float(r.loss0), "loss_result": float(r.loss), "moves": r.moves, "choices": r.history_choice.tolist(),
                  "largest_centre_error_px_seed": cerr(c0), "largest_centre_error_px_result": cerr(rc),
                  "largest_relative_defocus_error_seed": derr(d0), "largest_relative_defocus_error_result": derr(rd),
                  "centre_error_shrank": cerr(rc) < cerr(c0), "defocus_error_shrank": derr(rd) < derr(d0)})
        del frames
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""),
                   "steps": a.steps, "iterations": ITERS, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
