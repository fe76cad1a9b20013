#!/usr/bin/env python3
"""Times emdenoise.resample (csrc/resample.hip) on one GPU:

    python tools/resample_bench.py [--steps K] [--warmup W] [--out profiles/resample_bench.json]

With HIP events after warm-up, in one process: ``resize`` at [4,4096,4096] -> 2048 x 2048 AREA (whole ratio 2: the block form),
[32,2048,2048] -> 512 x 512 AREA and CUBIC (the reference's load_image), [8,512,512] -> 1024 x 1024 LINEAR and CUBIC,
[8,2048,2048] -> 2047 x 2047 AREA (the general run form), and ``crop_resize`` of 32 random boxes with sides 512..2048 to 512 x 512
AREA.  Beside each: (i) a device-to-device copy that moves the same number of bytes as the call's traffic by design (it reads its
source rectangle once and writes its output, 4 B each), and the call's rate as a fraction of that copy's; (ii)
``torch.nn.functional.interpolate`` in the nearest matching mode on the same GPU -- a beside-number, not the same arithmetic: torch's
``area`` is adaptive average pooling (equal to cv2 only at whole ratios), its ``bicubic`` and ``bilinear`` keep the coordinate in the
compute type and accumulate in float32.

The yardstick that matters is ``harvest.box_resize`` at [4,4096,4096] -> 2048: the kernel this one descends from, reading the same
bytes.  ``yardstick`` holds both calls alternating in one loop (each between its own pair of events), and ``box_resize`` alternating
with itself: the spread a difference has to exceed.  ``kernel_specialisations`` holds the A/B of the one specialisation kept: the kernel instance whose inner
loop is written for the fixed forms (at most four taps a sample: nearest, linear, cubic, emulated area) against the instance whose loop
serves every form (the development knob ``resize_generic``), alternating on the same call."""
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

TORCH_MODE = {"nearest": "nearest", "linear": "bilinear", "cubic": "bicubic", "area": "area"}


def alternating(fa, fb, steps, warmup):
    """Medians (us) of fa and fb called in turn, each call between its own pair of HIP events, and the median of the per-step ratio."""
    import torch

    for _ in range(warmup):
        fa(), fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(steps):
        for fn, ts in ((fa, ta), (fb, tb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
    ta, tb = np.array(ta), np.array(tb)
    return float(np.median(ta)), float(np.median(tb)), float(np.median(tb / ta))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_bench.json"))
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F

    from emdenoise import _lib, harvest, resample

    dev = torch.device("cuda", 0)
    rows = []

    def images(B, H, W, seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        return torch.poisson(torch.rand((B, H, W), device=dev, generator=g) * 300.0 + 20.0, generator=g) - 25.0

    def copy_us(nbytes):
        n = int(nbytes // 8)
        src, dst = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
        us = timed(lambda: dst.copy_(src), a.steps, a.warmup)[0]
        del src, dst
        return us

    def row(name, shape, out, mode, ours, nbytes, beside):
        us, us_min = timed(ours, a.steps, a.warmup)
        cus = copy_us(nbytes)
        r = {"what": name, "shape": list(shape), "to": list(out), "interpolation": mode, "us": round(us, 1), "us_min": round(us_min, 1),
             "bytes": int(nbytes), "TB_per_s": round(nbytes / (us * 1e-6) / 1e12, 3), "same_bytes_copy_us": round(cus, 1),
             "fraction_of_copy_rate": round(cus / us, 3),
             "torch_interpolate_beside_us": round(timed(beside, a.steps, a.warmup)[0], 1), "torch_interpolate_mode": TORCH_MODE[mode]}
        rows.append(r)
        print(json.dumps(r), flush=True)

    def interpolate(x, hw, mode):
        kw = {} if mode in ("nearest", "area") else {"align_corners": False}
        return F.interpolate(x[:, None], size=hw, mode=TORCH_MODE[mode], **kw)

    def ab(name, shape, out, mode, ours):
        """The kernel's two instances on the same call, alternating: the fixed forms' inner loop against the loop for every form."""
        def generic():
            _lib.knob("resize_generic", 1)
            try:
                return ours()
            finally:
                _lib.knob("resize_generic", 0)

        same = bool(torch.equal(ours(), generic()))
        kept, gen, ratio = alternating(ours, generic, a.steps, a.warmup)
        r = {"what": name, "shape": list(shape), "to": list(out), "interpolation": mode, "fixed_form_loop_us": round(kept, 1),
             "generic_loop_us": round(gen, 1), "generic_over_fixed_form": round(ratio, 3), "same_bits": same}
        abs_.append(r)
        print(json.dumps(r), flush=True)

    yard, abs_ = {}, []
    for (B, H, W), (h, w), modes in (((4, 4096, 4096), (2048, 2048), ("area",)), ((32, 2048, 2048), (512, 512), ("area", "cubic")),
                                     ((8, 512, 512), (1024, 1024), ("linear", "cubic")), ((8, 2048, 2048), (2047, 2047), ("area",))):
        x = images(B, H, W, 1)
        for mode in modes:
            row("resize", (B, H, W), (h, w), mode, lambda: resample.resize(x, (w, h), mode), 4.0 * B * (H * W + h * w),
                lambda: interpolate(x, (h, w), mode))
            if mode != "area":   # true area runs the loop that serves every form: there is one instance to time
                ab("resize", (B, H, W), (h, w), mode, lambda: resample.resize(x, (w, h), mode))
        if H == 4096:
            box = lambda: harvest.box_resize(x, 2048)
            new = lambda: resample.resize(x, 2048, "area")
            same = bool(torch.equal(box(), new()))   # at a whole ratio the two kernels compute the same mean
            b0, n0, ratio = alternating(box, new, a.steps, a.warmup)
            s0, s1, spread = alternating(box, box, a.steps, a.warmup)
            yard = {"shape": [B, H, W], "to": [h, w], "box_resize_us": round(b0, 1), "resize_area_us": round(n0, 1),
                    "resize_over_box_resize": round(ratio, 3), "box_resize_against_itself_us": [round(s0, 1), round(s1, 1)],
                    "box_resize_against_itself_ratio": round(spread, 3), "same_bits": same}
            print(json.dumps(yard), flush=True)
        del x
        torch.cuda.empty_cache()

    B, S = 32, 2048
    x = images(B, S, S, 2)
    rng = np.random.default_rng(3)
    sides = rng.integers(512, S + 1, size=(B, 2))
    boxes = np.stack([rng.integers(0, S - sides[:, 0] + 1), rng.integers(0, S - sides[:, 1] + 1), sides[:, 0], sides[:, 1]], axis=1)
    bd = torch.from_numpy(boxes.astype(np.int32)).to(dev)
    crops = lambda: [F.interpolate(x[b:b + 1, None, y0:y0 + bh, x0:x0 + bw], size=(512, 512), mode="area") for b, (x0, y0, bw, bh) in enumerate(boxes)]
    row("crop_resize (32 random boxes, sides 512..2048; beside: 32 interpolate calls)", (B, S, S), (512, 512), "area",
        lambda: resample.crop_resize(x, bd, 512, "area"), 4.0 * (float((sides[:, 0] * sides[:, 1]).sum()) + B * 512 * 512), crops)

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""),
                   "steps": a.steps, "rows": rows, "yardstick": yard, "kernel_specialisations": abs_},
                  fh, indent=1)


if __name__ == "__main__":
    main()
