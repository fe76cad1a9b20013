"""Whole-micrograph denoising: the host denoise() loop against the device path denoise_images().

  python tools/tile_bench.py --out profiles/tile_bench.json             # timings, host and device paths alternating
  python tools/tile_bench.py --device-only CASE --reps R                # only that class, one warm-up + R calls of denoise_images
  python tools/tile_bench.py --merge-stats CASE A.csv B.csv --reps-a RA --reps-b RB --out FILE
        # two rocprofv3 --kernel-trace --stats runs of --device-only CASE with RA < RB calls: (B - A) / (RB - RA) is the kernel time
        # of one call, with model setup, weight packing and the warm-up cancelled out

Every case starts from float32 numpy micrographs and ends with numpy results, which is what a user's call does.  Synthetic
weights; the timings do not depend on them.  Wall time is taken between device events recorded around each call (the host
work inside a call is part of it)."""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# the kernels of csrc/tile_ops.hip
TILE_KERNELS = ("prep_partial_kernel", "prep_final_kernel", "prep_write_kernel", "resize_half_pixel_kernel", "gather_copy_kernel",
                "gather_rescale_kernel", "blend_kernel", "affine_kernel")

CASES = {
    # name: (class, N, side, kwargs)
    "D_pre0_N1": ("D", 1, 2048, dict(preprocess=False, overlap=80)),
    "D_pre0_N8": ("D", 8, 2048, dict(preprocess=False, overlap=80)),
    "D_pre1_N32": ("D", 32, 2048, dict(preprocess=True)),
    "S_N1": ("S", 1, 2048, dict(overlap=25, used_overlap=1)),
    "S_N8": ("S", 8, 2048, dict(overlap=25, used_overlap=1)),
    "K23_N1": ("K", 1, 2048, dict()),
    "K23_N8": ("K", 8, 2048, dict()),
}

# algorithmic bytes of the tiling kernels (float32): every array they must touch, read or written once.  D: the image read by
# the gather, the tiles written, the predictions read, the image written (the preprocess adds the image read and one 512^2 result
# written); S: its preprocess reads and writes the image, then as D with 160^2 crops; K: the rescale and its inverse each read and
# write the image.  Statistics passes that re-read an image are not counted: they are the kernels' overhead over the bound.
def tile_bytes(name, side):
    from emdenoise import tiling

    cls, N, _, kw = CASES[name]
    img = side * side * 4
    if cls == "D":
        if kw.get("preprocess"):
            s = 512 * 512 * 4
            return N * (img + s + 4 * s)
        tiles = tiling.d_plan(side, side, 512, kw["overlap"]).tiles_per_image * 512 * 512 * 4
        return N * (2 * img + 2 * tiles)
    if cls == "S":
        crops = tiling.s_plan(side, side, 160, kw["overlap"], kw["used_overlap"]).tiles_per_image * 160 * 160 * 4
        return N * (3 * img + 2 * crops)
    return N * 4 * img


def make_inputs(N, side, seed=0):
    from tests.synth_inputs import synthetic_lq

    one = synthetic_lq(1, side, side, seed=seed)[0, :, :, 0]
    rng = np.random.default_rng(seed)
    return np.stack([np.roll(one, (int(rng.integers(side)), int(rng.integers(side))), axis=(0, 1)) for _ in range(N)])


def models(only=None):
    import emdenoise
    from emdenoise import autoencoder as AE

    p = emdenoise.KernelParams.from_symmetric([[0.1, 0.12, 0.09], [0.2, 0.1, 0.05]], [[0, 0, 0], [0.1, -0.2, 0.05]], [1.0, 0.8], 3)
    make = {"D": emdenoise.Denoiser, "S": lambda: AE.Micrograph_Autoencoder(encoding_features=16),
            "K": lambda: emdenoise.Micrograph_Autoencoder(depth=2, width=3, params=p)}
    return {k: f() for k, f in make.items() if only in (None, k)}


def host_call(model, cls, imgs, kw):
    return [model.denoise(im, **kw) for im in imgs]


def device_call(model, cls, imgs, kw):
    return model.denoise_images(imgs, **kw)


def timed(fn):
    import torch

    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t = time.perf_counter()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), (time.perf_counter() - t) * 1e3


def run(args):
    ms = models()
    out = {"device": None, "cases": {}, "note": "ms per micrograph; host = the class's denoise() per image, device = denoise_images() on "
                                                "the stack; numpy in, numpy out; event-timed, host and device calls alternating"}
    import torch

    out["device"] = torch.cuda.get_device_name(0)
    for name in args.cases or CASES:
        cls, N, side, kw = CASES[name]
        imgs = make_inputs(N, side)
        m = ms[cls]
        h, d = [], []
        host_call(m, cls, imgs, kw)           # warm-up both paths
        device_call(m, cls, imgs, kw)
        for _ in range(args.reps):
            h.append(timed(lambda: host_call(m, cls, imgs, kw))[0])
            d.append(timed(lambda: device_call(m, cls, imgs, kw))[0])
        hm, dm = float(np.median(h)) / N, float(np.median(d)) / N
        out["cases"][name] = {"class": cls, "N": N, "side": side, "kwargs": kw, "reps": args.reps,
                              "host_ms_per_image": round(hm, 3), "device_ms_per_image": round(dm, 3), "speedup": round(hm / dm, 2),
                              "host_ms_per_image_min_max": [round(min(h) / N, 3), round(max(h) / N, 3)],
                              "device_ms_per_image_min_max": [round(min(d) / N, 3), round(max(d) / N, 3)],
                              "speedup_worst": round(min(h) / max(d), 2),
                              "host_ms_all": [round(v, 2) for v in h], "device_ms_all": [round(v, 2) for v in d],
                              "tile_kernel_bytes": tile_bytes(name, side)}
        print(json.dumps({name: out["cases"][name]}), flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


def device_only(args):
    import torch

    cls, N, side, kw = CASES[args.device_only]
    m = models(cls)[cls]
    imgs = make_inputs(N, side)
    device_call(m, cls, imgs, kw)
    torch.cuda.synchronize()
    for _ in range(args.reps):
        device_call(m, cls, imgs, kw)
    torch.cuda.synchronize()


def _kernel_ns(path):
    """{kernel name: total ns} of a rocprofv3 kernel_stats.csv"""
    return {r["Name"]: float(r["TotalDurationNs"]) for r in csv.DictReader(open(path))}


def merge_stats(args):
    name, path_a, path_b = args.merge_stats
    a, b = _kernel_ns(path_a), _kernel_ns(path_b)
    calls = args.reps_b - args.reps_a
    per = {k: (b.get(k, 0.0) - a.get(k, 0.0)) / calls for k in set(a) | set(b)}
    tot = sum(per.values())
    tile = {}
    for k, v in per.items():
        for t in TILE_KERNELS:
            if t in k:
                tile[t] = tile.get(t, 0.0) + v
    tile_ns = sum(tile.values())
    with open(args.out) as f:
        doc = json.load(f)
    c = doc["cases"][name]
    c["kernel_trace"] = {"how": f"(trace of {args.reps_b} calls - trace of {args.reps_a} calls) / {calls}, only this class built",
                         "all_kernels_us_per_call": round(tot / 1e3, 1), "tile_kernels_us_per_call": round(tile_ns / 1e3, 1),
                         "tile_kernel_share": round(tile_ns / tot, 4),
                         "tile_kernels_bound_us_at_8TBps": round(c["tile_kernel_bytes"] / 8e12 * 1e6, 1),
                         "by_kernel_us_per_call": {k: round(v / 1e3, 1) for k, v in sorted(tile.items())},
                         "other_kernels_us_per_call": {k[:90]: round(v / 1e3, 1) for k, v in sorted(per.items(), key=lambda kv: -kv[1])
                                                       if not any(t in k for t in TILE_KERNELS) and v / 1e3 >= 1.0}}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps({name: c["kernel_trace"]}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/tile_bench.json")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cases", nargs="*")
    ap.add_argument("--device-only")
    ap.add_argument("--merge-stats", nargs=3)
    ap.add_argument("--reps-a", type=int, default=2)
    ap.add_argument("--reps-b", type=int, default=7)
    a = ap.parse_args()
    if a.merge_stats:
        merge_stats(a)
    elif a.device_only:
        device_only(a)
    else:
        run(a)
