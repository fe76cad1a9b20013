#!/usr/bin/env python3
"""The bits of the exit-wave operations (csrc/exitwave.hip) on seeded inputs, for a change that must not
move them: the sha256 of every output array of a fixed list of cases, one JSON object {case: {array: sha256}}.

    python tools/exitwave_bits.py --out A.json          (once in a work tree of each commit, one process each)
    python tools/exitwave_bits.py --compare A.json B.json

The cases are the smallest that reach every instance and branch: ``reconstruct`` at 8, 256, 512, 1024 and 2048 pixels a side (the
column kernel's 1, 1, 2, 4 and 8 elements per thread) with 1 and 3 iterations, every combination of its optional outputs, from
intensities, one image of 4096 (16 elements), with padding, and composed; ``reconstruct_candidates`` with 1 and 3 candidates of 1 and
3 images, padded, chunked; both methods of ``defocus_search``; ``propagate`` and ``fft2``, which share the pass kernel."""
from __future__ import annotations

import argparse
import hashlib
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LAM, PX = 2.51e-12, 1e-10


def series(N, s, seed=3):
    """N float32 images of side s around 1, a few of them with a negative and a zero pixel, and their defocuses."""
    x = (1.0 + 0.1 * (np.random.default_rng(seed).random((N, s, s)) - 0.5)).astype(np.float32)
    x[0, 1, 2], x[-1, 3, 1] = -0.5, 0.0
    k = np.arange(N, dtype=np.float64) - N // 2
    return x, 2e-9 * np.sign(k) * k * k + 1e-8


def cases():
    """(name, thunk -> tuple of arrays), in a fixed order."""
    from emdenoise import exitwave as ew

    def recon(N, s, **kw):
        x, d = series(N, s)
        return lambda: ew.reconstruct(x, d, LAM, px=PX, **kw)

    for s, it in itertools.product((8, 256, 512, 1024, 2048), (1, 3)):
        yield f"reconstruct [3,{s},{s}], {it} iterations", recon(3, s, iterations=it)
    for s, stack, losses in itertools.product((8, 512), (False, True), (False, True)):
        yield f"reconstruct [3,{s},{s}], 3 iterations, stack {stack}, losses {losses}", recon(3, s, iterations=3, return_stack=stack, return_losses=losses)
    for s in (8, 512):
        yield f"reconstruct [3,{s},{s}] from intensities", recon(3, s, iterations=3, from_intensity=True, return_stack=True, return_losses=True)
    yield "reconstruct [1,4096,4096], 1 iteration", recon(1, 4096, iterations=1, return_losses=True)
    for s in (8, 64):
        yield f"reconstruct [2,{s},{s}], pad_periods 1", recon(2, s, iterations=2, pad_periods=1, return_stack=True, return_losses=True)
    yield "reconstruct [3,64,64] composed", recon(3, 64, iterations=2, _composed=True, return_stack=True, return_losses=True)

    def cand(C, N, s, **kw):
        x, d = series(N, s)
        table = np.linspace(0.6, 1.5, C)[:, None] * d[None, :]
        return lambda: (*ew.reconstruct_candidates(x, table, LAM, px=PX, iterations=3, per_image=True, return_waves=True, return_stack=True, **kw),
                        ew.reconstruct_candidates(x, table, LAM, px=PX, iterations=3, **kw))

    for C, N in itertools.product((1, 3), (1, 3)):
        for s in (8, 512):
            yield f"candidates {C} of [{N},{s},{s}]", cand(C, N, s)
        yield f"candidates {C} of [{N},8,8], pad_periods 1", cand(C, N, 8, pad_periods=1)
    yield "candidates 3 of [3,8,8], 2 per launch", cand(3, 3, 8, candidates_per_launch=2)
    yield "candidates 3 of [3,512,512], 2 per launch", cand(3, 3, 512, candidates_per_launch=2)

    def search(**kw):
        x, d = series(3, 64)
        def run():
            r = ew.defocus_search(x, LAM, d / 1e-8, px=PX, iterations=3, return_wave=True, **kw)
            return (r.increment, r.loss, r.defocuses, r.history_increments, r.history_losses, r.status, r.steps, r.wave)
        return run

    yield "defocus_search section, 4 candidates, 3 rounds", search(bracket=(0.4e-8, 2.0e-8), candidates=4, rounds=3)
    yield "defocus_search plateau, 4 steps", search(method="plateau", bracket=(0.6e-8, 1.2e-8, 1e30), max_steps=4)

    for S in (8, 512):
        rng = np.random.default_rng(5)
        z = rng.standard_normal((2, S, S)) + 1j * rng.standard_normal((2, S, S))
        yield f"propagate [2,{S},{S}]", lambda z=z: ew.propagate(z, [1e-8, -2e-8], LAM, px=PX)
        yield f"fft2, ifft2 [2,{S},{S}]", lambda z=z: (ew.fft2(z), ew.ifft2(z))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", help="JSON file to write")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"), help="compare two files; exit status 1 if they differ")
    a = ap.parse_args()
    if a.compare:
        da, db = (json.load(open(p)) for p in a.compare)
        flat = lambda d: {(c, k): h for c, arrays in d.items() for k, h in arrays.items()}
        fa, fb = flat(da), flat(db)
        differ = sorted(k for k in set(fa) | set(fb) if fa.get(k) != fb.get(k))
        print(f"{len(da)} / {len(db)} cases, {len(fa)} / {len(fb)} arrays compared, {len(differ)} differ {differ}")
        return 1 if differ else 0
    out = {}
    for name, thunk in cases():
        res = thunk()
        res = res if isinstance(res, tuple) else (res,)
        out[name] = {f"{i}": hashlib.sha256(np.ascontiguousarray(np.asarray(v)).tobytes()).hexdigest() for i, v in enumerate(res) if v is not None}
        print(name, len(out[name]), flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
