"""CPU tests of whole-micrograph tiling (emdenoise.tiling, csrc/tile_ops.hip): the plans reproduce the tile positions of the
host denoise() methods, every output pixel is covered, and the new C entry points reject bad arguments before any launch."""
import ctypes

import numpy as np
import pytest

from emdenoise import _lib, tiling


# ---- the host methods' formulas, restated (denoiser.Denoiser.denoise, autoencoder.Micrograph_Autoencoder.denoise)
def host_d_starts(n, cs=512, overlap=80):
    num = (n - cs + (cs - overlap) - 1) // (cs - overlap) + 1 if n > cs else 1
    return [int(round(i * (n - cs) / max(num - 1, 1))) for i in range(num)]


def host_s_positions(H, W, cs=160, overlap=25, used_overlap=1):
    overlap = max(overlap, used_overlap)
    Hp, Wp = H + 2 * overlap, W + 2 * overlap
    step = cs - 2 * overlap

    def starts(n):
        s = list(range(0, max(n - cs, 0) + 1, step))
        if s[-1] != n - cs:
            s.append(n - cs)
        return s

    return starts(Hp), starts(Wp), overlap, overlap - used_overlap


@pytest.mark.parametrize("n", [512, 513, 600, 700, 945, 947, 1031, 2047, 2048, 4096])
@pytest.mark.parametrize("overlap", [0, 80, 200])
def test_d_plan_matches_host(n, overlap):
    assert tiling.d_starts(n, 512, overlap) == host_d_starts(n, 512, overlap)
    p = tiling.d_plan(n, 700, 512, overlap)
    assert p.ys == host_d_starts(n, 512, overlap) and p.xs == host_d_starts(700, 512, overlap)
    assert (p.pad, p.m, p.cs) == (0, 0, 512)


def test_d_plan_rounds_half_to_even():
    # 945: three tiles, the middle one at 433/2 = 216.5 -> 216; 947: 435/2 = 217.5 -> 218 (Python's round, not floor(x + .5))
    assert tiling.d_starts(945, 512, 80) == [0, 216, 433]
    assert tiling.d_starts(947, 512, 80) == [0, 218, 435]


@pytest.mark.parametrize("shape", [(110, 110), (230, 301), (2048, 2048), (160, 500)])
@pytest.mark.parametrize("ov", [(25, 1), (25, 25), (10, 3), (1, 25)])
def test_s_plan_matches_host(shape, ov):
    H, W = shape
    overlap, used = ov
    ys, xs, ovl, m = host_s_positions(H, W, 160, overlap, used)
    p = tiling.s_plan(H, W, 160, max(overlap, used), used)
    assert p.ys == ys and p.xs == xs and p.pad == ovl and p.m == m
    if ov == (25, 25):
        assert p.m == 0          # overlap == used_overlap: the whole crop is kept
    if shape == (2048, 2048) and ov == (25, 1):
        assert p.tiles_per_image == 19 * 19


def brute_cover(starts, n, pad, cs, m):
    out = []
    for y in range(n):
        hit = [i for i, s in enumerate(starts) if s + m <= y + pad < s + cs - m]
        out.append(hit)
    return out


@pytest.mark.parametrize("case", ["d945", "d2048", "s110", "s230x301_10_3", "s2048", "s_flat_used"])
def test_every_output_pixel_is_covered(case):
    plans = {
        "d945": tiling.d_plan(945, 1031, 512, 80),
        "d2048": tiling.d_plan(2048, 2048, 512, 80),
        "s110": tiling.s_plan(110, 110, 160, 25, 1),
        "s230x301_10_3": tiling.s_plan(230, 301, 160, 10, 3),
        "s2048": tiling.s_plan(2048, 2048, 160, 25, 1),
        "s_flat_used": tiling.s_plan(300, 170, 160, 25, 25),
    }
    p = plans[case]
    for starts, n, rng in ((p.ys, p.H, p.row_range), (p.xs, p.W, p.col_range)):
        brute = brute_cover(starts, n, p.pad, p.cs, p.m)
        assert rng.shape == (n, 2) and rng.dtype == np.int32
        for y, hit in enumerate(brute):
            assert hit, f"{case}: position {y} is covered by no tile"
            assert list(range(rng[y, 0], rng[y, 1])) == hit, (case, y)


def host_overlap_count(p):
    """The host's contributions array over the core, restated."""
    cnt = np.zeros((p.H + 2 * p.pad, p.W + 2 * p.pad))
    for y in p.ys:
        for x in p.xs:
            cnt[y + p.m:y + p.cs - p.m, x + p.m:x + p.cs - p.m] += 1
    return cnt[p.pad:p.pad + p.H, p.pad:p.pad + p.W]


@pytest.mark.parametrize("plan", [lambda: tiling.d_plan(1031, 2047, 512, 80), lambda: tiling.s_plan(230, 301, 160, 25, 1)])
def test_cover_counts_match_host_contributions(plan):
    p = plan()
    rows = p.row_range[:, 1] - p.row_range[:, 0]
    cols = p.col_range[:, 1] - p.col_range[:, 0]
    np.testing.assert_array_equal(np.outer(rows, cols), host_overlap_count(p))


# ---- C ABI: validation runs before any launch, so it needs no GPU
NULL = ctypes.c_void_p(0)
A = ctypes.c_void_p(256)
B = ctypes.c_void_p(512)
Cp = ctypes.c_void_p(768)


def test_tile_constants_match_the_header(repo_root):
    import os
    import re

    text = open(os.path.join(repo_root, "include", "emdenoise.h")).read()
    got = {k: int(v) for k, v in re.findall(r"#define (EMD_TILE_PREP_[A-Z]) (\d+)", text)}
    assert got == {"EMD_TILE_PREP_S": tiling.PREP_S, "EMD_TILE_PREP_K": tiling.PREP_K, "EMD_TILE_PREP_D": tiling.PREP_D}


def test_prep_validation_needs_no_gpu():
    lib = _lib.load()
    ws = lib.emd_tile_prep_workspace_bytes(2, 64, 64, tiling.PREP_S, 0)
    assert ws > 0 and lib.emd_tile_prep_workspace_bytes(0, 64, 64, 0, 0) == 0
    assert lib.emd_tile_prep_workspace_bytes(1, 64, 64, tiling.PREP_D, 512) > lib.emd_tile_prep_workspace_bytes(1, 64, 64, tiling.PREP_S, 0)
    f = lib.emd_tile_prep_f32
    assert f(NULL, B, 2, 64, 64, tiling.PREP_S, 0, None, Cp, ws, NULL) == -1 and b"null" in lib.emd_last_error()
    assert f(A, B, 2, 64, 64, tiling.PREP_S, 0, None, NULL, ws, NULL) == -1
    assert f(A, B, 0, 64, 64, tiling.PREP_S, 0, None, Cp, ws, NULL) == -1
    assert f(A, B, -3, 64, 64, tiling.PREP_S, 0, None, Cp, ws, NULL) == -1
    assert f(A, B, 2, 0, 64, tiling.PREP_S, 0, None, Cp, ws, NULL) == -1
    assert f(A, B, 2, 64, 64, 7, 0, None, Cp, ws, NULL) == -1 and b"mode" in lib.emd_last_error()
    assert f(A, B, 2, 64, 64, tiling.PREP_S, 0, None, Cp, ws - 1, NULL) == -1 and b"workspace" in lib.emd_last_error()
    wk = lib.emd_tile_prep_workspace_bytes(2, 64, 64, tiling.PREP_K, 1)
    assert f(A, B, 2, 64, 64, tiling.PREP_K, 1, None, Cp, wk, NULL) == -1 and b"stats" in lib.emd_last_error()
    assert f(A, B, 2, 4, 64, tiling.PREP_K, 4, A, Cp, wk, NULL) == -1 and b"pad" in lib.emd_last_error()
    wd = lib.emd_tile_prep_workspace_bytes(2, 64, 64, tiling.PREP_D, 512)
    assert f(A, A, 2, 64, 64, tiling.PREP_D, 512, None, Cp, wd, NULL) == -1 and b"alias" in lib.emd_last_error()
    assert f(A, B, 2, 64, 64, tiling.PREP_D, 0, None, Cp, wd, NULL) == -1
    assert f(A, B, 70000, 8, 8, tiling.PREP_S, 0, None, Cp, lib.emd_tile_prep_workspace_bytes(70000, 8, 8, 0, 0), NULL) == -2


def test_gather_validation_needs_no_gpu():
    lib = _lib.load()
    g = lib.emd_tile_gather_f32
    # src N H W pad cs ys ny xs nx t0 count out crop_stats stream
    assert g(NULL, 1, 300, 300, 25, 160, A, 3, A, 3, 0, 9, B, None, NULL) == -1 and b"null" in lib.emd_last_error()
    assert g(A, 1, 300, 300, 25, 160, NULL, 3, A, 3, 0, 9, B, None, NULL) == -1
    assert g(A, 1, 300, 300, 25, 160, A, 3, A, 3, 0, 9, NULL, Cp, NULL) == -1
    assert g(A, 0, 300, 300, 25, 160, A, 3, A, 3, 0, 9, B, None, NULL) == -1
    assert g(A, -1, 300, 300, 25, 160, A, 3, A, 3, 0, 9, B, None, NULL) == -1
    assert g(A, 1, 300, 300, 25, 160, A, 3, A, 3, 0, 0, B, None, NULL) == -1
    assert g(A, 1, 100, 300, 25, 160, A, 3, A, 3, 0, 9, B, None, NULL) == -1 and b"padded" in lib.emd_last_error()   # 150 < 160
    assert g(A, 1, 300, 300, 25, 160, A, 3, A, 3, 5, 5, B, None, NULL) == -1 and b"plan" in lib.emd_last_error()     # 10 > 9 tiles
    assert g(A, 1, 300, 300, -1, 160, A, 3, A, 3, 0, 9, B, None, NULL) == -1


def test_blend_validation_needs_no_gpu():
    lib = _lib.load()
    b = lib.emd_tile_blend_f32
    # preds crop_stats N H W pad cs m ys ny xs nx row_range col_range clip out stream
    ok = (A, None, 1, 300, 300, 25, 160, 24, A, 3, A, 3, A, A, 0, B, NULL)

    def call(**kw):
        names = ["preds", "cst", "N", "H", "W", "pad", "cs", "m", "ys", "ny", "xs", "nx", "rr", "cr", "clip", "out", "st"]
        args = dict(zip(names, ok))
        args.update(kw)
        return b(*[args[k] for k in names])

    assert call(preds=NULL) == -1 and b"null" in lib.emd_last_error()
    assert call(rr=NULL) == -1
    assert call(out=NULL) == -1
    assert call(N=0) == -1 and call(N=-2) == -1
    assert call(H=100) == -1 and b"padded" in lib.emd_last_error()
    assert call(m=80) == -1 and b"cs/2" in lib.emd_last_error()    # m >= cs/2: an empty kept window
    assert call(m=-1) == -1
    assert call(clip=2) == -1
    assert call(N=70000) == -2


def test_affine_validation_needs_no_gpu():
    lib = _lib.load()
    a = lib.emd_tile_affine_f32
    assert a(A, A, 1, 16, NULL, NULL) == -1 and b"null" in lib.emd_last_error()
    assert a(NULL, A, 1, 16, B, NULL) == -1
    assert a(A, A, 0, 16, B, NULL) == -1
    assert a(A, A, 1, 0, B, NULL) == -1
