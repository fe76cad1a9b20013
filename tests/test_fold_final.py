"""Where graph D's deconv0_b runs with deconv_final's channel sum folded into its epilogue (emd_sep3x3_fused_fold_f32 followed by
emd_cout1_gather9_f32) and where the pair of launches stays: the library's predicate, the entry points' own checks and the engine's
gate must say the same.  No GPU.

The predicate's rule is stride 1, split-bf16, H % 8 == 0, W % 16 == 0 (the 4-wave kernel's 8 x 16 pixel tiles), Cin % 32 == 0,
Cout == 64; it does not look at the batch size.  S = 48 and S = 80 are multiples of 16 and are covered (the stride-2 generated-residual
instance of tests/test_enc0_genres.py, with its 32-pixel tiles, refuses them); S = 40, 72 and 20 are the sizes this one refuses.
"""
import ctypes
import types

import pytest

from emdenoise import _lib, denoiser, ops

F0 = 64   # deconv0_b's channels, in and out


@pytest.mark.parametrize("S,ok", [(64, True), (512, True), (96, True), (48, True), (80, True), (40, False), (72, False), (20, False)])
def test_predicate_and_engine_gate_agree(S, ok, monkeypatch):
    lib = _lib.load()
    assert bool(lib.emd_sep3x3_fused_fold_supported(S, S, F0, F0)) == ok
    assert bool(lib.emd_sep3x3_fused_fold_supported(S, S, F0, F0)) <= bool(lib.emd_sep3x3_fused_supported(S, S, F0, F0, 1, 1))
    eng = types.SimpleNamespace(fuse_sep=True, precision=ops.PREC_BF16X3, layers=denoiser.declare_layers("D"))
    gate = denoiser.DenoiserEngine._fold_final
    monkeypatch.delenv("EMD_D_FOLD_FINAL", raising=False)
    for B in (1, 2, 3, 32):   # the rule does not depend on the batch size
        assert gate(eng, types.SimpleNamespace(B=B, H=S, W=S, C=F0)) == ok
    x = types.SimpleNamespace(B=1, H=S, W=S, C=F0)
    # every switch that takes deconv0_b off the one-launch split-bf16 form takes it off this one too
    eng.fuse_sep = False
    assert not gate(eng, x)
    eng.fuse_sep, eng.precision = True, ops.PREC_BF16
    assert not gate(eng, x)
    eng.precision = ops.PREC_BF16X3
    monkeypatch.setenv("EMD_D_FOLD_FINAL", "0")
    assert not gate(eng, x)
    monkeypatch.setenv("EMD_D_FOLD_FINAL", "1")
    assert gate(eng, x) == ok


def test_predicate_limits():
    lib = _lib.load()
    ok = lambda H, W, ci, co: bool(lib.emd_sep3x3_fused_fold_supported(H, W, ci, co))
    assert ok(8, 16, 32, 64) and ok(8, 16, 64, 64) and ok(24, 48, 128, 64) and ok(512, 512, 64, 64)
    assert not ok(8, 16, 64, 128)     # the FOLD instance has 64 columns
    assert not ok(8, 16, 64, 32)
    assert not ok(8, 16, 48, 64)      # Cin % 32
    assert not ok(8, 16, 0, 64)
    assert not ok(12, 16, 64, 64)     # H % 8
    assert not ok(8, 24, 64, 64)      # W % 16
    assert not ok(0, 16, 64, 64)


def test_knobs_that_take_the_kernel_away_take_the_predicate_away():
    lib = _lib.load()
    try:
        _lib.knob("sep_pipe", 0)      # the FOLD instance lives in the LDS-DMA pipelined kernel only
        assert not lib.emd_sep3x3_fused_fold_supported(64, 64, F0, F0)
        _lib.knob("sep_pipe", 1)
        _lib.knob("sep_nw", 8)        # ... in its 4-wave form
        assert not lib.emd_sep3x3_fused_fold_supported(64, 64, F0, F0)
    finally:
        _lib.knob("sep_pipe", 1)
        _lib.knob("sep_nw", 0)
    assert lib.emd_sep3x3_fused_fold_supported(64, 64, F0, F0)


def test_entry_points_refuse_what_the_predicate_refuses():
    lib = _lib.load()
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    # x ldx dw whi wlo scale1 shift1 scale2 shift2 res ldres wfin z B H W Cin Cout act stream
    args = lambda H, W, ci=F0, co=F0, wfin=p: (p, ci, p, p, p, p, p, null, null, p, co, wfin, p, 1, H, W, ci, co, 1, null)
    for bad in (args(40, 40), args(12, 16), args(8, 24), args(64, 64, 48), args(64, 64, 64, 128)):
        assert lib.emd_sep3x3_fused_fold_f32(*bad) != 0 and b"fold" in lib.emd_last_error()
    assert lib.emd_sep3x3_fused_fold_f32(*args(64, 64, wfin=null)) != 0 and b"null" in lib.emd_last_error()
    # z scale shift y B H W act stream
    g = lambda H, W, z=p, act=1: (z, 1.0, 0.0, p, 1, H, W, act, null)
    for bad in (g(40, 40), g(12, 16), g(8, 24)):
        assert lib.emd_cout1_gather9_f32(*bad) != 0 and b"gather9" in lib.emd_last_error()
    assert lib.emd_cout1_gather9_f32(*g(64, 64, null)) != 0 and b"null" in lib.emd_last_error()
    assert lib.emd_cout1_gather9_f32(*g(64, 64, p, 3)) != 0 and b"act" in lib.emd_last_error()
