"""Where graph D's first strided block takes the generated-residual entry point (emd_sep3x3_fused_s2_genres_f32) and where it keeps
the residual tensor: the library's predicate, the entry point's own shape check and the engine's gate must say the same.  No GPU."""
import ctypes
import types

import pytest

from emdenoise import _lib, denoiser, ops

F0, F1 = 64, 128   # cnn0_last's channels, cnn0_strided's


@pytest.mark.parametrize("S,ok", [(64, True), (512, True), (96, True), (48, False), (80, False), (16, False)])
def test_predicate_and_engine_gate_agree(S, ok, monkeypatch):
    lib = _lib.load()
    assert bool(lib.emd_sep3x3_fused_s2_genres_supported(S, S, F0, F1)) == ok
    assert bool(lib.emd_sep3x3_fused_s2_genres_supported(S, S, F0, F1)) <= bool(lib.emd_sep3x3_fused_supported(S, S, F0, F1, 2, 1))
    x = types.SimpleNamespace(B=1, H=S, W=S, C=F0)
    eng = types.SimpleNamespace(fuse_sep=True, precision=ops.PREC_BF16X3, layers=denoiser.declare_layers("D"))
    gate = denoiser.DenoiserEngine._residual0_generated
    monkeypatch.delenv("EMD_D_SEP_S2", raising=False)
    assert gate(eng, x) == ok
    # every switch that takes cnn0_strided off the one-launch stride-2 form takes it off this one too
    eng.fuse_sep = False
    assert not gate(eng, x)
    eng.fuse_sep, eng.precision = True, ops.PREC_BF16
    assert not gate(eng, x)
    eng.precision = ops.PREC_BF16X3
    monkeypatch.setenv("EMD_D_SEP_S2", "0")
    assert not gate(eng, x)


def test_predicate_limits():
    lib = _lib.load()
    ok = lambda H, W, ci, co: bool(lib.emd_sep3x3_fused_s2_genres_supported(H, W, ci, co))
    assert ok(8, 32, 32, 128) and ok(8, 32, 64, 64) and ok(8, 32, 64, 16)
    assert not ok(8, 32, 64, 256)      # the stride-2 block has a 256-column instance; the generated residual has not
    assert not ok(8, 32, 64, 36)       # Cout / 4 does not divide 64: emd_cin1_f32 would not write that residual either
    assert not ok(8, 32, 48, 128)      # Cin % 32
    assert not ok(12, 32, 64, 128)     # H % 8
    assert not ok(8, 48, 64, 128)      # W % 32


def test_entry_point_refuses_what_the_predicate_refuses():
    lib = _lib.load()
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    args = lambda S, img=p, stride=2: (p, F0, p, p, p, p, p, null, null, img, 1, stride, p, p, 1, p, F1, 1, S, S, F0, F1, 1, null)
    assert lib.emd_sep3x3_fused_s2_genres_f32(*args(48)) != 0 and b"genres" in lib.emd_last_error()
    assert lib.emd_sep3x3_fused_s2_genres_f32(*args(64, null)) != 0 and b"null" in lib.emd_last_error()
    assert lib.emd_sep3x3_fused_s2_genres_f32(*args(64, p, 3)) != 0 and b"stride" in lib.emd_last_error()
