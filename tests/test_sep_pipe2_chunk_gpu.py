"""The whole-chunk instance of the software-pipelined fused separable conv (csrc/sep_pipe2.hip: sep_pipe2_chunk_kernel; two fp32 outputs on
the 256-column tile -- deconv1_a + residual1_d of graph D) against the lockstep kernel it stands in for (csrc/sep_pipe.hip; dev knob
sep_pipe2_chunk = 0), through the same C entry point emd_sep3x3_dual_f32.  Nothing in it changes the order of any sum, so every check is
bit identity:
  * both outputs, chunk counts Cin / 32 in {1, 2, 3, 12} (odd and even, and graph D's 384), one tile and three tiles per workgroup (the peeled
    fill and drain, the tile change), one and two tile rows, W = 32 and 64 (left and right halo columns), B = 1 and 3, both epilogue forms
    (dev knob epi_width), channel tails, on inputs with large positive, large negative and zero pixel rows (relu6 clamps on both sides);
  * the outputs sit between sentinel guard bands and in the middle of wider rows, which must come back untouched (tests/guarded.py);
  * image 1 of a batch of three equals the same image run alone;
  * DenoiserEngine.forward at [2,64,64,1] with the instance on and off."""
import numpy as np
import pytest
import torch

from tests.guarded import assert_written, guarded_act
from tests.test_ops_gpu import dev, rnd, to_act

pytestmark = pytest.mark.gpu

KNOBS = (("sep_pipe2_chunk", -1), ("sep_tpw", 0), ("epi_width", 0))


@pytest.fixture(autouse=True)
def _restore_knobs():
    from emdenoise import _lib

    yield
    for k, v in KNOBS:
        _lib.knob(k, v)


def _inputs(B, H, W, ci, co, co2, seed):
    """x with pixel rows scaled by +-60 and rows of zeros; weights and affines of both signs."""
    x = rnd((B, H, W, ci), seed)
    x[:, 1::4] *= 60.0
    x[:, 2::4, ::3] *= -60.0
    x[:, 3::8] = 0.0
    x[:, :, W // 2] = 0.0
    dw = rnd((9, ci), seed + 1, 0.35)
    pw = rnd((1, ci, co), seed + 2, (2.0 / (ci + co)) ** 0.5)
    w2 = rnd((1, ci, co2), seed + 3, (2.0 / (ci + co2)) ** 0.5)
    s1, t1 = rnd((co,), seed + 4, 0.2) + 1, rnd((co,), seed + 5, 0.5)
    sb, tb = rnd((co2,), seed + 6, 0.2) + 1, rnd((co2,), seed + 7, 0.5)
    return x, dw, pw, w2, s1, t1, sb, tb


def _run(x, dw, pw, w2, s1, t1, sb, tb, chunk, epi, tpw, guard=True):
    """-> (out1, out2) of emd_sep3x3_dual_f32 on the whole-chunk instance (chunk = 1) or the lockstep kernel (0), as device tensors."""
    from emdenoise import _lib, ops

    B, H, W, ci = x.shape
    co, co2 = pw.shape[2], w2.shape[2]
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev())
    xa = to_act(x, ld=ci + 64, c0=32)
    assert ops.sep_dual_supported(xa, co, co2)
    o1, g1 = guarded_act(B, H, W, co, ld=co + 8, c0=4, name="out")
    o2, g2 = guarded_act(B, H, W, co2, ld=co2 + 12, c0=8, name="out2")
    _lib.knob("sep_pipe2_chunk", chunk)
    _lib.knob("epi_width", epi)
    _lib.knob("sep_tpw", tpw)
    ops.sep_dual(xa, d(dw), ops.PackedWeights(pw, False, dev()), ops.PackedWeights(w2, False, dev()), d(s1), d(t1), o1, d(sb), d(tb), o2)
    torch.cuda.synchronize()
    if guard:
        g1()
        g2()
        assert_written(o1.torch(), "out")
        assert_written(o2.torch(), "out2")
    return o1.torch().clone(), o2.torch().clone()


CASES = [
    # B, H, W, Cin, Cout, Cout2, tiles per workgroup
    (1, 8, 32, 32, 128, 128, 0),      # one tile, one chunk: fill, one loop iteration, drain
    (3, 16, 64, 64, 128, 128, 0),     # two tile rows, two tile columns, two chunks, a batch
    (1, 8, 96, 96, 128, 128, 3),      # three tiles in one workgroup, odd chunk count: left-edge, interior and right-edge tile
    (1, 16, 96, 64, 128, 128, 3),     # the same with an even chunk count and two tile rows
    (3, 8, 64, 384, 128, 128, 2),     # graph D's deconv1_a + residual1_d: twelve chunks, two tiles per workgroup
    (1, 8, 32, 96, 72, 128, 0),       # channel tail in the block's output (masked lanes: the conservative waits)
    (1, 8, 64, 32, 128, 40, 2),       # channel tail in the projection
]


@pytest.mark.parametrize("epi", [0, 4], ids=["epi_dword", "epi_16B"])
@pytest.mark.parametrize("B,H,W,ci,co,co2,tpw", CASES)
def test_chunk_instance_equals_lockstep_kernel(B, H, W, ci, co, co2, tpw, epi):
    from emdenoise import _lib

    assert _lib.load().emd_debug_sep_pipe2_chunk_covers(H, W, ci, co, co2) == 1
    args = _inputs(B, H, W, ci, co, co2, 500 + ci + W)
    want1, want2 = _run(*args, chunk=0, epi=epi, tpw=tpw)
    got1, got2 = _run(*args, chunk=1, epi=epi, tpw=tpw)
    assert float(want1.max()) == 6.0 and float(want1.min()) == 0.0 and float(want2.max()) == 6.0 and float(want2.min()) == 0.0
    assert 0.05 < float(((want1 > 0) & (want1 < 6)).float().mean())       # ... and values in between
    assert torch.equal(got1.view(torch.int32), want1.view(torch.int32))
    assert torch.equal(got2.view(torch.int32), want2.view(torch.int32))


@pytest.mark.parametrize("epi", [0, 4], ids=["epi_dword", "epi_16B"])
def test_chunk_instance_image_of_a_batch_equals_the_image_alone(epi):
    B, H, W, ci, co, co2 = 3, 16, 64, 96, 128, 128
    x, *rest = _inputs(B, H, W, ci, co, co2, 700)
    got1, got2 = _run(x, *rest, chunk=1, epi=epi, tpw=0)
    one1, one2 = _run(np.ascontiguousarray(x[1:2]), *rest, chunk=1, epi=epi, tpw=0)
    assert torch.equal(got1[1:2].view(torch.int32), one1.view(torch.int32))
    assert torch.equal(got2[1:2].view(torch.int32), one2.view(torch.int32))


def test_chunk_rule_is_a_function_of_the_shape():
    from emdenoise import _lib

    ok = _lib.load().emd_debug_sep_pipe2_chunk_covers       # (H, W, Cin, Cout, Cout2): no batch argument
    assert ok(256, 256, 384, 128, 128) and ok(32, 32, 384, 128, 128) and ok(8, 32, 32, 68, 4)
    assert not ok(8, 32, 32, 64, 64)        # the 128-column tile: not this instance
    assert not ok(8, 48, 32, 128, 128) and not ok(12, 32, 32, 128, 128) and not ok(8, 32, 48, 128, 128) and not ok(8, 32, 32, 132, 128)


def test_engine_with_and_without_chunk_instance():
    import emdenoise
    from emdenoise import _lib
    from tests.synth_inputs import synthetic_lq

    eng = emdenoise.DenoiserEngine(emdenoise.synthetic_weights(), dev(), "bf16x3")
    x = torch.from_numpy(synthetic_lq(2, 64, 64, seed=31)).to(dev())
    _lib.knob("sep_pipe2_chunk", 0)
    want = eng.forward(x).clone()
    _lib.knob("sep_pipe2_chunk", 1)
    got = eng.forward(x).clone()
    alone = eng.forward(x[1:2].contiguous()).clone()
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.equal(got[1:2], alone)
