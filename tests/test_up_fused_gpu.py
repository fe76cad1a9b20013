"""Graph D's upsampled ASPP output formed inside its two consumers (DenoiserEngine._up_fused; csrc/graph_exec.hip applies the same rule):
  * emd_dw3x3_up_split32_f32 against emd_resize_bilinear_f32 into a concat buffer followed by emd_dw3x3_split32_f32, bit for bit,
    the zero padding of the last channel group included;
  * emd_conv1x1_up_f32 against the float64 host computation of act(s (concat . W) + t), and against today's route (resize ->
    emd_conv1x1_f32) on the same inputs;
  * the engine with the switch on against the switch off, the launches it no longer makes, and the native executor bit for bit.
Outputs sit between guard bands (tests/guarded.py)."""
import numpy as np
import pytest
import torch

from tests import guarded as G
from tests.synth_inputs import synthetic_lq
from tests.test_ops_gpu import TOL_X3, dev, rel_l2, rnd, t64, to_act

pytestmark = pytest.mark.gpu


def guarded_split(B, H, W, Cc, name="split32 output"):
    """A SplitAct whose buffer lies between guard bands -> (SplitAct, check)."""
    from emdenoise import _lib, ops

    s = object.__new__(ops.SplitAct)
    s.B, s.H, s.W, s.C = B, H, W, Cc
    s.ld = _lib.load().emd_split32_ld(Cc)
    view, check = G.guarded(B * H * W * s.ld, torch.float32, dev(), name=name)
    s.buf = view.view(B, H, W, s.ld)
    assert s.buf.data_ptr() % 128 == 0
    return s, check


# ------------------------------------------------------------------------------------------------ entry 1
# (Hi, Wi) -> (Ho, Wo), B, (Cup, Cdirect).  Families: the upsampling factor (4, 4, 2, 1); a width tail (Wo % 16 != 0); 16-row strips
# (Ho >= 64) with an even and a ragged last strip; the channel splits (64 | 32: one generated and one half-filled read workgroup column,
# 64 | 40: a padded split32 group, 256 | 128: graph D's); B = 1 and 2.  The short maps run as 4-row strips, the tall ones as 16-row
# strips: the heights the dispatch rule picks at these sizes.
DW_CASES = [
    (2, 2, 8, 8, 1, 64, 32),
    (2, 2, 8, 8, 2, 256, 128),
    (4, 4, 16, 16, 2, 64, 40),
    (4, 4, 16, 16, 1, 256, 128),
    (4, 4, 8, 8, 1, 256, 128),
    (4, 4, 8, 8, 2, 64, 32),
    (5, 3, 5, 3, 2, 64, 32),
    (5, 3, 5, 3, 1, 64, 40),
    (3, 5, 12, 20, 1, 64, 40),
    (3, 5, 12, 20, 2, 256, 128),
    (16, 16, 64, 64, 2, 64, 32),
    (18, 16, 72, 64, 1, 256, 128),
    (18, 16, 72, 64, 2, 64, 40),
    # heights that are not 4 times the source's (the factors 2 and 1 above are not either): the instance that follows the source row at run time
    (3, 3, 9, 9, 1, 64, 32),
    (4, 4, 6, 10, 2, 64, 40),
    (12, 16, 66, 64, 1, 64, 32),
    # a ratio just below 1
    (15, 15, 16, 16, 1, 64, 32),
    # y0 = floor((float)row * sy) steps by TWO, over the row held for y1, only where y0 + 1 is a power of two and 1 - sy is below the
    # spacing of floats there: at 19657 -> 19663 rows, row 16389 -> 16390 gives y0 = 16383 -> 16385 (numpy float32 finds no such pair
    # below 19663 rows).  One pixel column keeps it small: the branch of the run-time instance that reloads the upper row.
    (19657, 1, 19663, 1, 1, 64, 32),
]


@pytest.mark.parametrize("Hi,Wi,Ho,Wo,B,Cup,Cd", DW_CASES)
def test_dw3x3_up_split32_is_resize_then_depthwise(Hi, Wi, Ho, Wo, B, Cup, Cd):
    from emdenoise import ops

    Cc = Cup + Cd
    assert ops.dw3x3_up_split32_supported(Hi, Wi, Ho, Wo, Cup, Cc)
    lo = to_act(rnd((B, Hi, Wi, Cup), 500 + Ho, 2.0))
    x = to_act(rnd((B, Ho, Wo, Cd), 501 + Wo, 2.0))
    w = torch.from_numpy(rnd((9, Cc), 502, 0.4)).to(dev())
    # today's route: the concat buffer exists
    concat = ops.Act.empty(B, Ho, Wo, Cc, dev())
    ops.resize_bilinear(lo, concat.slice(0, Cup))
    concat.slice(Cup, Cd).torch().copy_(x.torch())
    ref, ref_check = guarded_split(B, Ho, Wo, Cc, "reference")
    ops.dw3x3_split32(concat, w, ref)
    got, got_check = guarded_split(B, Ho, Wo, Cc)
    ops.dw3x3_split32(x, w, got, up=lo)
    torch.cuda.synchronize()
    ref_check()
    got_check()
    G.assert_written(got.buf, "split32 output")
    assert torch.equal(got.buf.view(torch.int32), ref.buf.view(torch.int32))   # the bytes: values and the zero padding
    if Cc % 32:   # [.., group, hi | lo, 32 channels] as bf16 words: the channels past Cc in the last group are zero
        assert not got.buf.view(torch.int16).view(B, Ho, Wo, got.ld // 32, 2, 32)[..., -1, :, Cc % 32:].any()


def test_the_double_step_case_steps_by_two():
    """The premise of DW_CASES' last entry, in the kernels' float32 arithmetic."""
    Hi, _, Ho = DW_CASES[-1][:3]
    y0 = np.floor(np.arange(Ho, dtype=np.float32) * (np.float32(Hi) / np.float32(Ho))).astype(np.int64)
    assert np.diff(y0).max() == 2 and y0.max() <= Hi - 1


def test_dw3x3_up_split32_refuses_what_it_has_no_instance_for():
    from emdenoise import _lib, ops

    assert not ops.dw3x3_up_split32_supported(8, 8, 4, 4, 64, 96)      # downsampling
    assert not ops.dw3x3_up_split32_supported(2, 2, 8, 8, 32, 96)      # Cup not a multiple of 64
    assert not ops.dw3x3_up_split32_supported(2, 2, 8, 8, 64, 64)      # nothing read
    lo, x = to_act(rnd((1, 2, 2, 32), 1)), to_act(rnd((1, 8, 8, 64), 2))
    out, _ = guarded_split(1, 8, 8, 96)
    with pytest.raises(_lib.EmdError, match=r"code -2"):
        ops.dw3x3_split32(x, torch.zeros((9, 96), device=dev()), out, up=lo)


# ------------------------------------------------------------------------------------------------ entry 2
# (Hi, Wi) -> (Ho, Wo), B, K (channels of the full-resolution operand), N; the low-resolution operand has Ka channels
UP_CASES = [
    (2, 2, 8, 8, 2, 32, 64, 64),
    (4, 4, 16, 16, 2, 128, 256, 256),
    (3, 5, 12, 20, 1, 32, 72, 64),     # 240 rows: an M tail; N = 72: an N tail
    # the cases above have fewer than 192 tiles of 128 x 128 and run on the 128 x 64 instance; 12992 rows x 256 columns = 102 x 2 tiles
    # (the last row tile half full): the 128 x 128 instance, graph D's
    (28, 29, 112, 116, 1, 128, 256, 256),
]


@pytest.mark.parametrize("relu6", [True, False])
@pytest.mark.parametrize("Hi,Wi,Ho,Wo,B,K,N,Ka", UP_CASES)
def test_conv1x1_up_against_float64_and_todays_route(Hi, Wi, Ho, Wo, B, K, N, Ka, relu6):
    from emdenoise import ops
    from oracle import tf_ops as T

    a = rnd((B, Hi, Wi, Ka), 600 + N)
    x = rnd((B, Ho, Wo, K), 601 + N)
    w = rnd((1, Ka + K, N), 602 + N, 1.0 / np.sqrt(Ka + K))
    s, t = rnd((N,), 603, 0.3) + 1.5, rnd((N,), 604, 1.0)
    cat64 = np.concatenate([T.resize_bilinear_legacy_t(t64(a), Ho, Wo).numpy(), x.astype(np.float64)], axis=-1)
    ref = (cat64.reshape(-1, Ka + K) @ w[0].astype(np.float64)).reshape(B, Ho, Wo, N) * s + t
    if relu6:
        ref = np.clip(ref, 0.0, 6.0)
    d = lambda v: torch.from_numpy(v).to(dev())
    sd, td = d(s), d(t)
    # the new route: P' at the low resolution, then the K-channel GEMM whose shift is sampled from it
    pp = ops.conv1x1(to_act(a), ops.PackedWeights(w[:, :Ka], False, dev()), sd, td, ops.Act.empty(B, Hi, Wi, N, dev()), act=False)
    out, check = G.guarded_act(B, Ho, Wo, N, ld=N + 8, c0=4, name="conv1x1 up output")
    ops.conv1x1(to_act(x), ops.PackedWeights(w[:, Ka:], False, dev()), sd, None, out, act=relu6, up=pp)
    # today's route: resize into the concat buffer, one GEMM over Ka + K channels
    concat = ops.Act.empty(B, Ho, Wo, Ka + K, dev())
    ops.resize_bilinear(to_act(a), concat.slice(0, Ka))
    concat.slice(Ka, K).torch().copy_(d(x))
    today = ops.conv1x1(concat, ops.PackedWeights(w, False, dev()), sd, td, ops.Act.empty(B, Ho, Wo, N, dev()), act=relu6)
    torch.cuda.synchronize()
    check()
    G.assert_written(out.torch(), "conv1x1 up output")
    e_new, e_today = rel_l2(out.torch().cpu().numpy(), ref), rel_l2(today.torch().cpu().numpy(), ref)
    print(f"conv1x1 up ({Hi},{Wi})->({Ho},{Wo}) B={B} K={K}+{Ka} N={N} relu6={relu6}: rel L2 {e_new:.3e}; resize -> conv1x1 {e_today:.3e}")
    assert e_new <= TOL_X3
    assert e_new <= 1.5 * e_today


def test_conv1x1_up_refuses_a_second_affine_and_a_residual():
    from emdenoise import _lib, ops

    B, Hi, Ho, K, N = 1, 2, 8, 32, 64
    x, pp = to_act(rnd((B, Ho, Ho, K), 1)), to_act(rnd((B, Hi, Hi, N), 2))
    w = ops.PackedWeights(rnd((1, K, N), 3, 0.2), False, dev())
    v = torch.ones(N, device=dev())
    out = ops.Act.empty(B, Ho, Ho, N, dev())
    with pytest.raises(_lib.EmdError, match=r"code -2"):
        ops.conv1x1(x, w, v, None, out, scale2=v, shift2=v, up=pp)
    with pytest.raises(_lib.EmdError, match=r"code -2"):
        ops.conv1x1(x, w, v, None, out, res=ops.Act.empty(B, Ho, Ho, N, dev()), up=pp)


# ------------------------------------------------------------------------------------------------ the engine
@pytest.fixture(scope="module")
def weights():
    import emdenoise

    return emdenoise.synthetic_weights()


def count_resizes(monkeypatch):
    from emdenoise import ops

    calls, orig = [], ops.resize_bilinear

    def spy(*a, **kw):
        calls.append(1)
        return orig(*a, **kw)

    monkeypatch.setattr(ops, "resize_bilinear", spy)
    return calls


@pytest.mark.parametrize("S", [64, 96])
def test_engine_switch_on_against_off(S, weights, monkeypatch):
    import emdenoise

    x = torch.from_numpy(synthetic_lq(2, S, S, seed=700 + S)).to(dev())
    calls = count_resizes(monkeypatch)
    monkeypatch.delenv("EMD_D_UP_FUSED", raising=False)
    eng = emdenoise.DenoiserEngine(weights, dev(), "bf16x3")
    on = eng.forward(x).clone()
    torch.cuda.synchronize()
    assert not calls, "the default route forms the upsampled tensor inside its consumers: no resize launch"
    monkeypatch.setenv("EMD_D_UP_FUSED", "0")
    off = eng.forward(x).clone()
    torch.cuda.synchronize()
    assert len(calls) == 1
    r = rel_l2(on.cpu().numpy(), off.cpu().numpy())
    print(f"graph D [2,{S},{S},1] upsampling inside the consumers vs the resize launch: rel_l2 = {r:.3e}")
    assert r < 3e-4   # the oracle bar of tests/test_d_gpu.py::test_engine_matches_oracle


def test_engine_keeps_the_resize_where_the_predicate_refuses(weights, monkeypatch):
    """The predicate refuses through the precision here, not through a shape: deconv2_a has 384 input channels, and no input size makes
    emd_sep3x3_fused_supported hold for it (its wide form stops at 256) or takes it off the split32 route, so graph D has no refused
    SHAPE by default.  One-pass bf16 is the refusal a user can reach: deconv2_a does not run as depthwise -> split32 GEMM there."""
    import emdenoise

    monkeypatch.delenv("EMD_D_UP_FUSED", raising=False)
    calls = count_resizes(monkeypatch)
    eng = emdenoise.DenoiserEngine(weights, dev(), "bf16")
    assert not eng._up_fused(4, 16)
    eng.forward(torch.from_numpy(synthetic_lq(2, 64, 64, seed=764)).to(dev()))
    torch.cuda.synchronize()
    assert len(calls) == 1


def test_native_executor_equals_the_engine(weights, monkeypatch):
    import emdenoise
    from emdenoise.graph_exec import NativeGraph

    monkeypatch.delenv("EMD_D_UP_FUSED", raising=False)
    x = torch.from_numpy(synthetic_lq(2, 64, 64, seed=765)).to(dev())
    eng = emdenoise.DenoiserEngine(weights, dev(), "bf16x3")
    assert eng._up_fused(4, 16)
    got = eng.forward(x).clone()
    nat = NativeGraph(weights, dev())
    try:
        native = nat.forward(x)
        torch.cuda.synchronize()
        assert torch.equal(native, got)
    finally:
        nat.close()
