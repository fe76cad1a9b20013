"""emd_sep3x3_fused_gen9_f32: the generated-input separable block (graph D's cnn0 -> cnn0_last) that takes the 1-channel image and the
nine depthwise taps, forms d per tile inside the kernel and builds the Cin-channel input in registers.

  * bit for bit against the written-out route: emd_cin1_f32 (taps w9, unit scale, no activation) into a 4-channel scratch, then
    emd_sep3x3_fused_gen_f32 from it;
  * guard bands: ld > Cout, NaN canaries in the pad channels and in whole image slots before and after the tensor;
  * against a float64 numpy restatement, held to the split-bf16 bar tests/test_sep_pipe_gpu.py applies to the same block (TOL_X3);
  * DenoiserEngine.forward with the route on and off (EMD_D_GEN9), and image b of a batch against the image run alone;
  * the rule and the argument checks.

The inputs make a wrong border visible: the image has no zeros, t has entries of both signs (a padding pixel generated as relu6(t[c])
instead of 0 changes the output) and a is scaled so that both clamps of relu6 act on a good share of the generated values."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from tests.test_ops_gpu import TOL_X3, dev, out_act, rel_l2, rnd

pytestmark = pytest.mark.gpu


def d_(v):
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev())


def make_inputs(B, H, W, ci, co, seed):
    img = rnd((B, H, W, 1), seed)
    img = (np.sign(img) + (img == 0)) * (np.abs(img) + 0.1)           # no zeros
    p = {"img": img.astype(np.float32), "w9": rnd((9,), seed + 1, 0.4), "a": rnd((ci,), seed + 2, 20.0), "t": rnd((ci,), seed + 3, 1.5),
         "dw": rnd((3, 3, ci), seed + 4, 0.35), "pw": rnd((1, ci, co), seed + 5, scale=(2.0 / (ci + co)) ** 0.5),
         "s1": rnd((co,), seed + 6, 0.2) + 1, "t1": rnd((co,), seed + 7, 0.5), "s2": rnd((co,), seed + 8, 0.2) + 1,
         "t2": rnd((co,), seed + 9, 0.5), "res": rnd((B, H, W, co), seed + 10)}
    assert (p["t"] > 0).any() and (p["t"] < 0).any()
    return p


def conv3x3_same(x, w):
    """x [B,H,W,C] float64, w [3,3,C] (or [3,3,1]): depthwise 3x3, zero padding."""
    B, H, W, _ = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    return sum(w[i, j] * xp[:, i:i + H, j:j + W, :] for i in range(3) for j in range(3))


def restate64(p, extra, res):
    f = lambda k: p[k].astype(np.float64)
    d = conv3x3_same(f("img"), f("w9").reshape(3, 3, 1))
    u = d * f("a") + f("t")
    g = np.clip(u, 0.0, 6.0)
    y = conv3x3_same(g, f("dw")) @ f("pw")[0]
    y = np.clip(y * f("s1") + f("t1"), 0.0, 6.0)
    if extra:
        y = np.clip(y * f("s2") + f("t2"), 0.0, 6.0)
    return (y + f("res") if res else y), u


def run_gen9(p, pw, out, extra, res):
    from emdenoise import ops

    B, H, W, _ = p["img"].shape
    return ops.sep_fused_gen(ops.Act(d_(p["img"])), d_(p["a"]), d_(p["t"]), d_(p["dw"]), pw, d_(p["s1"]), d_(p["t1"]), out,
                             scale2=d_(p["s2"]) if extra else None, shift2=d_(p["t2"]) if extra else None,
                             res=ops.Act(d_(p["res"])) if res else None, gen_w9=d_(p["w9"]))


def run_written_out(p, pw, out, extra, res):
    from emdenoise import ops

    B, H, W, _ = p["img"].shape
    d4 = ops.cin1(d_(p["img"]), d_(p["w9"]), d_(np.array([1, 0, 0, 0])), d_(np.zeros(4)), out_act(B, H, W, 4, ld=4, c0=0), act=False)
    return ops.sep_fused_gen(d4, d_(p["a"]), d_(p["t"]), d_(p["dw"]), pw, d_(p["s1"]), d_(p["t1"]), out,
                             scale2=d_(p["s2"]) if extra else None, shift2=d_(p["t2"]) if extra else None,
                             res=ops.Act(d_(p["res"])) if res else None)


@pytest.mark.parametrize("B,H,W,tpw", [
    (1, 8, 16, 0),      # one tile: all four image borders in it
    (2, 16, 32, 0),
    (1, 24, 48, 3),     # left-edge, interior and right-edge tile in one workgroup; an interior tile row
    (3, 8, 128, 8),     # eight tiles walked by one workgroup
    (1, 40, 16, 0),
])
def test_gen9_equals_the_written_out_route_bit_for_bit(B, H, W, tpw):
    from emdenoise import _lib, ops

    for ci, co, extra, res in itertools.product((32, 64), (64, 32), (False, True), (False, True)):
        p = make_inputs(B, H, W, ci, co, 300 + ci + co)
        _, u = restate64(p, extra, res)
        assert (u < 0).mean() > 0.1 and (u > 6).mean() > 0.1, "both clamps of relu6 must act on a good share of the generated input"
        pw = ops.PackedWeights(p["pw"], False, dev())
        want = run_written_out(p, pw, out_act(B, H, W, co, ld=co, c0=0), extra, res)
        try:
            _lib.knob("sep_tpw", tpw)
            got = run_gen9(p, pw, out_act(B, H, W, co, ld=co, c0=0), extra, res)
        finally:
            _lib.knob("sep_tpw", 0)
        torch.cuda.synchronize()
        assert not torch.isnan(got.torch()).any()
        assert torch.equal(got.torch(), want.torch()), (ci, co, extra, res)


@pytest.mark.parametrize("B,H,W,ci,co,res", [(2, 16, 32, 64, 64, False), (1, 8, 48, 32, 24, True)])
def test_gen9_writes_nothing_outside_its_output(B, H, W, ci, co, res):
    from emdenoise import ops

    p = make_inputs(B, H, W, ci, co, 400)
    pw = ops.PackedWeights(p["pw"], False, dev())
    ld, c0 = co + 8, 4
    big = torch.full((B + 2, H, W, ld), float("nan"), dtype=torch.float32, device=dev())   # one image slot of canaries on either side
    out = ops.Act(big[1:B + 1], co, c0)
    got = run_gen9(p, pw, out, True, res)
    want = run_written_out(p, pw, out_act(B, H, W, co, ld=co, c0=0), True, res)
    torch.cuda.synchronize()
    assert torch.equal(got.torch(), want.torch())
    full = big.cpu().numpy()
    assert np.isnan(full[0]).all() and np.isnan(full[B + 1]).all()
    assert np.isnan(full[1:B + 1, :, :, :c0]).all() and np.isnan(full[1:B + 1, :, :, c0 + co:]).all()


def test_gen9_against_a_float64_restatement():
    """One ragged-border case (three tile columns, three tile rows, every border kind), second affine and residual."""
    from emdenoise import ops

    B, H, W, ci, co = 2, 24, 48, 64, 64
    p = make_inputs(B, H, W, ci, co, 500)
    want, _ = restate64(p, True, True)
    got = run_gen9(p, ops.PackedWeights(p["pw"], False, dev()), out_act(B, H, W, co, ld=co, c0=0), True, True)
    torch.cuda.synchronize()
    err = rel_l2(got.torch().cpu().numpy(), want)
    print("gen9 vs float64 restatement: rel l2 =", err)
    assert err < TOL_X3


@pytest.mark.parametrize("S", [32, 64])
def test_engine_with_and_without_gen9(S, monkeypatch):
    import emdenoise
    from emdenoise import ops
    from tests.synth_inputs import synthetic_lq

    calls = []
    real = ops.sep_fused_gen

    def spy(*a, **kw):
        calls.append(kw.get("gen_w9") is not None)
        return real(*a, **kw)

    monkeypatch.setattr(ops, "sep_fused_gen", spy)
    eng = emdenoise.DenoiserEngine(emdenoise.synthetic_weights(), dev(), "bf16x3")
    x = torch.from_numpy(synthetic_lq(2, S, S, seed=31)).to(dev())
    monkeypatch.setenv("EMD_D_GEN9", "0")
    want = eng.forward(x).clone()
    monkeypatch.setenv("EMD_D_GEN9", "1")
    got = eng.forward(x).clone()
    alone = eng.forward(x[1:2].contiguous()).clone()
    torch.cuda.synchronize()
    assert calls == [False, True, True]
    assert torch.equal(got, want)
    assert torch.equal(got[1:2], alone)


def test_gen9_rule_and_argument_checks():
    from emdenoise import _lib, ops

    lib = _lib.load()
    ok = lib.emd_sep3x3_fused_gen9_supported          # (H, W, Cin, Cout): no batch argument, a function of the layer's shape alone
    assert ok(512, 512, 64, 64) and ok(8, 16, 32, 4) and ok(40, 16, 64, 32)
    assert not ok(12, 16, 64, 64) and not ok(8, 24, 64, 64) and not ok(8, 16, 96, 64) and not ok(8, 16, 64, 128) and not ok(8, 16, 64, 30)
    H, W = 8, 16
    img = torch.ones(1, H, W, 1, device=dev())
    a = torch.zeros(64, device=dev())
    w9 = torch.zeros(12, device=dev())
    pw = ops.PackedWeights(rnd((1, 64, 128), 150), False, dev())
    dw, s1 = torch.zeros(9 * 64, device=dev()), torch.ones(128, device=dev())
    y = out_act(1, 16, W, 128, ld=128, c0=0)
    p = lambda t: C.c_void_p(t.data_ptr())
    args = lambda B=1, H=H, co=64, reflect=0, gen_act=1: (p(img), p(w9), p(a), p(a), gen_act, p(dw), p(pw.hi), p(pw.lo), p(s1), p(s1), None,
                                                        None, None, 0, y.ptr, 128, B, H, W, 64, co, 1, ops.PREC_BF16X3, reflect, None)
    f = lib.emd_sep3x3_fused_gen9_f32
    assert f(*args(B=0)) == 0                          # empty batch: a no-op
    for bad in (dict(reflect=1), dict(co=128), dict(H=12), dict(gen_act=4)):
        assert f(*args(**bad)) == -2, bad              # EMD_E_UNSUPPORTED
        assert b"gen9" in lib.emd_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(y.buf).all()                    # nothing was launched
    assert f(*args()) == 0                             # (the same arguments without the fault do run)
    torch.cuda.synchronize()
    assert not torch.isnan(y.buf[:, :H, :, :64]).any() and torch.isnan(y.buf[:, H:]).all() and torch.isnan(y.buf[..., 64:]).all()
