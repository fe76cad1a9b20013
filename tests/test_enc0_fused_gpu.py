"""emd_sep3x3_fused_s2_genres_f32 (csrc/sep_pipe.hip, RGEN): graph D's cnn0_strided with residual0 = relu6(x[2y, 2x] * a + shift)
(machine_learning/denoiser.py:252) evaluated in the epilogue.  It promises the bits of

    res = emd_cin1_f32(img, NULL, a, shift, stride)   then   emd_sep3x3_fused_s2_f32(..., res)

so every comparison is torch.equal.  Images are non-zero up to and including their borders; outputs are channel slices of NaN-filled
buffers, so an unwritten pixel and a write outside the slice both show.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_ops_gpu import dev, out_act, rnd, to_act

pytestmark = pytest.mark.gpu


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev())


class Block:
    """Operands of one stride-2 separable block [B,H,W,ci] -> [B,H/2,W/2,co] and of its rank-1 residual."""

    def __init__(self, B, H, W, ci, co, seed):
        from emdenoise import ops

        self.dims = (B, H // 2, W // 2, co)
        self.x = to_act(rnd((B, H, W, ci), seed, positive=True), ld=ci + 32, c0=16)
        self.dw = up(rnd((3, 3, ci, 1), seed + 1, 0.35)[..., 0])
        self.pw = ops.PackedWeights(rnd((1, 1, ci, co), seed + 2, scale=(2.0 / (ci + co)) ** 0.5)[0], False, dev())
        self.s1, self.t1 = up(rnd((co,), seed + 3, 0.2) + 1), up(rnd((co,), seed + 4, 0.5))
        self.s2, self.t2 = up(rnd((co,), seed + 5, 0.2) + 1), up(rnd((co,), seed + 6, 0.5))
        self.a, self.t = up(rnd((co,), seed + 7, 1.5)), up(rnd((co,), seed + 8, 1.0))   # both signs: the clamp bites at 0 and at 6

    def out(self):
        B, Ho, Wo, co = self.dims
        return out_act(B, Ho, Wo, co, ld=co + 8, c0=4)

    def affine2(self, on):
        return dict(scale2=self.s2 if on else None, shift2=self.t2 if on else None)


# B, H, W of the 1-channel image: one tile row per image; ragged against nothing the kernel tiles by but against 8 x 32 (3 x 5 tiles of
# 4 x 16 outputs twice over); the benchmark's crop
@pytest.mark.parametrize("B,H,W", [(2, 64, 64), (3, 96, 160), (1, 512, 512)])
@pytest.mark.parametrize("ci,co,extra,res_act", [(64, 128, False, True), (64, 128, True, True), (32, 64, False, False), (96, 64, True, True)])
def test_generated_residual_is_cin1_plus_residual_tensor(B, H, W, ci, co, extra, res_act):
    from emdenoise import _lib, ops

    k = Block(B, H, W, ci, co, 7000 + ci + co)
    img = up(rnd((B, H, W, 1), 6999, positive=True) + 0.05)
    assert ops.sep_fused_s2_genres_supported(k.x, co)
    got = ops.sep_fused(k.x, k.dw, k.pw, k.s1, k.t1, k.out(), stride=2, gen_res=(img, k.a, k.t, 2, res_act), **k.affine2(extra))
    torch.cuda.synchronize()
    assert not torch.isnan(got.torch()).any(), "every output pixel is written"
    assert torch.isnan(got.buf[..., :4]).all() and torch.isnan(got.buf[..., 4 + co:]).all(), "nothing outside the channel slice is"
    _, Ho, Wo, _ = k.dims
    try:
        for mode in (1, 0):   # the reference on either issue schedule
            _lib.knob("sep_mode", mode)
            res = ops.cin1(img, None, k.a, k.t, out_act(B, Ho, Wo, co), stride=2, act=res_act)
            want = ops.sep_fused(k.x, k.dw, k.pw, k.s1, k.t1, k.out(), res=res, stride=2, **k.affine2(extra))
            torch.cuda.synchronize()
            assert torch.equal(got.torch(), want.torch())
    finally:
        _lib.knob("sep_mode", -1)
    bare = ops.sep_fused(k.x, k.dw, k.pw, k.s1, k.t1, k.out(), stride=2, **k.affine2(extra))
    torch.cuda.synchronize()
    assert not torch.equal(got.torch(), bare.torch()), "the residual takes part in the result"


def test_pitch_4_image_sampled_at_every_pixel():
    """The C entry point's other form: the image as channel 0 of a 4-channel tensor (pitch 4), half-size and sampled with stride 1."""
    from emdenoise import _lib, ops
    from emdenoise.ops import _p

    B, H, W, ci, co = 2, 32, 64, 64, 128
    k = Block(B, H, W, ci, co, 7500)
    img = rnd((B, H // 2, W // 2, 1), 7499, positive=True) + 0.05
    wide = torch.full((B, H // 2, W // 2, 4), float("nan"), dtype=torch.float32, device=dev())
    wide[..., 0] = up(img[..., 0])
    got = k.out()
    rc = _lib.load().emd_sep3x3_fused_s2_genres_f32(k.x.ptr, k.x.ld, _p(k.dw), _p(k.pw.hi), _p(k.pw.lo), _p(k.s1), _p(k.t1), _p(None), _p(None),
                                                    _p(wide), 4, 1, _p(k.a), _p(k.t), 1, got.ptr, got.ld, B, H, W, ci, co, 1, ctypes.c_void_p(0))
    _lib.check(rc, "emd_sep3x3_fused_s2_genres_f32")
    res = ops.cin1(up(img), None, k.a, k.t, out_act(B, H // 2, W // 2, co), stride=1)
    want = ops.sep_fused(k.x, k.dw, k.pw, k.s1, k.t1, k.out(), res=res, stride=2)
    torch.cuda.synchronize()
    assert torch.equal(got.torch(), want.torch())


@pytest.mark.parametrize("B,S", [(2, 64), (1, 96)])
def test_engine_with_and_without_the_residual_tensor(B, S):
    """DenoiserEngine.forward on its default route (residual0 generated) against an engine that writes residual0 and reads it back."""
    import emdenoise
    from tests.synth_inputs import synthetic_lq

    routes = []

    class Spy(emdenoise.DenoiserEngine):
        def _residual0_generated(self, t):
            routes.append(super()._residual0_generated(t))
            return routes[-1]

    class Tensor(emdenoise.DenoiserEngine):
        def _residual0_generated(self, t):
            return False

    w = emdenoise.synthetic_weights()
    x = torch.from_numpy(synthetic_lq(B, S, S, seed=21)).to(dev())
    got = Spy(w, dev(), "bf16x3").forward(x).clone()
    want = Tensor(w, dev(), "bf16x3").forward(x).clone()
    torch.cuda.synchronize()
    assert routes and all(routes), "S % 32 == 0: the default route generates the residual"
    assert torch.equal(got, want)
