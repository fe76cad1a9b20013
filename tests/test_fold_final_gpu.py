"""emd_sep3x3_fused_fold_f32 + emd_cout1_gather9_f32 (csrc/sep_pipe.hip FOLD, csrc/dw_misc.hip): a stride-1 separable block whose
output feeds only a 3x3 convolution to one channel (deconv0_b -> deconv_final of graph D, machine_learning/denoiser.py:383-387), the
convolution's channel sum formed in the block's epilogue as nine tap planes z [9,B,H,W], its spatial sum in a gather.

Against float64 the pair is held to TOL_X3, the bar of every split-bf16 op.  Against the unfused pair of launches (whose fp32 y the
folded kernel reproduces bit for bit: swapped MFMA operands, same products, same K order) only the order of the 576-term fp32 sum
differs: |got - ref| <= 600 * 2^-24 * |scale| * sum_{t,c} |w_tc * y| + 2^-23 * |ref|, ref the float64 3x3 conv of that y -- the
worst case of 576 fmaf plus the nine-term tap sum plus the final affine, derived, not measured.  Inputs are non-zero up to and
including their borders; z and the output live inside NaN-filled buffers with guard regions on both sides.
"""
import numpy as np
import pytest
import torch

from tests.test_ops_gpu import TOL_X3, dev, out_act, rel_l2, rnd, t64, to_act

pytestmark = pytest.mark.gpu

GUARD = 256   # floats on either side of z and of the output (a multiple of 4: the buffers stay 16-byte aligned)
CO = 64


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev())


def guarded(n):
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=dev())
    return buf, buf[GUARD:GUARD + n]


def conv3x3_to_one(y, w9):
    """float64 3x3 SAME convolution of y [B,H,W,C] with taps w9 [9,C] -> [B,H,W]; tap t reads pixel (h + t // 3 - 1, w + t % 3 - 1)."""
    B, H, W, _ = y.shape
    p = np.pad(np.asarray(y, np.float64), ((0, 0), (1, 1), (1, 1), (0, 0)))
    out = np.zeros((B, H, W))
    for t in range(9):
        out += p[:, t // 3:t // 3 + H, t % 3:t % 3 + W, :] @ np.asarray(w9[t], np.float64)
    return out


def act64(v, act):
    return v if act == 0 else np.clip(v, 0.0, 1.0 if act == 2 else 6.0)


class Pair:
    """Operands of one separable block [B,H,W,ci] -> 64 channels (+ residual) and of the 3x3 conv to one channel behind it."""

    def __init__(self, B, H, W, ci, seed):
        from emdenoise import ops

        self.B, self.H, self.W, self.ci = B, H, W, ci
        self.x_np = rnd((B, H, W, ci), seed, positive=True) + 0.05
        self.dw_np = rnd((3, 3, ci, 1), seed + 1, 0.35)
        self.pw_np = rnd((1, 1, ci, CO), seed + 2, scale=(2.0 / (ci + CO)) ** 0.5)
        self.s1_np, self.t1_np = rnd((CO,), seed + 3, 0.2) + 1, rnd((CO,), seed + 4, 0.5)
        self.s2_np, self.t2_np = rnd((CO,), seed + 5, 0.2) + 1, rnd((CO,), seed + 6, 0.5)
        self.r_np = rnd((B, H, W, CO), seed + 7, positive=True) + 0.05
        self.wf_np = rnd((9, CO), seed + 8, 0.06)
        self.scale, self.shift = 0.8, 0.3
        self.dw, self.pw = up(self.dw_np[..., 0]), ops.PackedWeights(self.pw_np[0], False, dev())
        self.s1, self.t1, self.s2, self.t2, self.wf = up(self.s1_np), up(self.t1_np), up(self.s2_np), up(self.t2_np), up(self.wf_np)

    def x(self, x_np=None):
        return to_act(self.x_np if x_np is None else x_np, ld=self.ci + 32, c0=16)

    def res(self, r_np=None):
        return to_act(self.r_np if r_np is None else r_np, ld=CO + 4, c0=4)

    def affine2(self, on):
        return dict(scale2=self.s2 if on else None, shift2=self.t2 if on else None)

    def fold(self, extra, act, x_np=None, r_np=None, residual=True):
        """The folded pair -> (output [B,H,W], z, the two guarded buffers)."""
        from emdenoise import ops

        n = self.B * self.H * self.W
        zbuf, z = guarded(9 * n)
        obuf, out = guarded(n)
        ops.sep_fused(self.x(x_np), self.dw, self.pw, self.s1, self.t1, None, res=self.res(r_np) if residual else None,
                      fold_final=(self.wf, z), **self.affine2(extra))
        ops.cout1_gather9(z, self.scale, self.shift, out, self.B, self.H, self.W, act=act)
        torch.cuda.synchronize()
        return out.view(self.B, self.H, self.W), z, zbuf, obuf

    def y64(self, extra, residual=True):
        from oracle import tf_ops as T

        y = T.relu6_t(T.conv2d_t(T.depthwise_conv2d_t(t64(self.x_np), t64(self.dw_np)), t64(self.pw_np)) * t64(self.s1_np) + t64(self.t1_np))
        if extra:
            y = T.relu6_t(y * t64(self.s2_np) + t64(self.t2_np))
        y = y.numpy()
        return y + self.r_np.astype(np.float64) if residual else y

    def unfused_y(self, extra, residual=True):
        """Today's launch: the fp32 y the folded kernel never stores."""
        from emdenoise import ops

        y = ops.sep_fused(self.x(), self.dw, self.pw, self.s1, self.t1, out_act(self.B, self.H, self.W, CO, ld=CO + 8, c0=4),
                          res=self.res() if residual else None, **self.affine2(extra))
        torch.cuda.synchronize()
        return y.torch().cpu().numpy()


def check_pair(k, extra, act, residual=True):
    got_t, z, zbuf, obuf = k.fold(extra, act, residual=residual)
    n = k.B * k.H * k.W
    assert not torch.isnan(z).any() and not torch.isnan(got_t).any(), "every plane element and every output pixel is written"
    for buf, m in ((zbuf, 9 * n), (obuf, n)):
        assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + m:]).all(), "nothing outside the buffers is"
    got = got_t.cpu().numpy().astype(np.float64)
    # against float64, the whole pair from the same inputs
    want = act64(k.scale * conv3x3_to_one(k.y64(extra, residual), k.wf_np) + k.shift, act)
    r = rel_l2(got, want)
    print(f"fold pair [{k.B},{k.H},{k.W},{k.ci}] extra={extra} act={act}: rel_l2 vs float64 = {r:.3e}")
    assert r < TOL_X3
    # against the unfused pair: the float64 3x3 conv of the fp32 y today's launch writes
    y = k.unfused_y(extra, residual)
    s = conv3x3_to_one(y, k.wf_np)
    ref = act64(k.scale * s + k.shift, act)
    mag = conv3x3_to_one(np.abs(y), np.abs(k.wf_np))
    bound = 600 * 2.0 ** -24 * abs(k.scale) * mag + 2.0 ** -23 * np.abs(ref)
    err = np.abs(got - ref)
    print(f"    vs the unfused pair: largest |got - ref| / bound = {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    again, z2, _, _ = k.fold(extra, act, residual=residual)
    assert torch.equal(again, got_t) and torch.equal(z2, z), "two runs give equal bits"


# one tile with every pixel at a border; 3 x 3 tiles with all seams; Cin = 32 (one chunk) and 128 (four)
@pytest.mark.parametrize("B,H,W,ci,extra,act", [(2, 8, 16, 64, False, 1), (2, 8, 16, 64, True, 2), (3, 24, 48, 64, False, 2), (3, 24, 48, 64, True, 1),
                                                (2, 8, 16, 32, True, 1), (3, 24, 48, 128, False, 1)])
def test_folded_pair(B, H, W, ci, extra, act):
    check_pair(Pair(B, H, W, ci, 8000 + H + ci), extra, act)


@pytest.mark.parametrize("mode", [0, 1])
def test_both_schedules(mode):
    from emdenoise import _lib

    try:
        _lib.knob("sep_mode", mode)
        check_pair(Pair(3, 24, 48, 64, 8100), mode == 0, 1 + mode)
    finally:
        _lib.knob("sep_mode", -1)


@pytest.mark.parametrize("tpw,extra,act", [(2, False, 1), (4, True, 2)])
def test_several_tiles_per_workgroup(tpw, extra, act):
    from emdenoise import _lib

    try:
        _lib.knob("sep_tpw", tpw)
        check_pair(Pair(1, 16, 64, 64, 8200 + tpw), extra, act)
    finally:
        _lib.knob("sep_tpw", 0)


def test_without_a_residual():
    check_pair(Pair(2, 16, 32, 64, 8300), False, 1, residual=False)


def test_a_changed_border_row_or_column_reaches_one_pixel_further_and_no_more():
    """The depthwise 3x3 and the final 3x3 each reach one pixel: a changed last row of x moves outputs within two rows of it, a changed
    last row of the residual (which enters behind the depthwise stage) within one; the same for the last column."""
    k = Pair(2, 24, 48, 64, 8400)
    base = k.fold(False, 1)[0]
    r = k.r_np.copy(); r[:, -1] += 0.5
    d = (k.fold(False, 1, r_np=r)[0] != base)
    assert d[:, -2:].any() and not d[:, :-2].any()
    r = k.r_np.copy(); r[:, :, -1] += 0.5
    d = (k.fold(False, 1, r_np=r)[0] != base)
    assert d[:, :, -2:].any() and not d[:, :, :-2].any()
    x = k.x_np.copy(); x[:, -1] += 0.5
    d = (k.fold(False, 1, x_np=x)[0] != base)
    assert d[:, -3:].any() and not d[:, :-3].any()
    x = k.x_np.copy(); x[:, :, 0] += 0.5
    d = (k.fold(False, 1, x_np=x)[0] != base)
    assert d[:, :, :3].any() and not d[:, :, 3:].any()


@pytest.mark.parametrize("B,H,W,act", [(2, 8, 16, 0), (3, 24, 48, 1), (1, 16, 64, 2)])
def test_gather_alone(B, H, W, act):
    """Random planes against the float64 sum: nine fp32 additions and one fmaf, |got - ref| <= 10 * 2^-24 * sum|z_t| * |scale| + 2^-23 * |ref|."""
    from emdenoise import ops

    scale, shift = -1.3, 0.7
    z_np = rnd((9, B, H, W), 8500 + H, 1.0)
    zbuf, z = guarded(9 * B * H * W)
    z.copy_(up(z_np).reshape(-1))
    obuf, out = guarded(B * H * W)
    ops.cout1_gather9(z, scale, shift, out, B, H, W, act=act)
    torch.cuda.synchronize()
    p = np.pad(z_np.astype(np.float64), ((0, 0), (0, 0), (1, 1), (1, 1)))
    s = sum(p[t, :, t // 3:t // 3 + H, t % 3:t % 3 + W] for t in range(9))
    mag = sum(np.abs(p[t, :, t // 3:t // 3 + H, t % 3:t % 3 + W]) for t in range(9))
    ref = act64(scale * s + shift, act)
    got = out.view(B, H, W).cpu().numpy().astype(np.float64)
    assert not np.isnan(got).any()
    assert (np.abs(got - ref) <= 10 * 2.0 ** -24 * mag * abs(scale) + 2.0 ** -23 * np.abs(ref)).all()
    assert torch.isnan(obuf[:GUARD]).all() and torch.isnan(obuf[GUARD + B * H * W:]).all()
    assert torch.equal(z, up(z_np).reshape(-1)), "the planes are read, not written"
