"""Every default-reachable instance of the pointwise split32 GEMM (csrc/gemm_split.hip) against a float64 reference, each test first
asserting through emd_debug_split32_plan (tests/test_split_plan.py pins that rule on the CPU) which instance it is about to run.

One input of 2000 rows and one weight [Cin, 3076] (25 column tiles of 128, 49 of 64, an N tail of 4 channels) for Cin = 48 (one K unit
with an all-padding half step) and Cin = 160 (more K steps than the ring has stages); three calls on row prefixes of that input:
M = 2000 -> 256 x 128 tiles, M = 1400 -> 128 x 128, M = 1000 -> 128 x 64, each with a ragged last row tile, with and without a residual
(channels [4, 4 + Cout) of a pitch-(Cout + 8) buffer) and a second affine + relu6, into a channel slice of a guard-banded buffer.

  (a) relative L2 against oracle/tf_ops.py in float64 below 2e-5 (the split-bf16 bar of tests/test_split_gpu.py) for each form;
  (b) the rows the calls share hold equal bits ("all forms give the same bits": same products, same K order);
  (c) a per-element bar, because relative L2 cannot see one wrong row of 2000.  The yardstick is a numpy restatement of the arithmetic,
      not of the kernel: x and w as bf16 round-to-nearest hi plus bf16 lo of the rest, the three products hi.hi + hi.lo + lo.hi, float32
      accumulation, the epilogue in float32.  Its distance from the float64 reference, element by element, over
      d = |s1| sum_k |x_ik| |w_kj| + |t1| (through the second affine: |s2| d + |t2|; with a residual: + |r|) gives a largest ratio per
      case; the kernel's largest ratio must stay below 4 x that (4: the MFMAs sum a K step in another order than numpy does).
  (d) the split32 output at M = 2000 (256 x 128) and M = 1400 (128 x 128): to_split32 of the fp32 output as integers, padding zero.

Yardstick (largest ratio of the numpy restatement over a case; ``python -m tests.test_split_forms_gpu`` prints it, no GPU needed) and
the kernel's largest ratio as a fraction of it, measured on an MI355X:

    Cin  residual  affine2   yardstick   256 x 128   128 x 128   128 x 64    rel L2 (every form)
     48     -         -      6.46e-6       1.00        0.96        0.96          3.99e-6
     48     -        yes     6.26e-6       1.01        0.96        0.96          3.70e-6
     48    yes        -      6.13e-6       0.99        0.99        0.99          2.53e-6
     48    yes       yes     5.86e-6       1.00        1.00        1.00          2.44e-6
    160     -         -      3.00e-6       0.99        0.99        0.99          3.99e-6
    160     -        yes     2.91e-6       0.99        0.99        0.99          3.70e-6
    160    yes        -      2.83e-6       0.99        0.99        0.99          2.53e-6
    160    yes       yes     2.72e-6       0.99        0.99        0.99          2.44e-6
(the forms differ in the rows they cover, not in the bits of a row: assert (b))

What one wrong bf16 mantissa bit in one product would give: 2^-8 |x_ik w_kj| against d ~ sum over Cin such terms, that is 2^-8 / Cin
for a term of average size: 8.1e-5 at Cin = 48, 2.4e-5 at Cin = 160.  The bars (4 x the yardstick) are 2.6e-5 and 1.2e-5: below that, but
by a factor of 3 and 2 only, not comfortably -- the yardstick is the largest of six million ratios, and the dropped lo.lo products and
the rounding of the lo planes (2^-18 each) put it there, not float32 accumulation.  Measured on the CPU restatement: the lowest
mantissa bit of the hi plane of ONE input element flipped moves 36 % (Cin = 48) and 33 % (Cin = 160) of the 3076 outputs of its row past
the bar, and at least one of them in 195 and 189 of 200 random elements; what stays below is a product much smaller than average.  A wrong
bit in a lo plane (2^-16 / Cin) is below the arithmetic's own error and cannot be seen by any bar.

Two forms that tests/test_split_gpu.py runs only against themselves are compared with something else here: the plain 128 x 128 form at
(20, 32, 32, 96, 192) against emd_conv1x1_f32 and float64, and the 256 x 192 form with ONE column tile at (64, 32, 32, 96, 192) against
knob 0, bit for bit.
"""
import functools

import numpy as np
import pytest
import torch

from tests.test_split_plan import N64_L2, N128_L2, N256_L2, OSPLIT, WIDE4W, WIDE8W, big, gemm_plan, small

pytestmark = pytest.mark.gpu

TOL_X3 = 2e-5        # tests/test_split_gpu.py's relative-L2 bar of the split-bf16 path
MARGIN = 4.0
ROWS, COUT = 2000, 3076
# M, (B, H, W), kernel, tile rows, tile columns
FORMS = [(2000, (1, 40, 50), N256_L2, 256, 128), (1400, (1, 35, 40), N128_L2, 128, 128), (1000, (1, 25, 40), N64_L2, 128, 64)]


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def rnd(shape, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


def dev():
    return torch.device("cuda", 0)


def up(a):
    return torch.from_numpy(np.array(a)).to(dev())      # (a copy: the cached arrays are read-only)


def bf16_rne(a):
    """float32 -> the nearest bf16 (ties to even), as float32."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return ((u + (((u >> 16) & 1) + 0x7FFF)) & 0xFFFF0000).astype(np.uint32).view(np.float32)


def hi_lo(a):
    h = bf16_rne(a)
    return h, bf16_rne(a - h)


@functools.lru_cache(maxsize=None)
def base(ci):
    """Inputs, the float64 accumulators (oracle/tf_ops.py), sum_k |x| |w|, and the restated float32 accumulators -- once per Cin."""
    from oracle import tf_ops as T

    x, w = rnd((ROWS, ci), 100 + ci), rnd((ci, COUT), 200 + ci, ci ** -0.5)
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    acc64 = T.conv2d_t(t64(x).view(1, 40, 50, ci), t64(w).view(1, 1, ci, COUT), None).numpy().reshape(ROWS, COUT)
    mag = np.abs(x).astype(np.float64) @ np.abs(w).astype(np.float64)
    (xh, xl), (wh, wl) = hi_lo(x), hi_lo(w)
    acc32 = (xh @ wh + (xh @ wl + xl @ wh)).astype(np.float32)
    vec = {n: rnd((COUT,), 300 + i, s) + o for i, (n, s, o) in enumerate((("s1", 0.3, 1.0), ("t1", 0.5, 0.0), ("s2", 0.2, 1.0), ("t2", 0.3, 0.0)))}
    for a in (x, w, acc64, mag, acc32):
        a.setflags(write=False)
    return dict(x=x, w=w, acc64=acc64, mag=mag, acc32=acc32, r=rnd((ROWS, COUT), 400 + ci), **vec)


def epilogue(b, acc, res, extra, dtype):
    c = lambda n: b[n].astype(dtype)
    u = np.clip(acc.astype(dtype) * c("s1") + c("t1"), 0, 6)
    if extra:
        u = np.clip(u * c("s2") + c("t2"), 0, 6)
    return u + c("r") if res else u


def reference(ci, res, extra):
    """-> float64 reference [ROWS, COUT], the per-element scale d, and the yardstick: the largest |restatement - reference| / d."""
    b = base(ci)
    ref = epilogue(b, b["acc64"], res, extra, np.float64)
    d = np.abs(b["s1"]).astype(np.float64) * b["mag"] + np.abs(b["t1"])
    if extra:
        d = np.abs(b["s2"]).astype(np.float64) * d + np.abs(b["t2"])
    if res:
        d = d + np.abs(b["r"])
    yard = float((np.abs(epilogue(b, b["acc32"], res, extra, np.float32) - ref) / d).max())
    return ref, d, yard


def split_rows(xs, B, H, W):
    """The first B * H * W rows of a split32 tensor as a split32 tensor [B, H, W, C] (the same memory)."""
    from emdenoise import ops

    v = object.__new__(ops.SplitAct)
    v.B, v.H, v.W, v.C, v.ld = B, H, W, xs.C, xs.ld
    v.buf = xs.buf.view(-1, xs.ld)[:B * H * W].view(B, H, W, xs.ld)
    return v


def guarded_split(B, H, W, Cc):
    """A split32 output between two guards, the pattern in every word."""
    from emdenoise import ops
    from tests import guarded

    out = object.__new__(ops.SplitAct)
    out.B, out.H, out.W, out.C, out.ld = B, H, W, Cc, -(-Cc // 32) * 32
    view, check = guarded.guarded(B * H * W * out.ld, torch.float32, dev(), name="split32 output")
    out.buf = view.view(B, H, W, out.ld)
    return out, check


def operands(ci, res, extra):
    from emdenoise import ops
    from tests import guarded

    b = base(ci)
    xs = ops.to_split32(ops.Act(up(b["x"]).view(1, 40, 50, ci)))
    pw = ops.PackedWeights(b["w"][None], False, dev())
    s1, t1 = up(b["s1"]), up(b["t1"])
    kw = dict(scale2=up(b["s2"]) if extra else None, shift2=up(b["t2"]) if extra else None)

    def residual(M, B, H, W):
        return guarded.guarded_act(B, H, W, COUT, ld=COUT + 8, c0=4, fill=b["r"][:M].reshape(B, H, W, COUT), name="residual")[0] if res else None

    return xs, pw, s1, t1, kw, residual


@pytest.mark.parametrize("extra", [False, True], ids=["", "affine2"])
@pytest.mark.parametrize("res", [False, True], ids=["", "res"])
@pytest.mark.parametrize("ci", [48, 160])
def test_three_forms_against_float64_and_each_other(ci, res, extra):
    from emdenoise import _lib, ops
    from tests import guarded

    lib = _lib.load()
    ref, d, yard = reference(ci, res, extra)
    xs, pw, s1, t1, kw, residual = operands(ci, res, extra)
    ys = []
    for M, (B, H, W), kernel, bm, bn in FORMS:
        assert gemm_plan(lib, M, ci, COUT)[:3] == (kernel, bm, bn) and M % bm, M
        out, check = guarded.guarded_act(B, H, W, COUT, ld=COUT + 8, c0=4, name=f"y of {bm} x {bn}")
        ops.conv1x1_split32(split_rows(xs, B, H, W), pw, s1, t1, out, res=residual(M, B, H, W), **kw)
        torch.cuda.synchronize()
        check()
        guarded.assert_written(out.torch(), f"y of {bm} x {bn}")
        ys.append(out.torch().cpu().numpy().reshape(M, COUT))
    l2 = [rel_l2(y, ref[:len(y)]) for y in ys]
    ratio = [float((np.abs(y - ref[:len(y)]) / d[:len(y)]).max()) for y in ys]
    print(f"split32 forms Cin {ci} res {int(res)} affine2 {int(extra)}: yardstick {yard:.3e}; 256x128, 128x128, 128x64: rel L2 "
          + ", ".join(f"{v:.2e}" for v in l2) + "; largest ratio / yardstick " + ", ".join(f"{v / yard:.2f}" for v in ratio))
    bits = [y.view(np.int32) for y in ys]
    for (M, _, _, bm, bn), v, r, y in zip(FORMS, l2, ratio, ys):
        assert v < TOL_X3, (bm, bn, v)
        worst = np.unravel_index(np.argmax(np.abs(y - ref[:M]) / d[:M]), y.shape)
        assert r <= MARGIN * yard, (bm, bn, r / yard, "row, channel", worst)
    assert np.array_equal(bits[0][:1000], bits[2]) and np.array_equal(bits[1][:1000], bits[2]), "rows [0, 1000) of the three forms"
    assert np.array_equal(bits[0][:1400], bits[1]), "rows [0, 1400) of the 256 x 128 and the 128 x 128 form"


@pytest.mark.parametrize("res,extra", [(False, False), (True, True)], ids=["plain", "res-affine2"])
@pytest.mark.parametrize("ci", [48, 160])
def test_split32_output_of_the_two_forms_that_have_one(ci, res, extra):
    from emdenoise import _lib, ops
    from tests import guarded

    lib = _lib.load()
    xs, pw, s1, t1, kw, residual = operands(ci, res, extra)
    for M, (B, H, W), kernel, bm, bn in FORMS[:2]:
        assert gemm_plan(lib, M, ci, COUT, OSPLIT)[:3] == (kernel, bm, bn)
        x = split_rows(xs, B, H, W)
        want = ops.conv1x1_split32(x, pw, s1, t1, ops.Act.empty(B, H, W, COUT, dev()), res=residual(M, B, H, W), **kw)
        got, check = guarded_split(B, H, W, COUT)
        ops.conv1x1_split32(x, pw, s1, t1, got, res=residual(M, B, H, W), **kw)
        torch.cuda.synchronize()
        check()
        guarded.assert_written(got.buf, f"split32 output of {bm} x {bn}")
        assert torch.equal(got.buf.view(torch.int32), ops.to_split32(want).buf.view(torch.int32)), (bm, bn)
        planes = got.buf.view(torch.int16).view(M, got.ld // 32, 2, 32)
        assert got.ld == 3104 and not planes[:, -1, :, COUT % 32:].any(), "padding channels [3076, 3104) of both planes"
    assert gemm_plan(lib, 1000, ci, COUT, OSPLIT)[:3] == (N128_L2, 128, 128)    # there is no 128 x 64 form with a split32 output


def test_plain_128x128_form_against_another_kernel_and_float64():
    """(20, 32, 32, 96, 192): 80 x 2 tiles of 256 rows < 192, 160 x 2 of 128 rows >= 256 -- the only fp32-output shape of
    tests/test_split_gpu.py on this instance, where both sides of its comparison run it."""
    from emdenoise import _lib, ops
    from oracle import tf_ops as T
    from tests import guarded

    B, H, W, ci, co = 20, 32, 32, 96, 192
    assert gemm_plan(_lib.load(), B * H * W, ci, co) == small(160, 2)
    x, w = rnd((B, H, W, ci), 71), rnd((1, 1, ci, co), 72, ci ** -0.5)
    s1, t1 = rnd((co,), 74, 0.3) + 1.0, rnd((co,), 75, 0.5)
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    ref = T.relu6_t(T.conv2d_t(t64(x), t64(w), None) * t64(s1) + t64(t1)).numpy()
    pw = ops.PackedWeights(w[0], False, dev())
    xa = ops.Act(up(x))
    out, check = guarded.guarded_act(B, H, W, co, ld=co + 8, c0=4)
    ops.conv1x1_split32(ops.to_split32(xa), pw, up(s1), up(t1), out)
    old = ops.conv1x1(xa, pw, up(s1), up(t1), ops.Act.empty(B, H, W, co, dev()), precision=ops.PREC_BF16X3)
    torch.cuda.synchronize()
    check()
    guarded.assert_written(out.torch())
    assert float((out.torch() - old.torch()).norm() / old.torch().norm()) < 1e-6      # the register-staged kernel: another summation order
    assert rel_l2(out.torch().cpu().numpy(), ref) < TOL_X3


@pytest.mark.parametrize("form,kernel,threads", [(1, WIDE8W, 512), (2, WIDE4W, 256)])
def test_wide_form_with_one_column_tile(form, kernel, threads):
    """(64, 32, 32, 96, 192): 256 row tiles x one tile of 192 columns, the smallest grid at which split_wide selects its kernel for a
    single column tile -- against knob 0 (256 x 128 tiles, two column tiles), bit for bit."""
    from emdenoise import _lib, ops

    lib = _lib.load()
    B, H, W, ci, co = 64, 32, 32, 96, 192
    x, w = rnd((B, H, W, ci), 81), rnd((1, ci, co), 82, ci ** -0.5)
    pw = ops.PackedWeights(w, False, dev())
    s1, t1 = up(rnd((co,), 84, 0.3) + 1.0), up(rnd((co,), 85, 0.5))
    xs = ops.to_split32(ops.Act(up(x)))
    try:
        _lib.knob("split_wide", 0)
        assert gemm_plan(lib, B * H * W, ci, co) == big(256, 2)
        ref = ops.conv1x1_split32(xs, pw, s1, t1, ops.Act.empty(B, H, W, co, dev()))
        _lib.knob("split_wide", form)
        assert gemm_plan(lib, B * H * W, ci, co) == (kernel, 256, 192, threads, 256, 1, form, 0)
        wide = torch.full((B, H, W, co + 8), float("nan"), dtype=torch.float32, device=dev())
        got = ops.conv1x1_split32(xs, pw, s1, t1, ops.Act(wide, co, 4))
        torch.cuda.synchronize()
    finally:
        _lib.knob("split_wide", 0)
    assert not torch.isnan(got.torch()).any() and torch.equal(got.torch(), ref.torch())
    assert torch.isnan(wide[..., :4]).all() and torch.isnan(wide[..., 4 + co:]).all()


if __name__ == "__main__":   # the yardsticks, on the CPU
    for ci_ in (48, 160):
        for res_ in (False, True):
            for extra_ in (False, True):
                print(f"Cin {ci_} res {int(res_)} affine2 {int(extra_)}: yardstick {reference(ci_, res_, extra_)[2]:.3e}")
