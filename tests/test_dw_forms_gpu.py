"""Every strip height of the rolling stride-1 depthwise kernel (csrc/dw_misc.hip, dw3x3_s1_roll<TH, SPLIT, REFLECT, PRE>) that the launch
rule selects, and the ones only the knob dw_th reaches, against a float64 reference -- each test first asserting through
emd_debug_dw_plan (tests/test_split_plan.py pins that rule on the CPU) which instance it is about to run.

Reference: oracle/tf_ops.py's depthwise conv in float64 (REFLECT: oracle/gan_graph.py's reflect pad + VALID depthwise, the restatement
of tests/test_gan_train_gpu.py); for the pre forms on relu(x * scale + shift) formed in float64.

The per-element bar is derived, not measured.  An output is nine fused multiply-adds (three per input row, each chain starting from
zero) and two additions of row sums: eleven roundings, each at most 2^-24 of a partial sum whose magnitude is at most
S = sum |w| |x| over the window.  To first order |y - ref| <= 11 * 2^-24 * S; the bar is 16 * 2^-24 * S.  The pre forms round the affine
once more per input (one fma: 2^-24 (|x s| + |t|) at most, and relu does not enlarge it): + 2 * 2^-24 * sum |w| (|x s| + |t|), with
S taken over relu(x s + t).  The file's relative-L2 bar 2e-6 (tests/test_ops_gpu.py's for the fp32 depthwise) is kept as well.
A split32 output equals emd_to_split32_f32 of the plain output as integers, padding channels zero.
"""
import functools

import numpy as np
import pytest
import torch

from tests.test_split_plan import PLAIN, PRE, PRE_SPLIT, REFLECT, REFLECT_SPLIT, SPLIT, dw_plan

pytestmark = pytest.mark.gpu

TOL_L2 = 2e-6
EPS = 2.0 ** -24
KINDS = [PLAIN, SPLIT, PRE, PRE_SPLIT]
KIND_IDS = ["plain", "split32", "pre", "pre-split32"]
# shape -> strip height the rule selects, and why
NATURAL = [
    ((16, 9, 17, 1000), 8),      # 1024 workgroups of 8 rows; a split32 padding quad block; W = 17, H = 9 ragged
    ((16, 17, 17, 1024), 16),    # 16 <= H < 64 with 1024 workgroups of 16 rows; the last strip is one row
    ((1, 65, 17, 40), 16),       # H >= 64; the last strip is one row
    ((1, 129, 128, 8), 16),      # H * W > 128 * 128: launch-order tiles (dw_xcd off)
    ((1, 3, 3, 384), 4),         # a grid of 6 workgroups, no multiple of 8, in XCD-contiguous order
]


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def rnd(shape, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


def dev():
    return torch.device("cuda", 0)


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def t64(a):
    return torch.from_numpy(np.asarray(a, np.float64))


@functools.lru_cache(maxsize=None)
def case(shape, reflect=False):
    """Inputs, the float64 references (plain and pre) and their per-element bars, once per shape."""
    from oracle import gan_graph as GG
    from oracle import tf_ops as T

    B, H, W, Cc = shape
    x, w = rnd(shape, 21), rnd((3, 3, Cc, 1), 22, 0.3)
    sc, sh = rnd((Cc,), 23, 0.5) + 1.0, rnd((Cc,), 24, 0.5)
    conv = (lambda a, k: GG.depthwise_valid_t(GG.reflect_pad_t(a, 1), k, 1)) if reflect else T.depthwise_conv2d_t
    x64, w64 = t64(x), t64(w)
    ref = conv(x64, w64).numpy()
    bar = 16 * EPS * conv(x64.abs(), w64.abs()).numpy()
    out = dict(x=x, w9=w[..., 0].reshape(9, Cc), sc=sc, sh=sh, ref=ref, bar=bar)
    if not reflect:
        a64 = torch.relu(x64 * t64(sc) + t64(sh))
        out["ref_pre"] = conv(a64, w64).numpy()
        out["bar_pre"] = (16 * EPS * conv(a64, w64.abs()) + 2 * EPS * conv((x64 * t64(sc)).abs() + t64(sh).abs(), w64.abs())).numpy()
    return out


def guarded_split(B, H, W, Cc):
    from emdenoise import ops
    from tests import guarded

    out = object.__new__(ops.SplitAct)
    out.B, out.H, out.W, out.C, out.ld = B, H, W, Cc, -(-Cc // 32) * 32
    view, check = guarded.guarded(B * H * W * out.ld, torch.float32, dev(), name="split32 output")
    out.buf = view.view(B, H, W, out.ld)
    return out, check


def run(kind, c, shape):
    """One launch of `kind` into guard-banded memory -> the output's words as int32 on the host: [B,H,W,C] (fp32), [B,H,W,ld] (split32)."""
    from emdenoise import ops
    from tests import guarded

    B, H, W, Cc = shape
    xa, wd = ops.Act(up(c["x"])), up(c["w9"])
    pre = (up(c["sc"]), up(c["sh"])) if kind in (PRE, PRE_SPLIT) else None
    if kind in (SPLIT, PRE_SPLIT, REFLECT_SPLIT):
        out, check = guarded_split(*shape)
        if kind == REFLECT_SPLIT:
            ops.dw3x3_reflect_split32(xa, wd, out)
        else:
            ops.dw3x3_split32(xa, wd, out, pre=pre)
        words = out.buf
    else:
        out, check = guarded.guarded_act(B, H, W, Cc, ld=Cc + 8, c0=4)
        if kind == REFLECT:
            ops.dw3x3_reflect(xa, wd, out)
        else:
            ops.dw3x3(xa, wd, out, pre=pre)
        words = out.torch()
    torch.cuda.synchronize()
    check()
    guarded.assert_written(words)
    return words.contiguous().view(torch.int32).cpu().numpy()


def check_fp32(words, ref, bar, what):
    y = words.view(np.float32)
    err = np.abs(y - ref)
    l2, worst = rel_l2(y, ref), float((err / bar).max())
    print(f"{what}: rel L2 {l2:.2e}, largest |y - ref| / bar {worst:.3f}")
    assert l2 < TOL_L2, (what, l2)
    assert worst <= 1.0, (what, worst, "at [b, y, x, c]", np.unravel_index(np.argmax(err / bar), y.shape))


def check_split(words, plain_words, Cc, what):
    """== emd_to_split32_f32 of the plain output, as integers; the padding channels of both planes are zero."""
    from emdenoise import ops

    want = ops.to_split32(ops.Act(torch.from_numpy(plain_words.view(np.float32)).to(dev())))
    torch.cuda.synchronize()
    assert np.array_equal(words, want.buf.view(torch.int32).cpu().numpy()), what
    planes = words.view(np.int16).reshape(-1, words.shape[-1] // 32, 2, 32)
    if Cc % 32:
        assert not planes[:, -1, :, Cc % 32:].any(), what


def check_kind(kind, shape, c, name):
    pre = kind in (PRE, PRE_SPLIT)
    plain = run(PRE if pre else PLAIN, c, shape)
    check_fp32(plain, c["ref_pre" if pre else "ref"], c["bar_pre" if pre else "bar"], f"{name} {shape}")
    if kind in (SPLIT, PRE_SPLIT):
        check_split(run(kind, c, shape), plain, shape[3], f"{name} {shape}")


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("shape,th", NATURAL, ids=[f"th{t}-{'x'.join(map(str, s))}" for s, t in NATURAL])
def test_strip_height_the_rule_selects(shape, th, kind):
    from emdenoise import _lib

    B, H, W, Cc = shape
    p = dw_plan(_lib.load(), kind, *shape)
    assert p[0] == th and p[1] == (H * W <= 128 * 128) and p[3] == -(-H // th), p
    if kind in (PRE, PRE_SPLIT):
        assert dw_plan(_lib.load(), kind - 2, *shape) == p      # the affine on the fly changes nothing in the plan
    check_kind(kind, shape, case(shape), KIND_IDS[kind])


@pytest.mark.parametrize("kind", [REFLECT, REFLECT_SPLIT], ids=["reflect", "reflect-split32"])
@pytest.mark.parametrize("shape,th", [((1, 63, 17, 40), 8), ((1, 64, 17, 40), 16)], ids=["th8-H63", "th16-H64"])
def test_reflect_strip_heights(shape, th, kind):
    from emdenoise import _lib

    assert dw_plan(_lib.load(), kind, *shape)[:2] == (th, 0) and dw_plan(_lib.load(), REFLECT, *shape)[0] == th
    c = case(shape, True)
    plain = run(REFLECT, c, shape)
    check_fp32(plain, c["ref"], c["bar"], f"reflect {shape}")
    if kind == REFLECT_SPLIT:
        check_split(run(kind, c, shape), plain, shape[3], f"reflect-split32 {shape}")


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("shape,heights", [((2, 37, 19, 40), (4, 8, 16, 32)), ((1, 5, 3, 8), (32,))], ids=["37x19", "5x3"])
def test_forced_strip_heights_give_equal_bits(shape, heights, kind):
    """dw_th = 4, 8, 16, 32 at H = 37: a ragged last strip at each of them (1, 5, 5, 5 rows), at 32 a second strip shorter than the
    first; dw_th = 32 at H = 5: one strip far taller than the image.  All give the bits of the strip height the rule selects (the three
    row contributions of an output are added in the same order at every strip height), and those bits meet the float64 bar."""
    from emdenoise import _lib

    lib = _lib.load()
    c = case(shape)
    assert dw_plan(lib, kind, *shape)[0] == 4
    ruled = run(kind, c, shape)
    try:
        for th in heights:
            _lib.knob("dw_th", th)
            assert dw_plan(lib, kind, *shape)[0] == th and dw_plan(lib, kind, *shape)[3] == -(-shape[1] // th)
            assert np.array_equal(run(kind, c, shape), ruled), (KIND_IDS[kind], shape, th)
        if kind in (PLAIN, PRE):    # the last forced height against float64
            pre = kind == PRE
            check_fp32(run(kind, c, shape), c["ref_pre" if pre else "ref"], c["bar_pre" if pre else "bar"], f"{KIND_IDS[kind]} dw_th {th} {shape}")
    finally:
        _lib.knob("dw_th", 0)
    check_kind(kind, shape, c, KIND_IDS[kind])


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_tile_order_does_not_show(kind):
    """dw_xcd 0 (launch order) against 2 (one contiguous run of tiles per XCD) at (1, 13, 9, 128): 4 strips x 2 channel blocks."""
    from emdenoise import _lib

    lib = _lib.load()
    shape = (1, 13, 9, 128)
    c = case(shape)
    try:
        _lib.knob("dw_xcd", 0)
        assert dw_plan(lib, kind, *shape)[1:3] == (0, 8)
        a = run(kind, c, shape)
        _lib.knob("dw_xcd", 2)
        assert dw_plan(lib, kind, *shape)[1:3] == (1, 8)
        b = run(kind, c, shape)
    finally:
        _lib.knob("dw_xcd", 1)
    assert np.array_equal(a, b)
    check_kind(kind, shape, c, KIND_IDS[kind])
