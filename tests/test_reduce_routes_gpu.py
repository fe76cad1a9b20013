"""The size-selected routes of the two-stage per-channel reductions, at the smallest shapes that select them.

Every reduction of the training path is a producer of double partial sums and a second stage, bn_stats_final<FOLD, TRAIN, CL>
(csrc/dw_misc.hip) or chan_reduce_final<CL> (csrc/bn_train.hip), whose geometry CL = 16 / 4 / 1 follows from the number of partials
per channel (emd::reduce_final_cl: 128 and 1024 are the thresholds).  The op tests elsewhere sit almost entirely in CL = 16; the
shapes here (tests/reduce_route_cases.py; tests/test_reduce_routes.py proves on the CPU which class each one selects) sit on both
sides of each threshold, in CL = 1 with ragged last tiles, per image with B >= 2, and with 36 channels as a tail.

    instance                          launched by (one image list)                   (B >= 2 lists)
    bn_stats_final<0,0,16 | 4 | 1>    conv / split32 / deconv / stats cases          conv, deconv, stats ... -img cases
    bn_stats_final<0,1,16 | 4 | 1>    conv / deconv cases with fold = FoldRequest    conv-2x64x64, conv-2x128x128 / deconv-2x64x64,
      (training fold)                                                                conv-2x256x512 / deconv-2x128x256
    bn_stats_final<1,0,16 | 4 | 1>    split32 cases with fold = (gamma, beta, eps)   -- (the inference fold has one list only)
    chan_reduce_final<16 | 4 | 1>
      with the per-channel step       every bn_backward[_dw] of the dw / slabs /     dw-2x40x72, dw-2x64x512 ..., dw-2x256x1024,
      ("prep")                        cout1 cases                                    dw-2x1022x515-s2, slabs-2x..., cout1-2x...
      plain                           the mask-0 leg (the reduction entry alone)     the same cases
      accumulating                    accum cases (CL 16, 4: at most 512 slabs)      -- (one list only)

Statistics cases assert: y bit for bit the plain convolution's; mean and biased variance against float64 sums of the y the device
wrote, per channel,
    |mean - ref| <= 2^-24 |ref| + N 2^-52 mean|y|,     |var - ref| <= 2^-24 ref + N 2^-52 (ref + mean^2)
(N pixels per sum: sequential double summation of N terms, the cancellation in q / n - m^2 included, plus one rounding to float);
the two-pass form (bn_batch_stats[_images]) against the same reference to the same bar, hence within two bars of the epilogue's
(two correctly rounded floats of nearly equal doubles may still differ by a whole ulp, which one bar does not allow); image 1 of a
batch bit-equal to the image alone; a second run bit-equal; the fold in the same launch bit-equal to bn_train_fold[_images] /
bn_fold on those statistics, the moving statistics updated from image 0.  The ill-conditioned channels (one constant input channel
with a large weight into channels ILL; |mean| / std asserted inside [500, 2000] on the reference) make the variance bar about
6e-5 relative at N = 2^18 where a float anywhere in the chain gives 6e-2.

Backward cases assert: with mask = 0 the two sums s1 = sum g and s2 = sum g (r - mean) rstd against float64 of the written-out
gradient g, to 4 2^-24 sum|g r^| + 2^-24 |ref| (three float roundings per term and the final cast; for s1 the terms are g alone, so
r^ = 1 there); with the relu6 mask the fused form against the unfused one with the bars of
test_bn_backward_of_a_never_written_gradient (2e-5 of the largest element); the per-image form bit-equal to the image alone.

Each case prints its largest ratio to the derived bars before asserting.  Measured on an MI355X: see DESIGN.md 4."""
import ctypes as C

import pytest
import torch

from tests import reduce_route_cases as R
from tests.test_ops_gpu import dev

pytestmark = pytest.mark.gpu

ILL = (0, 1, 35)          # output channels fed by the constant input channel: one in each CL = 16 / CL = 4 group position, and the tail
E24, E52 = 2.0 ** -24, 2.0 ** -52


def gen(seed):
    return torch.Generator(device=dev()).manual_seed(seed)


def randn(g, *shape):
    return torch.randn(*shape, device=dev(), generator=g)


def ratio(got, ref, bar):
    """Largest |got - ref| / bar over the channels (float64)."""
    return float(((got.double() - ref).abs() / bar).max())


# ------------------------------------------------------------------------------------------------ statistics producers
def stat_weights(c, g):
    """Weights of the case [taps, ci, co] (conv, split32) or [3, 3, co, ci] (deconv) on the device, float32.  ill: input channel 0 is
    constant 1 and reaches the channels ILL through one tap that no border cuts, with the weight 1000 x the standard deviation the other
    input channels (unit variance) leave there."""
    ci, co = R.CI, R.CO
    if c.kind == "deconv":
        w = randn(g, 3, 3, co, ci) * (2.0 / (9 * ci + co)) ** 0.5
        if c.ill:
            for o in ILL:
                std = float((w[:, :, o, 1:].double() ** 2).sum() / 4) ** 0.5      # every output pixel belongs to one of four phases
                w[:, :, o, 0] = 0.0
                w[0:2, 0:2, o, 0] = 1000.0 * std     # y[2i + k] += x[i] w[k]: the taps k < 2 of an output pixel never fall outside
        return w
    taps = c.k * c.k
    w = randn(g, taps, ci, co) * (2.0 / (taps * ci + co)) ** 0.5
    if c.ill:
        for o in ILL:
            std = float((w[:, 1:, o].double() ** 2).sum()) ** 0.5
            w[:, 0, o] = 0.0
            w[taps // 2, 0, o] = 1000.0 * std         # the centre tap
    return w


def stat_input(c, g):
    x = randn(g, c.B, c.H, c.W, R.CI) + 0.5
    if c.ill:
        x[..., 0] = 1.0
    return x


def reference(y, nl):
    """float64 mean, biased variance and mean |y| per list and channel of y [B, H, W, C] (nl lists of N pixels), and N."""
    yy = y.double().reshape(nl, -1, y.shape[-1])
    m = yy.mean(1)
    v = ((yy - m[:, None]) ** 2).mean(1)
    return m.reshape(-1), v.reshape(-1), yy.abs().mean(1).reshape(-1), yy.shape[1]


def check_stats(tag, mean, var, ref, n_terms):
    rm, rv, rabs, _ = ref
    bar_m = E24 * rm.abs() + n_terms * E52 * rabs
    bar_v = E24 * rv + n_terms * E52 * (rv + rm ** 2)
    a, b = ratio(mean, rm, bar_m), ratio(var, rv, bar_v)
    print(f"    {tag}: mean {a:.3f}, var {b:.3f} of the bar (largest relative bar on var {float((bar_v / rv).max()):.2e})")
    return a, b


@pytest.mark.parametrize("c", R.STATS, ids=R.case_id)
def test_statistics_route(c):
    from emdenoise import ops, train_ops as TO

    idx = R.STATS.index(c)
    g = gen(4000 + idx)
    B, co, images = c.B, R.CO, c.images
    nl = B if images else 1
    print(f"\n{R.case_id(c)}: {R.stat_nslab(c)} partials per channel, CL = {c.cl}")
    if c.kind == "stats":
        y = randn(g, B, c.H, c.W, co) * 0.7 + 0.3
        if c.ill:
            for o in ILL:
                y[..., o] += 700.0
        ya = ops.Act(y)
        run = lambda a=ya: (ops.bn_batch_stats_images if images else ops.bn_batch_stats)(a)
        mean, var = run()
        y_view = y
    else:
        x, w = stat_input(c, g), stat_weights(c, g)
        ones, zeros = torch.ones(co, device=dev()), torch.zeros(co, device=dev())
        if c.kind == "deconv":
            pk = ops.pack_deconv(w.cpu().numpy(), dev())
            Ho, Wo = 2 * c.H, 2 * c.W
        else:
            pk = ops.PackedWeights(w.cpu().numpy(), False, dev())
            Ho, Wo = -(-c.H // c.stride), -(-c.W // c.stride)
        out = lambda b=B: ops.Act(torch.full((b, Ho, Wo, co + 4), float("nan"), device=dev()), co, 0)
        y1, y2 = out(), out()
        if c.kind == "conv":
            xa = ops.Act(x)
            assert ops.conv_stats_supported(xa, c.stride, images)
            run = lambda a=xa, o=y1, **kw: ops.conv_stats(a, pk, ones, zeros, o, stride=c.stride, rate=c.rate, images=images, **kw)
            if c.k == 1:
                ops.conv1x1(xa, pk, ones, zeros, y2, stride=c.stride, act=False)
            else:
                ops.conv3x3(xa, pk, ones, zeros, y2, rate=c.rate, act=False)
        elif c.kind == "deconv":
            xa = ops.Act(x)
            run = lambda a=xa, o=y1, **kw: ops.deconv_stats(a, pk, ones, zeros, o, images=images, **kw)
            ops.deconv3x3s2(xa, pk, ones, zeros, y2, act=False)
        else:
            xa = ops.to_split32(ops.Act(x))
            run = lambda a=xa, o=y1, **kw: ops.conv1x1_split32(a, pk, ones, zeros, o, act=ops.ACT_NONE, stats=True, **kw)[1:]
            ops.conv1x1_split32(xa, pk, ones, zeros, y2, act=ops.ACT_NONE)
        mean, var = run()
        torch.cuda.synchronize()
        assert torch.equal(y1.torch(), y2.torch()), "y must be the plain convolution's, bit for bit"
        y_view = y2.torch()
    torch.cuda.synchronize()
    # float64 of the y the device wrote
    ref = reference(y_view, nl)
    n_terms = ref[3]
    assert mean.numel() == nl * co and bool(torch.isfinite(mean).all()) and bool(torch.isfinite(var).all())
    if c.ill:
        cond = (ref[0].abs() / ref[1].sqrt()).reshape(nl, co)[:, list(ILL)]
        print(f"    |mean| / std of the ill-conditioned channels: {float(cond.min()):.0f} .. {float(cond.max()):.0f}")
        assert float(cond.min()) >= 500 and float(cond.max()) <= 2000
    a, b = check_stats("epilogue" if c.kind != "stats" else "two-pass", mean, var, ref, n_terms)
    ok = a <= 1.0 and b <= 1.0
    if c.kind != "stats":
        m2, v2 = (ops.bn_batch_stats_images if images else ops.bn_batch_stats)(y2)
        torch.cuda.synchronize()
        a2, b2 = check_stats("two-pass", m2, v2, ref, n_terms)
        ok = ok and a2 <= 1.0 and b2 <= 1.0
        # ... and so the two forms against each other, to two bars
        bar_m = 2 * (E24 * ref[0].abs() + n_terms * E52 * ref[2])
        bar_v = 2 * (E24 * ref[1] + n_terms * E52 * (ref[1] + ref[0] ** 2))
        a3, b3 = ratio(mean, m2.double(), bar_m), ratio(var, v2.double(), bar_v)
        print(f"    epilogue against two-pass: mean {a3:.3f}, var {b3:.3f} of two bars")
        ok = ok and a3 <= 1.0 and b3 <= 1.0
    assert ok, "a statistic misses its derived bar (figures above)"
    # determinism
    mean_b, var_b = run()
    torch.cuda.synchronize()
    assert torch.equal(mean, mean_b) and torch.equal(var, var_b), "a second run must give the same bits"
    # image 1 of the batch alone
    if images:
        if c.kind == "stats":
            mo, vo = run(ops.Act(y[1:2].contiguous()))
        else:
            mo, vo = run(ops.Act(x[1:2].contiguous()), out(1))
        torch.cuda.synchronize()
        assert torch.equal(mo, mean[co:2 * co]) and torch.equal(vo, var[co:2 * co]), "image 1 must not depend on its batch"
    # the fold in the same launch
    if c.kind in ("conv", "deconv"):
        double_bn = idx % 2 == 0
        gamma2, beta2 = torch.rand(co, device=dev(), generator=g) + 0.5, randn(g, co)
        gamma1, beta1 = (torch.rand(co, device=dev(), generator=g) + 0.5, randn(g, co)) if double_bn else (None, None)
        moving = lambda: [t for _ in range(2 if double_bn else 1) for t in (torch.zeros(co, device=dev()), torch.ones(co, device=dev()))]
        mv_a, mv_b, mv_c = moving(), moving(), moving()
        req = TO.FoldRequest(dev(), B if images else 0, co, gamma2, beta2, gamma1=gamma1, beta1=beta1, moving=mv_a)
        y3 = out()
        mean_f, var_f = run(o=y3, fold=req)
        want = TO.bn_train_fold(mean, var, gamma2, beta2, n_terms, gamma1=gamma1, beta1=beta1, moving=mv_b, images=B if images else 0)
        TO.bn_train_fold(mean[:co].contiguous(), var[:co].contiguous(), gamma2, beta2, n_terms, gamma1=gamma1, beta1=beta1, moving=mv_c)
        torch.cuda.synchronize()
        assert torch.equal(y3.torch(), y2.torch()) and torch.equal(mean_f, mean) and torch.equal(var_f, var)
        got = req.result(mean_f)
        for k in ("scale", "shift", "rstd1") + (("rstd2",) if double_bn else ()):
            assert torch.equal(got[k], want[k]), f"training fold: {k} differs from bn_train_fold's"
        for u, v, w0 in zip(mv_a, mv_b, mv_c):
            assert torch.equal(u, v) and torch.equal(u, w0), "moving statistics: the update from image 0, bit for bit"
        assert not torch.equal(mv_a[-2], torch.zeros(co, device=dev())) and not torch.equal(mv_a[-1], torch.ones(co, device=dev()))
    elif c.kind == "split32":
        beta, gamma = randn(g, co) * 0.4, torch.rand(co, device=dev(), generator=g) + 0.5
        for gm in (None, gamma):
            y3 = out()
            _, m3, v3, sc, sh = ops.conv1x1_split32(xa, pk, ones, zeros, y3, act=ops.ACT_NONE, stats=True, fold=(gm, beta, 1e-3))
            sc2, sh2 = ops.bn_fold(mean, var, gm, beta, 1e-3)
            torch.cuda.synchronize()
            assert torch.equal(y3.torch(), y2.torch()) and torch.equal(m3, mean) and torch.equal(v3, var)
            assert torch.equal(sc, sc2) and torch.equal(sh, sh2), "inference fold: differs from bn_fold's"


# ------------------------------------------------------------------------------------------------ backward producers
def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def dw_reduce(dd, wf, r, fold, mask, images, c, gdw=None):
    """emd_dw3x3_bn_bwd_reduce_f32 alone, no per-channel step: the plain chan_reduce_final -> (s1, s2)."""
    from emdenoise import _lib, ops

    lib = _lib.load()
    n = (c.B if images else 1) * c.C
    s1, s2 = torch.empty(n, device=dev()), torch.empty(n, device=dev())
    ws = ops.workspace(lib.emd_dw3x3_bn_bwd_workspace_bytes(c.B, c.H, c.W, c.C), dev())
    ms, mh = (fold["scale"], fold["shift"]) if mask else (None, None)
    _lib.check(lib.emd_dw3x3_bn_bwd_reduce_f32(dd.ptr, dd.ld, _p(wf), r.ptr, r.ld, _p(fold["mean"]), _p(fold["rstd1"]), _p(ms), _p(mh), mask,
                                               1 if images else 0, c.B, c.H, c.W, c.C, c.stride, c.rate, _p(s1), _p(s2), _p(gdw), _p(ws), None,
                                               _lib.stream_ptr(None)), "emd_dw3x3_bn_bwd_reduce_f32")
    return s1, s2


def slab_reduce(dy, r, fold, images, c):
    """emd_bn_bwd_reduce[_images]_f32 alone, mask 0 -> (s1, s2)."""
    from emdenoise import _lib, ops, train_ops as TO

    lib = _lib.load()
    n = (c.B if images else 1) * c.C
    s1, s2 = torch.empty(n, device=dev()), torch.empty(n, device=dev())
    if not images:
        TO.chan_reduce(dy, s1, r, fold["mean"], fold["rstd1"], s2)
        return s1, s2
    npix = c.H * c.W
    ws = ops.workspace(c.B * lib.emd_chan_reduce_workspace_bytes(npix, c.C), dev())
    _lib.check(lib.emd_bn_bwd_reduce_images_f32(dy.ptr, dy.ld, r.ptr, r.ld, _p(fold["mean"]), _p(fold["rstd1"]), None, None, 0, c.B,
                                                C.c_long(npix), c.C, _p(s1), _p(s2), _p(ws), _lib.stream_ptr(None)),
               "emd_bn_bwd_reduce_images_f32")
    return s1, s2


def check_sums(s1, s2, gy, r0, fold, nl, Cc):
    """The two sums against float64 of the written-out gradient gy [B, H, W, C]."""
    G = gy.double().reshape(nl, -1, Cc)
    rhat = (r0.double().reshape(nl, -1, Cc) - fold["mean"].double().view(nl, 1, Cc)) * fold["rstd1"].double().view(nl, 1, Cc)
    ref1, ref2 = G.sum(1).reshape(-1), (G * rhat).sum(1).reshape(-1)
    bar1 = 4 * E24 * G.abs().sum(1).reshape(-1) + E24 * ref1.abs()
    bar2 = 4 * E24 * (G * rhat).abs().sum(1).reshape(-1) + E24 * ref2.abs()
    a, b = ratio(s1, ref1, bar1), ratio(s2, ref2, bar2)
    print(f"    mask 0 against float64: s1 {a:.3f}, s2 {b:.3f} of the bar")
    assert a <= 1.0 and b <= 1.0


def make_fold(r0, c, g):
    from emdenoise import ops, train_ops as TO

    Cc, images = c.C, c.images
    gamma2, beta2 = torch.rand(Cc, device=dev(), generator=g) + 0.5, randn(g, Cc)
    gamma1, beta1 = (torch.rand(Cc, device=dev(), generator=g) + 0.5, randn(g, Cc)) if c.double_bn else (None, None)

    def fold_of(r, b):
        mean, var = (ops.bn_batch_stats_images if images else ops.bn_batch_stats)(ops.Act(r.clone()))
        return TO.bn_train_fold(mean, var, gamma2, beta2, c.H * c.W if images else b * c.H * c.W, gamma1=gamma1, beta1=beta1,
                                images=b if images else 0)

    return gamma2, gamma1, fold_of


@pytest.mark.parametrize("c", [c for c in R.BWD if c.kind == "dw"], ids=R.case_id)
def test_fused_depthwise_backward_route(c):
    from emdenoise import ops, train_ops as TO

    g = gen(5000 + R.BWD.index(c))
    B, H, W, Cc, images = c.B, c.H, c.W, c.C, c.images
    nl = B if images else 1
    print(f"\n{R.case_id(c)}: {R.bwd_nslab(c)} partials per channel, CL = {c.cl}")
    r0 = randn(g, B, H, W, Cc) * 2
    Ho, Wo = -(-H // c.stride), -(-W // c.stride)
    dd = ops.Act(randn(g, B, Ho, Wo, Cc))
    wf = randn(g, 9, Cc) * 0.3
    w0 = wf.flip(0).contiguous()
    gamma2, gamma1, fold_of = make_fold(r0, c, g)
    fold = fold_of(r0, B)

    def written(ddx, b):
        if c.stride == 1:
            return ops.dw3x3(ddx, wf, ops.Act.empty(b, H, W, Cc, dev()), rate=c.rate)
        return TO.dw3x3_bwd_data(ddx, w0, ops.Act.empty(b, H, W, Cc, dev()), stride=c.stride, rate=c.rate)

    gy = written(dd, B)
    # mask 0: the sums against float64
    s1, s2 = dw_reduce(dd, wf, ops.Act(r0.clone()), fold, 0, images, c)
    torch.cuda.synchronize()
    check_sums(s1, s2, gy.torch(), r0, fold, nl, Cc)
    # relu6 mask: fused against unfused
    def backward(fused, r_in, dd_in, f, b):
        r = ops.Act(r_in.clone())
        dg2, db2 = torch.zeros(Cc, device=dev()), torch.zeros(Cc, device=dev())
        dg1 = torch.zeros(Cc, device=dev()) if c.double_bn else None
        gdw = torch.zeros(9, Cc, device=dev())
        if fused:
            TO.bn_backward_dw(TO.DwGrad(dd_in, wf, gdw if c.wg else None, stride=c.stride, rate=c.rate, hw=(H, W)), r, f, gamma2, dg2, db2, r,
                              mask=TO.MASK_RELU6, gamma1=gamma1, dgamma1=dg1)
        else:
            if c.wg:
                TO.dw3x3_wgrad_pre(ops.PreAct(r, f["scale"], f["shift"], images=images, act=ops.ACT_RELU6), dd_in, gdw, stride=c.stride,
                                   rate=c.rate)
            TO.bn_backward(written(dd_in, b), r, f, gamma2, dg2, db2, r, mask=TO.MASK_RELU6, gamma1=gamma1, dgamma1=dg1)
        torch.cuda.synchronize()
        return r.buf, dg2, db2, dg1, gdw if c.wg else None

    a, b = backward(True, r0, dd, fold, B), backward(False, r0, dd, fold, B)
    assert not torch.isnan(a[0]).any()
    worst = (a[0] - b[0]).abs().max().item() / b[0].abs().max().item()
    for u, v in zip(a[1:], b[1:]):
        if u is not None:
            worst = max(worst, (u - v).abs().max().item() / max(v.abs().max().item(), 1e-3))
    print(f"    relu6 mask, fused against unfused: largest distance {worst:.2e} of the largest element (bar 2e-5)")
    assert worst < 2e-5
    if c.wg:
        assert b[4].abs().max().item() > 0
    if images:   # image 1 alone
        r1, dd1 = r0[1:2].contiguous(), ops.Act(dd.torch()[1:2].contiguous())
        alone = backward(True, r1, dd1, fold_of(r1, 1), 1)
        assert torch.equal(alone[0][0], a[0][1]), "the per-image form must give the bits of the image alone"


@pytest.mark.parametrize("c", [c for c in R.BWD if c.kind == "slabs"], ids=R.case_id)
def test_slab_backward_route(c, monkeypatch):
    """bn_backward on a written gradient: the sums against float64 (mask 0), and the per-channel step inside chan_reduce_final against
    the same step as a launch of its own: the same function on the same sums, so dr bit for bit; the parameter gradients are added
    with float atomics, 2e-6 as test_bn_backward_per_image_at_tower_sizes has it."""
    from emdenoise import ops, train_ops as TO

    g = gen(5000 + R.BWD.index(c))
    B, H, W, Cc, images = c.B, c.H, c.W, c.C, c.images
    nl = B if images else 1
    print(f"\n{R.case_id(c)}: {R.bwd_nslab(c)} partials per channel, CL = {c.cl}")
    r0, dy0 = randn(g, B, H, W, Cc) * 2, randn(g, B, H, W, Cc)
    gamma2, gamma1, fold_of = make_fold(r0, c, g)
    fold = fold_of(r0, B)
    s1, s2 = slab_reduce(ops.Act(dy0), ops.Act(r0), fold, images, c)
    torch.cuda.synchronize()
    check_sums(s1, s2, dy0, r0, fold, nl, Cc)

    def backward(r_in, dy_in, f, b):
        dg2, db2 = torch.zeros(Cc, device=dev()), torch.zeros(Cc, device=dev())
        dg1 = torch.zeros(Cc, device=dev()) if c.double_bn else None
        dr = TO.bn_backward(ops.Act(dy_in), ops.Act(r_in), f, gamma2, dg2, db2, ops.Act.empty(b, H, W, Cc, dev()), mask=TO.MASK_RELU6,
                            gamma1=gamma1, dgamma1=dg1)
        torch.cuda.synchronize()
        return dr.buf, dg2, db2, dg1

    assert TO.FUSE_PREP
    a = backward(r0, dy0, fold, B)
    monkeypatch.setattr(TO, "FUSE_PREP", False)
    b = backward(r0, dy0, fold, B)
    monkeypatch.setattr(TO, "FUSE_PREP", True)
    assert torch.equal(a[0], b[0])
    for u, v in zip(a[1:], b[1:]):
        if u is not None:
            assert float((u - v).norm() / v.norm().clamp_min(1e-20)) < 2e-6
    if images:
        r1, dy1 = r0[1:2].contiguous(), dy0[1:2].contiguous()
        alone = backward(r1, dy1, fold_of(r1, 1), 1)
        assert torch.equal(alone[0][0], a[0][1]), "the per-image form must give the bits of the image alone"


@pytest.mark.parametrize("c", [c for c in R.BWD if c.kind == "cout1"], ids=R.case_id)
def test_cout1_backward_route(c):
    """The never-written gradient of the final conv: with mask 0 the two sums of emd_bn_bwd_reduce_prep_cout1_f32 against float64 of
    the written-out gradient (conv3x3_cout1_bwd_data) -- the fused-against-unfused comparison alone shares the second stage between
    its two legs --, then exactly what test_bn_backward_of_the_final_convs_data_gradient checks."""
    import tests.test_train_ops_gpu as TOG
    from emdenoise import _lib, ops, train_ops as TO

    g = gen(5000 + R.BWD.index(c))
    B, H, W, Cc, images = c.B, c.H, c.W, c.C, c.images
    nl = B if images else 1
    print(f"\n{R.case_id(c)}: {R.bwd_nslab(c)} partials per channel, CL = {c.cl}")
    r0 = randn(g, B, H, W, Cc) * 2
    g1 = randn(g, B, H, W, 1).contiguous()
    w9 = (randn(g, 9, Cc) * 0.3).contiguous()
    gamma2, gamma1, fold_of = make_fold(r0, c, g)
    fold = fold_of(r0, B)
    gy = TO.conv3x3_cout1_bwd_data(g1, w9, ops.Act.empty(B, H, W, Cc, dev()))
    lib = _lib.load()
    n = nl * Cc
    s1, s2, K, m1, m2 = (torch.empty(n, device=dev()) for _ in range(5))
    dg2, db2 = torch.zeros(Cc, device=dev()), torch.zeros(Cc, device=dev())
    dg1 = torch.zeros(Cc, device=dev()) if c.double_bn else None
    prep = TO._prep_struct(fold, gamma1, gamma2, TO.BN_EPS, K, m1, m2, dg1, dg2, db2)
    npix = H * W if images else B * H * W
    ws = ops.workspace(nl * lib.emd_chan_reduce_workspace_bytes(npix, Cc), dev())
    r = ops.Act(r0)
    _lib.check(lib.emd_bn_bwd_reduce_prep_cout1_f32(_p(g1), _p(w9), B, H, W, r.ptr, r.ld, _p(fold["mean"]), _p(fold["rstd1"]), None, None, 0,
                                                    1 if images else 0, Cc, _p(s1), _p(s2), _p(ws), C.byref(prep), _lib.stream_ptr(None)),
               "emd_bn_bwd_reduce_prep_cout1_f32")
    torch.cuda.synchronize()
    check_sums(s1, s2, gy.torch(), r0, fold, nl, Cc)
    TOG.test_bn_backward_of_the_final_convs_data_gradient(B, H, W, Cc, images, c.double_bn)


@pytest.mark.parametrize("c", [c for c in R.BWD if c.kind == "accum"], ids=R.case_id)
def test_accumulating_reduction_route(c):
    """The bias gradient: s1 += sum dy.  Bar: the double sum of N terms, its rounding to float and the float add onto s1."""
    from emdenoise import ops, train_ops as TO

    g = gen(5000 + R.BWD.index(c))
    dy = randn(g, c.B, c.H, c.W, c.C) + 0.25
    s1 = torch.full((c.C,), 1.0, device=dev())
    TO.chan_reduce(ops.Act(dy), s1, accumulate_s1=True)
    torch.cuda.synchronize()
    D = dy.double().reshape(-1, c.C)
    ref = D.sum(0)
    bar = E24 * ref.abs() + E24 * (1.0 + ref).abs() + D.shape[0] * E52 * D.abs().sum(0)
    a = ratio(s1, 1.0 + ref, bar)
    print(f"\n{R.case_id(c)}: {R.bwd_nslab(c)} partials per channel, CL = {c.cl}: s1 {a:.3f} of the bar")
    assert a <= 1.0
