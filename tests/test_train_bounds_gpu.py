"""Guard-banded runs of the training entry points that take pointers and no sizes (tests/guarded.py).

Every case puts its inputs into guarded, pattern-padded buffers (pitch C + 8, offset 4 where the entry point takes a pitch: a read
outside the operand that reaches the result poisons it), takes every output, every per-channel vector and -- through the substituted
allocator ops.workspace -- every workspace from guarded memory, and after the device has finished asserts
  * the values against the float64 reference the op tests use (oracle/tf_ops.py autograd, numpy for the statistics), to their bars:
    weight gradients 2e-5, float32 element-wise / gather kernels 2e-6, split-bf16 matrix-core results 2e-5, statistics 2e-7 (mean) and
    2e-6 (variance), the batch-norm backward 1e-5 (tests/test_train_ops_gpu.py, tests/test_gan_train_gpu.py);
  * that an output which must be written completely holds the pattern nowhere;
  * that every guard and every pad column still holds the pattern, compared as integers.
The vectors the wrappers allocate themselves (mean, var, s1, s2, K, m1, m2, the folded scale / shift) are guarded by substituting
torch.empty / torch.empty_like for the length of the call (guarded.Vectors).  The shapes are the smallest that put each producer on a
ragged edge; the guard checks have no tolerance.

Refusals: none.  Every listed shape is accepted at pitch C + 8 / offset 4 by every entry point that takes a pitch, so no case is left
out or replaced by an assertion of an error code (emd_dw7_c1_reflect[_wgrad]_f32 takes no pitch: its 4-channel tensors are dense).

Two negative controls show that the check can fail on the device: one element written into a rear guard with torch, and deconv_stats
at (3, 8, 12, 128, 32) with the workspace of the size the library advertised before the + 3 rows of emd_conv_stats_workspace_bytes:
three rows (1 536 bytes) short, the over-run lands in the test's own 64 KiB guard."""
import numpy as np
import pytest
import torch

from tests import guarded as G
from tests.test_ops_gpu import dev, rel_l2, rnd, t64
from tests.test_train_ops_gpu import TOL_F32, TOL_WGRAD, TOL_X3, _bn_train_t, dw3x3_reference, leaf

pytestmark = pytest.mark.gpu

TOL_MEAN, TOL_VAR, TOL_BN = 2e-7, 2e-6, 1e-5

class Bench:
    """The guarded buffers of one case and their checks."""

    def __init__(self, monkeypatch):
        from emdenoise import ops

        self.mp, self.checks, self.ws, self.vec = monkeypatch, [], G.Workspaces(), G.Vectors()
        monkeypatch.setattr(ops, "workspace", self.ws)

    def _keep(self, pair):
        self.checks.append(pair[1])
        return pair[0]

    def x(self, a, pitch=True, name="input"):
        """An input activation [B,H,W,C] in a padded, guarded buffer."""
        B, H, W, Cc = a.shape
        return self._keep(G.guarded_act(B, H, W, Cc, ld=Cc + 8 if pitch else None, c0=4 if pitch else 0, fill=a, name=name))

    def y(self, B, H, W, Cc, pitch=True, fill=None, name="output"):
        """An output activation: the pattern (must be written completely) or a base (accumulating)."""
        return self._keep(G.guarded_act(B, H, W, Cc, ld=Cc + 8 if pitch else None, c0=4 if pitch else 0, fill=fill, name=name))

    def v(self, a, dtype=torch.float32, name="vector"):
        """A guarded tensor holding the array a (inputs, bases of accumulating outputs), in a's shape."""
        a = np.asarray(a)
        return self._keep(G.guarded(a.size, dtype, dev(), fill=torch.from_numpy(np.ascontiguousarray(a)), name=name)).view(a.shape)

    def out(self, shape, dtype=torch.float32, name="output"):
        """A guarded output holding the pattern."""
        return self._keep(G.guarded(int(np.prod(shape)), dtype, dev(), name=name)).view(shape)

    def vectors(self):
        return self.vec.installed(self.mp)

    def finish(self, ws=0):
        torch.cuda.synchronize()
        for c in self.checks:
            c()
        self.vec.check()
        if ws is not None:
            self.ws.check(at_least=ws)


@pytest.fixture
def gb(monkeypatch):
    return Bench(monkeypatch)


def written(*ts):
    for i, t in enumerate(ts):
        if t is not None:
            G.assert_written(t, f"output {i}")


def show(tag, **figs):
    print(f"    {tag}: " + ", ".join(f"{k} {v:.2e} (bar {b:.0e})" for k, (v, b) in figs.items()))
    for k, (v, b) in figs.items():
        assert v < b, (tag, k, v, b)


# ------------------------------------------------------------------------------------------------ negative controls
def test_a_write_into_a_rear_guard_is_seen_on_the_device(gb):
    y = gb.out((37,))
    gb.finish()
    y.fill_(1.0)
    gb.finish()
    gb.checks[0].parent[gb.checks[0].start + 37] = 0          # one element behind the view
    with pytest.raises(AssertionError, match="rear guard changed at element 37 "):
        gb.finish()
    a = gb.y(1, 2, 3, 8)
    a.buf[0, 1, 2, 13] = 1.0                                   # a 16-byte tail store's first victim: the next channels of the row
    with pytest.raises(AssertionError, match="pad column 13 of pixel 5 "):
        gb.checks[1]()


def deconv_stats_case(gb, B, H, W, ci, co, images, fold=False):
    from emdenoise import ops, train_ops as TO
    from oracle import tf_ops as T

    x = rnd((B, H, W, ci), 720, positive=True)
    w = rnd((3, 3, co, ci), 721, scale=(2.0 / (9 * ci + co)) ** 0.5)
    ph = ops.pack_deconv(w, dev())
    ones, zeros = gb.v(np.ones(co, np.float32)), gb.v(np.zeros(co, np.float32))
    xa, y = gb.x(x), gb.y(B, 2 * H, 2 * W, co)
    req = None
    with gb.vectors():
        if fold:
            g2, b2 = gb.v(rnd((co,), 722, 0.3) + 1.2), gb.v(rnd((co,), 723, 0.5))
            mv = [gb.v(np.zeros(co, np.float32)), gb.v(np.ones(co, np.float32))]
            req = TO.FoldRequest(dev(), B if images else 0, co, g2, b2, moving=mv)
        mean, var = ops.deconv_stats(xa, ph, ones, zeros, y, images=images, fold=req)
    return x, w, y, mean, var, req, (g2, b2) if fold else None


def test_the_workspace_size_from_before_the_fix_trips_the_guard(gb):
    """emd_deconv3x3s2_stats_f32 at (3, 8, 12, 128, 32): m = 288 input pixels, four phases x ceil(288 / 128) = 12 rows of partials against
    the ceil(4 * 288 / 128) = 9 the size function advertised before it added three rows."""
    from emdenoise import _lib, ops

    B, H, W, ci, co = 3, 8, 12, 128, 32
    have = _lib.load().emd_conv_stats_workspace_bytes(4 * B * H * W, co)
    short = -(-4 * B * H * W // 128) * 2 * co * 8
    assert have - short == 3 * 2 * co * 8 == 1536
    gb.ws = G.Workspaces(shrink_bytes=have - short)
    gb.mp.setattr(ops, "workspace", gb.ws)
    deconv_stats_case(gb, B, H, W, ci, co, False)
    torch.cuda.synchronize()
    with pytest.raises(AssertionError, match=r"workspace 0 \(6144 bytes\): rear guard changed at element \d+ ") as e:
        gb.finish(ws=1)
    first = int(str(e.value).split("changed at element ")[1].split()[0])
    assert 576 <= first < 768, first          # inside the three missing rows of 2 x 32 doubles


# ------------------------------------------------------------------------------------------------ statistics epilogues
def check_stats(y_dev, mean, var, images):
    yy = y_dev.double().cpu().numpy()
    ax = (1, 2) if images else (0, 1, 2)
    show("statistics", mean=(rel_l2(mean.cpu().numpy(), yy.mean(ax).ravel()), TOL_MEAN), var=(rel_l2(var.cpu().numpy(), yy.var(ax).ravel()), TOL_VAR))


def check_train_fold(gb, req, mean, var, gb2, npix, images):
    """The fold of the statistics' final kernel == bn_train_fold on those statistics (itself under guards), bit for bit."""
    from emdenoise import train_ops as TO

    co = gb2[0].numel()
    mv = [gb.v(np.zeros(co, np.float32)), gb.v(np.ones(co, np.float32))]
    with gb.vectors():
        want = TO.bn_train_fold(mean, var, gb2[0], gb2[1], npix, moving=mv, images=images)
    gb.finish(ws=None)
    got = req.result(mean)
    for k in ("scale", "shift", "rstd1"):
        written(got[k])
        assert torch.equal(got[k], want[k]), k
    # against float64: scale = gamma / sqrt(var + eps), shift = beta - mean * scale
    m64, v64 = mean.double().cpu().numpy(), var.double().cpu().numpy()
    n = images or 1
    g64, b64 = np.tile(gb2[0].double().cpu().numpy(), n), np.tile(gb2[1].double().cpu().numpy(), n)
    sc = g64 / np.sqrt(v64 + 1e-3)
    show("fold", scale=(rel_l2(got["scale"].cpu().numpy(), sc), TOL_F32), shift=(rel_l2(got["shift"].cpu().numpy(), b64 - m64 * sc), TOL_F32))


CONV_STATS = [
    # B, H, W, ci, co, k, stride, rate, images
    (1, 9, 13, 64, 36, 1, 1, 1, False),      # M = 117: one partial tile
    (2, 20, 12, 64, 64, 1, 1, 1, False),     # M = 480
    (3, 11, 13, 32, 36, 1, 2, 1, False),     # stride 2: M = 3 * 6 * 7 = 126
    (2, 16, 8, 64, 64, 1, 1, 1, True),       # one tile per image
    (3, 16, 24, 64, 36, 1, 1, 1, True),      # three tiles per image
    (1, 12, 11, 32, 36, 3, 1, 6, False),     # 3x3 at rate 6: M = 132, two tiles
]


@pytest.mark.parametrize("fold", [False, True], ids=["plain", "fold"])
@pytest.mark.parametrize("B,H,W,ci,co,k,stride,rate,images", CONV_STATS)
def test_conv_stats(gb, B, H, W, ci, co, k, stride, rate, images, fold):
    from emdenoise import ops, train_ops as TO
    from oracle import tf_ops as T

    x = rnd((B, H, W, ci), 700, positive=True)
    w = rnd((k * k, ci, co), 701, scale=(2.0 / (k * k * ci + co)) ** 0.5)
    pk = ops.PackedWeights(w, False, dev())
    ones, zeros = gb.v(np.ones(co, np.float32)), gb.v(np.zeros(co, np.float32))
    Ho, Wo = -(-H // stride), -(-W // stride)
    xa, y = gb.x(x), gb.y(B, Ho, Wo, co)
    assert ops.conv_stats_supported(xa, stride, images)
    req = None
    with gb.vectors():
        if fold:
            g2, b2 = gb.v(rnd((co,), 702, 0.3) + 1.2), gb.v(rnd((co,), 703, 0.5))
            req = TO.FoldRequest(dev(), B if images else 0, co, g2, b2, moving=[gb.v(np.zeros(co, np.float32)), gb.v(np.ones(co, np.float32))])
        mean, var = ops.conv_stats(xa, pk, ones, zeros, y, stride=stride, rate=rate, images=images, fold=req)
    gb.finish(ws=1)
    written(y.torch(), mean, var)
    ref = T.conv2d_t(t64(x), t64(w.reshape(k, k, ci, co)), None, stride=stride, rate=rate).numpy()
    show("conv", y=(rel_l2(y.torch().cpu().numpy(), ref), TOL_X3))
    check_stats(y.torch(), mean, var, images)
    if fold:
        check_train_fold(gb, req, mean, var, (g2, b2), Ho * Wo if images else B * Ho * Wo, B if images else 0)


DECONV_STATS = [
    (1, 8, 8, 64, 32, False),       # m = 64: 4 rows written where ceil(4 m / 128) = 2
    (3, 8, 12, 128, 32, False),     # m = 288: 12 against 9
    (1, 9, 15, 32, 36, False),      # m = 135: 8 against 5
    (2, 16, 8, 64, 64, True),       # per image, one tile per phase and image
]


@pytest.mark.parametrize("fold", [False, True], ids=["plain", "fold"])
@pytest.mark.parametrize("B,H,W,ci,co,images", DECONV_STATS)
def test_deconv_stats(gb, B, H, W, ci, co, images, fold):
    from oracle import tf_ops as T

    x, w, y, mean, var, req, gb2 = deconv_stats_case(gb, B, H, W, ci, co, images, fold)
    gb.finish(ws=1)
    written(y.torch(), mean, var)
    ref = T.conv2d_transpose_s2_t(t64(x), t64(w), None).numpy()
    show("deconv", y=(rel_l2(y.torch().cpu().numpy(), ref), TOL_X3))
    check_stats(y.torch(), mean, var, images)
    if fold:
        check_train_fold(gb, req, mean, var, gb2, 4 * H * W if images else 4 * B * H * W, B if images else 0)


def split_input(gb, x):
    """x [B,H,W,C] as a split32 activation whose buffer is guarded (ops.SplitAct allocates its own)."""
    from emdenoise import _lib, ops

    B, H, W, Cc = x.shape
    s = object.__new__(ops.SplitAct)
    s.B, s.H, s.W, s.C, s.ld = B, H, W, Cc, _lib.load().emd_split32_ld(Cc)
    s.buf = gb.out((B, H, W, s.ld), name="split32 activation")
    return ops.to_split32(gb.x(x), s)


@pytest.mark.parametrize("fold", [False, True], ids=["plain", "fold"])
@pytest.mark.parametrize("B,H,W,ci,co", [(1, 16, 16, 64, 36),        # M = 256: exactly one row of partials
                                         (1, 19, 23, 96, 132),       # M = 437
                                         (2, 19, 23, 96, 132)])      # M = 874
def test_conv1x1_split32_stats(gb, B, H, W, ci, co, fold):
    from emdenoise import ops
    from oracle import tf_ops as T

    x = rnd((B, H, W, ci), 730, positive=True)
    w = rnd((1, ci, co), 731, scale=(2.0 / (ci + co)) ** 0.5)
    pk = ops.PackedWeights(w, False, dev())
    ones, zeros = gb.v(np.ones(co, np.float32)), gb.v(np.zeros(co, np.float32))
    xs, y = split_input(gb, x), gb.y(B, H, W, co)
    beta, gamma = gb.v(rnd((co,), 732, 0.4)), gb.v(rnd((co,), 733, 0.2) + 1.0)
    with gb.vectors():
        got = ops.conv1x1_split32(xs, pk, ones, zeros, y, act=ops.ACT_NONE, stats=True, fold=(gamma, beta, 1e-3) if fold else None)
    gb.finish(ws=1)
    mean, var = got[1], got[2]
    written(y.torch(), *got[1:])
    ref = T.conv2d_t(t64(x), t64(w.reshape(1, 1, ci, co)), None).numpy()
    show("split32", y=(rel_l2(y.torch().cpu().numpy(), ref), TOL_X3))
    check_stats(y.torch(), mean, var, False)
    if fold:
        sc = gamma.double().cpu().numpy() / np.sqrt(var.double().cpu().numpy() + 1e-3)
        sh = beta.double().cpu().numpy() - mean.double().cpu().numpy() * sc
        show("fold", scale=(rel_l2(got[3].cpu().numpy(), sc), TOL_F32), shift=(rel_l2(got[4].cpu().numpy(), sh), TOL_F32))


STATS_SHAPES = [(1, 7, 9, 36), (1, 8, 8, 36), (1, 5, 13, 36), (3, 5, 13, 36),      # 63, 64, 65 pixels; 195 = three slabs and a tail
                (1, 181, 183, 8)]                                                    # 33 123 pixels: 65-row slabs, the last one ragged


@pytest.mark.parametrize("images", [False, True], ids=["batch", "images"])
@pytest.mark.parametrize("B,H,W,Cc", STATS_SHAPES)
def test_bn_batch_stats(gb, B, H, W, Cc, images):
    from emdenoise import ops

    x = rnd((B, H, W, Cc), 740, 0.7) + 0.3
    xa = gb.x(x)
    with gb.vectors():
        mean, var = (ops.bn_batch_stats_images if images else ops.bn_batch_stats)(xa)
    gb.finish(ws=1)
    written(mean, var)
    assert mean.numel() == (B if images else 1) * Cc
    check_stats(xa.torch(), mean, var, images)


@pytest.mark.parametrize("B,H,W", [(1, 7, 9), (1, 8, 8), (3, 5, 13), (1, 181, 183)])
def test_instnorm_tanh_statistics_of_a_one_channel_image(gb, B, H, W):
    from emdenoise import ops

    x = rnd((B, H, W, 1), 741, 0.7) + 0.3
    xd, out = gb.v(x), gb.out((B, H, W, 1))
    with gb.vectors():
        ops.instnorm_tanh(xd, out)
    gb.finish(ws=1)
    written(out)
    x64 = x.astype(np.float64)
    ref = np.tanh((x64 - x64.mean((1, 2, 3), keepdims=True)) / np.sqrt(x64.var((1, 2, 3), keepdims=True) + 1e-3))
    show("instnorm_tanh", y=(rel_l2(out.cpu().numpy(), ref), 5e-6))       # the bar of tests/test_g_graph.py


# ------------------------------------------------------------------------------------------------ reverse reductions
def bn_reference(r, g1, b1, g2, b2, dy, mask, images, double):
    """float64 autograd through [BN1] -> BN2 -> mask with batch (or per-image) statistics -> (dr, dg1, dg2, db2, y, z)."""
    rl, l1, lb1, l2, lb2 = leaf(r), leaf(g1), leaf(b1), leaf(g2), leaf(b2)
    zs = []
    for b in (range(r.shape[0]) if images else [slice(None)]):
        rb = rl[b:b + 1] if images else rl
        zs.append(_bn_train_t(_bn_train_t(rb, l1, lb1) if double else rb, l2, lb2))
    z = torch.cat(zs)
    y = torch.clamp(z, 0.0, 6.0) if mask else z
    if mask == 2:
        y = torch.clamp(y, 0.0, 1.0)
    gr, gg1, gg2, gb2 = torch.autograd.grad(y, (rl, l1, l2, lb2), t64(dy) if not torch.is_tensor(dy) else dy, allow_unused=True)
    return gr.numpy(), None if gg1 is None else gg1.numpy(), gg2.numpy(), gb2.numpy(), y.detach().numpy(), z.detach().numpy()


def bn_params(Cc, mask, seed):
    return (rnd((Cc,), seed, 0.3) + 1.0, rnd((Cc,), seed + 1, 0.3), rnd((Cc,), seed + 2, 0.3) + 1.2,
            rnd((Cc,), seed + 3, 0.5) + (0.4 if mask == 2 else 1.0))


KINK_MARGIN = 1e-5      # 20 ulp of 6.0: the float32 forward's z is within a few ulp of the float64 one


def off_the_kinks(z, mask):
    """The float32 forward and the float64 reference pick the same mask where no unit sits within float32 rounding of a kink."""
    kinks = ((0.0, 6.0) + ((1.0,) if mask == 2 else ())) if mask else ()
    return all(float(np.abs(z - k).min()) > KINK_MARGIN for k in kinks)


def bn_case(shape, mask, images, double, seed, dy_of=None):
    """-> (r, (g1, b1, g2, b2), dy, bn_reference's tuple) for the first seed of seed, seed + 1000, ... whose float64 forward keeps every
    unit KINK_MARGIN away from the kinks of the mask (one unit on a kink is a unit-sized difference in the gradient for ANY two
    implementations; among 10^5 units most seeds have one).  dy_of(seed): the incoming gradient where it is not plain noise."""
    Cc = shape[-1]
    for k in range(32):
        s = seed + 1000 * k
        r = rnd(shape, s, 1.5) + 0.7
        dy = dy_of(s) if dy_of else rnd(shape, s + 1)
        par = bn_params(Cc, mask, s + 2)
        ref = bn_reference(r, *par, dy, mask, images, double)
        if off_the_kinks(ref[5], mask):
            return r, par, dy, ref
    raise AssertionError("no seed keeps the units off the kinks")


def check_bn_grads(tag, dr, dg1, dg2, db2, ref):
    gr, gg1, gg2, gb2 = ref[:4]
    figs = dict(dr=(rel_l2(dr, gr), TOL_BN), dgamma2=(rel_l2(dg2.cpu().numpy(), gg2), TOL_BN), dbeta2=(rel_l2(db2.cpu().numpy(), gb2), TOL_BN))
    if dg1 is not None:     # d gamma1 is eps-suppressed: held to 2e-5 of d gamma2's scale (tests/test_train_ops_gpu.py)
        figs["dgamma1"] = (float(np.abs(dg1.cpu().numpy() - gg1).max() / np.abs(gg2).max()), 2e-5)
    show(tag, **figs)


@pytest.mark.parametrize("fused", [True, False], ids=["prep-in-reduce", "prep-apart"])
@pytest.mark.parametrize("mask", [0, 1, 2])
@pytest.mark.parametrize("double", [False, True], ids=["bn", "bn2"])
@pytest.mark.parametrize("images", [False, True], ids=["batch", "images"])
@pytest.mark.parametrize("B,H,W,Cc", [(3, 5, 13, 36), (2, 127, 64, 8)])
def test_bn_backward(gb, B, H, W, Cc, images, double, mask, fused):
    """fused: the per-channel step inside the reduction's final kernel (emd_bn_bwd_reduce_prep_f32, what training runs) or as a launch
    of its own behind emd_bn_bwd_reduce[_images]_f32 (emd_bn_bwd_prep[_images]_f32)."""
    from emdenoise import ops, train_ops as TO

    gb.mp.setattr(TO, "FUSE_PREP", fused)
    r, (g1, b1, g2, b2), dy, ref = bn_case((B, H, W, Cc), mask, images, double, 750)
    ra, dya, dr = gb.x(r, name="r"), gb.x(dy, name="dy"), gb.y(B, H, W, Cc, name="dr")
    dg1, dg2, db2 = (gb.v(np.zeros(Cc, np.float32), name=n) for n in ("dgamma1", "dgamma2", "dbeta2"))
    G1, B1, G2, B2 = (gb.v(a) for a in (g1, b1, g2, b2))
    npix = H * W if images else B * H * W
    with gb.vectors():
        mean, var = (ops.bn_batch_stats_images if images else ops.bn_batch_stats)(ra)
        fold = TO.bn_train_fold(mean, var, G2, B2, npix, gamma1=G1 if double else None, beta1=B1 if double else None, images=B if images else 0)
        TO.bn_backward(dya, ra, fold, G2, dg2, db2, dr, mask=mask, gamma1=G1 if double else None, dgamma1=dg1 if double else None)
    gb.finish(ws=2)
    written(dr.torch(), *(fold[k] for k in ("scale", "shift", "rstd1", "rstd2")))
    check_bn_grads("bn_backward", dr.torch().cpu().numpy(), dg1 if double else None, dg2, db2, ref)


@pytest.mark.parametrize("images", [False, True], ids=["batch", "images"])
def test_bn_backward_of_the_cout1_gradient(gb, images):
    """bn_backward on a Cout1Grad at (1, 5, 13, 36) (and two images of it): the gradient is formed from the 1-channel image in both passes."""
    from emdenoise import ops, train_ops as TO
    from oracle import tf_ops as T

    B, H, W, Cc, mask = (2 if images else 1), 5, 13, 36, 1
    g1img, w9 = rnd((B, H, W, 1), 761), rnd((3, 3, Cc, 1), 762, 0.3)
    xl = leaf(np.zeros((B, H, W, Cc), np.float32))
    (dy,) = torch.autograd.grad(T.depthwise_conv2d_t(xl, t64(w9)).sum(-1, keepdim=True), xl, t64(g1img))     # the conv to one channel's data gradient
    r, (g1, b1, g2, b2), _, ref = bn_case((B, H, W, Cc), mask, images, True, 760, dy_of=lambda s: dy)
    ra, dr = gb.x(r, name="r"), gb.y(B, H, W, Cc, name="dr")
    dg1, dg2, db2 = (gb.v(np.zeros(Cc, np.float32)) for _ in range(3))
    G1, B1, G2, B2 = (gb.v(a) for a in (g1, b1, g2, b2))
    with gb.vectors():
        mean, var = (ops.bn_batch_stats_images if images else ops.bn_batch_stats)(ra)
        fold = TO.bn_train_fold(mean, var, G2, B2, H * W if images else B * H * W, gamma1=G1, beta1=B1, images=B if images else 0)
        TO.bn_backward(TO.Cout1Grad(gb.v(g1img), gb.v(w9.reshape(9, Cc))), ra, fold, G2, dg2, db2, dr, mask=mask, gamma1=G1, dgamma1=dg1)
    gb.finish(ws=2)
    written(dr.torch())
    check_bn_grads("cout1", dr.torch().cpu().numpy(), dg1, dg2, db2, ref)


def test_bias_gradient_reduction_accumulates(gb):
    from emdenoise import train_ops as TO

    dy = rnd((3, 5, 13, 36), 770)
    s1 = gb.v(np.full(36, 1.0, np.float32))
    TO.chan_reduce(gb.x(dy), s1, accumulate_s1=True)
    gb.finish(ws=1)
    show("chan_reduce", s1=(rel_l2(s1.cpu().numpy(), 1.0 + dy.astype(np.float64).sum(axis=(0, 1, 2))), 1e-6))


DW_BN = [
    # B, H, W, C, stride, rate
    (1, 9, 17, 36, 1, 1),      # rolling form: 8-row strips, 2 x 2 slabs
    (2, 70, 33, 8, 1, 1),      # 16-row strips, 5 x 3 per image
    (1, 23, 23, 36, 2, 1),     # gather form at stride 2: 529 pixels, two slabs
    (1, 23, 23, 8, 1, 2),      # ... at rate 2
]


@pytest.mark.parametrize("fused", [True, False], ids=["prep-in-reduce", "prep-apart"])
@pytest.mark.parametrize("wg", [False, True], ids=["dr-only", "wgrad"])
@pytest.mark.parametrize("images", [False, True], ids=["batch", "images"])
@pytest.mark.parametrize("B,H,W,Cc,stride,rate", DW_BN)
def test_bn_backward_dw(gb, B, H, W, Cc, stride, rate, images, wg, fused):
    """r -> [BN1] -> BN2 -> relu6 -> depthwise 3x3 (the consumer) -> dd: dr, the norm's parameter gradients and (wg) the consumer's
    weight gradient, against float64 autograd through the whole chain."""
    from emdenoise import ops, train_ops as TO
    from oracle import tf_ops as T

    gb.mp.setattr(TO, "FUSE_PREP", fused)
    double = Cc == 36
    Ho, Wo = -(-H // stride), -(-W // stride)
    dd, w0 = rnd((B, Ho, Wo, Cc), 781), rnd((3, 3, Cc, 1), 782, 0.3)
    # the data gradient of the consumer is linear in dd: formed once in float64, then the norm's backward as everywhere in this file
    xl, wl = leaf(np.zeros((B, H, W, Cc), np.float32)), leaf(w0)
    (dy,) = torch.autograd.grad(T.depthwise_conv2d_t(xl, t64(w0), stride, rate), xl, t64(dd))
    r, (g1, b1, g2, b2), _, ref = bn_case((B, H, W, Cc), 1, images, double, 780, dy_of=lambda s: dy)
    (gw,) = torch.autograd.grad(T.depthwise_conv2d_t(t64(ref[4]), wl, stride, rate), wl, t64(dd))
    ra, dda, dr = gb.x(r, name="r"), gb.x(dd, name="dd"), gb.y(B, H, W, Cc, name="dr")
    dg1, dg2, db2 = (gb.v(np.zeros(Cc, np.float32)) for _ in range(3))
    gdw = gb.v(np.zeros((9, Cc), np.float32), name="gdw") if wg else None
    G1, B1, G2, B2 = (gb.v(a) for a in (g1, b1, g2, b2))
    wf = gb.v(np.ascontiguousarray(w0.reshape(9, Cc)[::-1]), name="flipped taps")
    with gb.vectors():
        mean, var = (ops.bn_batch_stats_images if images else ops.bn_batch_stats)(ra)
        fold = TO.bn_train_fold(mean, var, G2, B2, H * W if images else B * H * W, gamma1=G1 if double else None, beta1=B1 if double else None,
                                images=B if images else 0)
        TO.bn_backward_dw(TO.DwGrad(dda, wf, gdw, stride=stride, rate=rate, hw=(H, W)), ra, fold, G2, dg2, db2, dr, mask=TO.MASK_RELU6,
                          gamma1=G1 if double else None, dgamma1=dg1 if double else None)
    gb.finish(ws=2)
    written(dr.torch())
    check_bn_grads("bn_backward_dw", dr.torch().cpu().numpy(), dg1 if double else None, dg2, db2, ref)
    if wg:
        show("consumer", dW=(rel_l2(gdw.cpu().numpy().reshape(3, 3, Cc, 1), gw.numpy()), TOL_WGRAD))


@pytest.mark.parametrize("double,mask", [(True, 1), (False, 2), (False, 0)])
def test_bn_small(gb, double, mask):
    """emd_bn_train_fwd_small_f32 / _bwd_small_f32 at (3, 5, 7, 36): per-image statistics, one launch each way."""
    from emdenoise import ops, train_ops as TO

    B, H, W, Cc = 3, 5, 7, 36
    r, (g1, b1, g2, b2), dy, ref = bn_case((B, H, W, Cc), mask, True, double, 790)
    ra, dya, y, dr = gb.x(r, name="r"), gb.x(dy, name="dy"), gb.y(B, H, W, Cc, name="y"), gb.y(B, H, W, Cc, name="dr")
    assert TO.bn_small_supported(ra)
    dg1, dg2, db2 = (gb.v(np.zeros(Cc, np.float32)) for _ in range(3))
    G1, B1, G2, B2 = (gb.v(a) for a in (g1, b1, g2, b2))
    mv = [gb.v(a) for a in (np.zeros(Cc, np.float32), np.ones(Cc, np.float32)) * (2 if double else 1)]
    act = {0: ops.ACT_NONE, 1: ops.ACT_RELU6, 2: ops.ACT_RELU6_CLIP01}[mask]
    with gb.vectors():
        fold = TO.bn_train_fwd_small(ra, G2, B2, y, act, gamma1=G1 if double else None, beta1=B1 if double else None, moving=mv)
        TO.bn_backward_small(dya, ra, fold, G2, dg2, db2, dr, mask=mask, gamma1=G1 if double else None, dgamma1=dg1 if double else None)
    gb.finish()
    written(y.torch(), dr.torch(), *(fold[k] for k in ("scale", "shift", "rstd1", "rstd2", "mean")))
    show("bn_small forward", y=(rel_l2(y.torch().cpu().numpy(), ref[4]), 3e-6))       # the affine's bar in test_bn_train_forward_and_backward
    check_bn_grads("bn_small backward", dr.torch().cpu().numpy(), dg1 if double else None, dg2, db2, ref)


@pytest.mark.parametrize("n", [5, 300001])
def test_denoise_loss_and_sumsq(gb, n):
    from emdenoise import train_ops as TO

    truth = rnd((n,), 800, 0.2, positive=True)
    out = leaf(truth + rnd((n,), 801, 0.01))
    mse = ((out - t64(truth)) ** 2).mean()
    loss = 1000.0 * mse if float(mse.detach()) < 0.001 else torch.sqrt(1000.0 * mse)
    (ref,) = torch.autograd.grad(loss, out)
    dout = gb.out((n,), name="dout")
    x = gb.v(rnd((n,), 802))
    with gb.vectors():
        res = TO.denoise_loss(gb.v(out.detach().numpy().astype(np.float32)), gb.v(truth), dout)
        ss = TO.sumsq(x, scale=0.5)
    gb.finish(ws=2)
    written(dout, res, ss)
    res = res.cpu().numpy()
    show("denoise_loss", mse=(abs(res[0] - float(mse)) / float(mse), 1e-6), loss=(abs(res[1] - float(loss)) / float(loss), 2e-6),
         dout=(rel_l2(dout.cpu().numpy(), ref.numpy()), 2e-6))
    want = float((0.25 * x.double().cpu().numpy() ** 2).sum())
    show("sumsq", sumsq=(abs(float(ss[0]) - want) / want, TOL_F32))      # double accumulation, one rounding to float: 6e-8


# ------------------------------------------------------------------------------------------------ output-only entry points
@pytest.mark.parametrize("base", [False, True], ids=["zero", "base"])
@pytest.mark.parametrize("B,H,W,ci,co,k,stride,rate", [
    (2, 9, 13, 4, 24, 1, 1, 1),         # the K = 4 kernel: a slab tail, a column tail
    (1, 7, 9, 256, 728, 1, 2, 1),       # strided, odd sizes, N tail
    (2, 10, 6, 64, 64, 3, 2, 1),
    (1, 16, 16, 128, 64, 3, 1, 6),
])
def test_conv_wgrad(gb, B, H, W, ci, co, k, stride, rate, base):
    from emdenoise import train_ops as TO
    from oracle import tf_ops as T

    x, w = rnd((B, H, W, ci), 1), leaf(rnd((k, k, ci, co), 2, 0.1))
    Ho, Wo = -(-H // stride), -(-W // stride)
    dy = rnd((B, Ho, Wo, co), 3)
    (ref,) = torch.autograd.grad(T.conv2d_t(t64(x), w, None, stride=stride, rate=rate), w, t64(dy))
    b0 = rnd((k * k, ci, co), 4) * float(ref.abs().mean()) if base else np.zeros((k * k, ci, co), np.float32)
    dw = gb.v(b0, name="dw")
    tdy, tdx = ([0], [0]) if k == 1 else TO.conv_taps(H, W, stride, rate)
    TO.conv_wgrad(gb.x(x, name="a"), gb.x(dy, name="dy"), dw, tdy, tdx, sa=stride)
    gb.finish()
    show("conv_wgrad", dW=(rel_l2(dw.cpu().numpy().reshape(k, k, ci, co).astype(np.float64) - b0.reshape(k, k, ci, co), ref.numpy()), TOL_WGRAD))


def test_deconv_wgrad_and_dgrad(gb):
    from emdenoise import ops, train_ops as TO
    from oracle import tf_ops as T

    B, H, W, ci, co = 2, 5, 7, 64, 64
    x, w = leaf(rnd((B, H, W, ci), 6)), leaf(rnd((3, 3, co, ci), 7, 0.1))
    dy = rnd((B, 2 * H, 2 * W, co), 8)
    gx, gw = torch.autograd.grad(T.conv2d_transpose_s2_t(x, w, None), (x, w), t64(dy))
    dw = gb.v(np.zeros((9, co, ci), np.float32), name="dw")
    tdy, tdx = TO.conv_taps(2 * H, 2 * W, 2, 1)
    dya = gb.x(dy, name="dy")
    TO.conv_wgrad(dya, gb.x(x.detach().numpy().astype(np.float32), name="x"), dw, tdy, tdx, sa=2)
    pk = guarded_pack(gb, 9, co, ci).pack(gb.v(w.detach().numpy().reshape(9, co, ci).astype(np.float32)), 9, cout_major=False)
    dx = gb.y(B, H, W, ci, name="dx")
    ops.conv3x3(dya, pk, gb.v(np.ones(ci, np.float32)), gb.v(np.zeros(ci, np.float32)), dx, stride=2, act=False)
    gb.finish()
    written(dx.torch(), pk.hi, pk.lo)
    show("deconv", dW=(rel_l2(dw.cpu().numpy().reshape(3, 3, co, ci), gw.numpy()), TOL_WGRAD), dx=(rel_l2(dx.torch().cpu().numpy(), gx.numpy()), TOL_X3))


def guarded_pack(gb, taps, cin, cout):
    """A DevPackedWeights whose hi / lo planes are guarded int16 views."""
    from emdenoise import train_ops as TO

    p = TO.DevPackedWeights(taps, cin, cout, dev())
    n = p.hi.numel()
    p.hi, p.lo = gb.out((n,), torch.int16, name="hi plane"), gb.out((n,), torch.int16, name="lo plane")
    return p


def test_conv1x1_s2_bwd_data_accumulates_into_a_slice(gb):
    from emdenoise import train_ops as TO
    from oracle import tf_ops as T

    B, H, W, ci, co = 1, 7, 9, 256, 728
    x, w = leaf(rnd((B, H, W, ci), 11)), rnd((1, 1, ci, co), 12, 0.1)
    dy = rnd((B, 4, 5, co), 13)
    (ref,) = torch.autograd.grad(T.conv2d_t(x, t64(w), None, stride=2), x, t64(dy))
    pk = guarded_pack(gb, 1, co, ci).pack(gb.v(w.reshape(1, ci, co)), 1, cout_major=True, tap_sel=[0])
    base = rnd((B, H, W, ci), 14)
    dx = gb.y(B, H, W, ci, fill=base, name="dx")
    TO.conv1x1_s2_bwd_data(gb.x(dy, name="dy"), pk, gb.v(np.ones(ci, np.float32)), gb.v(np.zeros(ci, np.float32)), dx, accumulate=True)
    gb.finish()
    show("conv1x1_s2_bwd_data", dx=(rel_l2(dx.torch().cpu().numpy().astype(np.float64) - base, ref.numpy()), TOL_X3))


@pytest.mark.parametrize("taps,ci,co", [(1, 728, 728), (1, 4, 24), (9, 4, 24)])
def test_device_pack_equals_the_host_pack(gb, taps, ci, co):
    """DevPackedWeights.pack and PackBatch (one launch for a job table) with K and N tails, both orientations, into guarded planes."""
    from emdenoise import ops, train_ops as TO

    pb, want, got = TO.PackBatch(dev()), [], []
    for cm in (False, True):
        w = rnd((taps, co, ci) if cm else (taps, ci, co), 20 + cm)
        host = ops.PackedWeights(w, cm, dev())
        wd = gb.v(w)
        single = guarded_pack(gb, taps, ci, co).pack(wd, taps, cout_major=cm)
        batched = guarded_pack(gb, taps, ci, co)
        pb.add(batched, wd, taps, cout_major=cm)
        want += [host, host]
        got += [single, batched]
    pb.run()
    gb.finish()
    for a, b in zip(want, got):
        written(b.hi, b.lo)
        assert torch.equal(a.hi, b.hi) and torch.equal(a.lo, b.lo)


@pytest.mark.parametrize("B,H,W,Cc,stride", [(1, 13, 9, 36, 1), (2, 9, 7, 8, 2), (1, 70, 33, 8, 1)])
def test_dw3x3_gradients(gb, B, H, W, Cc, stride):
    """dw3x3_wgrad, dw3x3_bwd_data, dw3x3_bwd_both (stride 1) and dw3x3_wgrad_pre against float64 autograd of the depthwise conv."""
    from emdenoise import ops, train_ops as TO
    from oracle import tf_ops as T

    x, w, dy, gx, gw = dw3x3_reference(B, H, W, Cc, stride, 1)
    xa, dya = gb.x(x, name="x"), gb.x(dy, name="dy")
    dw, dx = gb.v(np.zeros((9, Cc), np.float32), name="dw"), gb.y(B, H, W, Cc, name="dx")
    TO.dw3x3_wgrad(xa, dya, dw, stride=stride)
    wdev = gb.v(w.reshape(9, Cc))
    TO.dw3x3_bwd_data(dya, wdev, dx, stride=stride)
    figs = {}
    if stride == 1:
        dw2, dx2 = gb.v(np.zeros((9, Cc), np.float32), name="dw (both)"), gb.y(B, H, W, Cc, name="dx (both)")
        TO.dw3x3_bwd_both(dya, gb.v(np.ascontiguousarray(w.reshape(9, Cc)[::-1])), xa, dx2, dw2)
    # the never-written input: x = relu6(r * scale + shift)
    r, sc, sh = rnd((B, H, W, Cc), 30, 2.0), rnd((Cc,), 31, 0.2) + 1.0, rnd((Cc,), 32, 0.5) + 1.0
    xp = np.clip(r.astype(np.float64) * sc + sh, 0.0, 6.0)
    wl = leaf(w)
    (gwp,) = torch.autograd.grad(T.depthwise_conv2d_t(t64(xp), wl, stride, 1), wl, t64(dy))
    dw3 = gb.v(np.zeros((9, Cc), np.float32), name="dw (pre)")
    TO.dw3x3_wgrad_pre(ops.PreAct(gb.x(r, name="r"), gb.v(sc), gb.v(sh), act=ops.ACT_RELU6), dya, dw3, stride=stride)
    gb.finish()
    written(dx.torch())
    sh4 = (3, 3, Cc, 1)
    figs = dict(dW=(rel_l2(dw.cpu().numpy().reshape(sh4), gw), TOL_WGRAD), dx=(rel_l2(dx.torch().cpu().numpy(), gx), TOL_F32),
                dW_pre=(rel_l2(dw3.cpu().numpy().reshape(sh4), gwp.numpy()), TOL_WGRAD))
    if stride == 1:
        written(dx2.torch())
        figs.update(dW_both=(rel_l2(dw2.cpu().numpy().reshape(sh4), gw), TOL_WGRAD), dx_both=(rel_l2(dx2.torch().cpu().numpy(), gx), TOL_F32))
    show("dw3x3", **figs)


def test_conv3x3_cout1_gradients(gb):
    from emdenoise import train_ops as TO
    from oracle import tf_ops as T

    B, H, W, ci = 1, 5, 7, 36
    x, w = leaf(rnd((B, H, W, ci), 18)), leaf(rnd((3, 3, ci, 1), 19, 0.1))
    dy = rnd((B, H, W, 1), 20)
    gx, gw = torch.autograd.grad(T.depthwise_conv2d_t(x, w).sum(-1, keepdim=True), (x, w), t64(dy))
    dw, dx, dyd = gb.v(np.zeros((9, ci), np.float32), name="dw"), gb.y(B, H, W, ci, name="dx"), gb.v(dy)
    TO.conv3x3_cout1_wgrad(gb.x(x.detach().numpy().astype(np.float32)), dyd, dw)
    TO.conv3x3_cout1_bwd_data(dyd, gb.v(w.detach().numpy().reshape(9, ci).astype(np.float32)), dx)
    gb.finish()
    written(dx.torch())
    show("conv3x3_cout1", dW=(rel_l2(dw.cpu().numpy().reshape(3, 3, ci, 1), gw.numpy()), TOL_WGRAD), dx=(rel_l2(dx.torch().cpu().numpy(), gx.numpy()), TOL_F32))


def test_resize_bilinear_backward(gb):
    from emdenoise import train_ops as TO
    from oracle import tf_ops as T

    x, dy = leaf(rnd((2, 3, 5, 36), 21)), rnd((2, 12, 20, 36), 22)
    (ref,) = torch.autograd.grad(T.resize_bilinear_legacy_t(x, 12, 20), x, t64(dy))
    dx = TO.resize_bilinear_bwd(gb.x(dy), gb.y(2, 3, 5, 36))
    gb.finish()
    written(dx.torch())
    show("resize_bilinear_bwd", dx=(rel_l2(dx.torch().cpu().numpy(), ref.numpy()), TOL_F32))


@pytest.mark.parametrize("H,W", [(7, 5), (1, 1)])
def test_avgpool2x2_backward(gb, H, W):
    from emdenoise import train_ops as TO
    from oracle import tf_ops as T

    x, dy = leaf(rnd((2, H, W, 36), 23)), rnd((2, -(-H // 2), -(-W // 2), 36), 24)
    (ref,) = torch.autograd.grad(T.avg_pool2x2_same_t(x), x, t64(dy))
    dx = TO.avgpool2x2_bwd(gb.x(dy), gb.y(2, H, W, 36))
    gb.finish()
    written(dx.torch())
    show("avgpool2x2_bwd", dx=(rel_l2(dx.torch().cpu().numpy(), ref.numpy()), TOL_F32))


ODD = [5, 1003, 70001]      # no multiple of 4, 64 or 256; 70 001 = several workgroups and a tail


def test_axpy(gb):
    from emdenoise import train_ops as TO

    x, y = rnd((1, 3, 7, 36), 25), rnd((1, 3, 7, 36), 26)
    ya = gb.y(1, 3, 7, 36, fill=y)
    TO.axpy(gb.x(x), ya, alpha=0.5)
    gb.finish()
    show("axpy", y=(rel_l2(ya.torch().cpu().numpy(), y + 0.5 * x.astype(np.float64)), 1e-7))


@pytest.mark.parametrize("n", ODD)
def test_optimizer_steps(gb, n):
    """nesterov_step (ApplyMomentum, use_nesterov) and adam_step (with the global-norm clip) on vectors of odd lengths."""
    from emdenoise import train_ops as TO
    from oracle import gan_graph as GG

    p, g, a = (rnd((n,), s).astype(np.float64) for s in (36, 37, 38))
    lr, mom, gs = 0.001, 0.9, 0.1
    pd, gd, ad = gb.v(p.astype(np.float32)), gb.v(g.astype(np.float32)), gb.v(a.astype(np.float32))
    TO.nesterov_step(pd, gd, ad, lr, mom, gs)
    a2 = mom * a + g * gs
    p2 = p - (g * gs * lr + a2 * mom * lr)
    # Adam, step 3, gradient norm above the clip
    m, v = np.abs(rnd((n,), 39, 0.1)).astype(np.float64), np.abs(rnd((n,), 40, 0.01)).astype(np.float64)
    gn2, clip = float((g * g).sum()), 0.5 * float(np.sqrt((g * g).sum()))
    q = (p * 1e-3).astype(np.float32)      # small parameters: their float32 rounding (2^-24 |q|) stays 5e-6 of the update (1.25e-5)
    pa, ma, va = gb.v(q), gb.v(m.astype(np.float32)), gb.v(v.astype(np.float32))
    TO.adam_step(pa, gd, ma, va, 3, 2e-4, gnorm_sq=gb.v(np.array([gn2], np.float32)), clip_norm=clip)
    gb.finish()
    newp, newm, newv = GG.adam_step({"w": q.astype(np.float64)}, {"w": g * 0.5}, {"w": m}, {"w": v}, 3, 2e-4)
    show("nesterov", accum=(rel_l2(ad.cpu().numpy(), a2), 1e-6), param=(rel_l2(pd.cpu().numpy(), p2), 1e-6))
    show("adam", m=(rel_l2(ma.cpu().numpy(), newm["w"]), 1e-6), v=(rel_l2(va.cpu().numpy(), newv["w"]), 1e-6),
         update=(rel_l2(pa.cpu().numpy().astype(np.float64) - q, newp["w"] - q), 2e-5))


# ------------------------------------------------------------------------------------------------ graph G's training operations
@pytest.mark.parametrize("B,H,W,Cc,stride", [(1, 9, 7, 36, 1), (2, 7, 5, 8, 2)])
def test_dw3x3_reflect_gradients(gb, B, H, W, Cc, stride):
    from emdenoise import train_ops as TO
    from tests.test_gan_train_gpu import dw_reflect_reference

    x, w, dy, gx, gw = dw_reflect_reference(B, H, W, Cc, stride)
    dya, dw, dx = gb.x(dy, name="dy"), gb.v(np.zeros((9, Cc), np.float32), name="dw"), gb.y(B, H, W, Cc, name="dx")
    TO.dw3x3_reflect_wgrad(gb.x(x, name="x"), dya, dw, stride=stride)
    TO.dw3x3_reflect_bwd_data(dya, gb.v(w.reshape(9, Cc)), dx, stride=stride)
    gb.finish()
    written(dx.torch())
    show("dw3x3_reflect", dW=(rel_l2(dw.cpu().numpy().reshape(3, 3, Cc, 1), gw), TOL_WGRAD), dx=(rel_l2(dx.torch().cpu().numpy(), gx), TOL_F32))


def test_first_and_last_layer_of_the_generator(gb):
    """conv3x3_cout1_reflect_wgrad / _bwd_data at (1, 5, 7, 36); dw7_c1_reflect and its weight gradient at (1, 9, 11)."""
    from emdenoise import train_ops as TO
    from tests.test_gan_train_gpu import cout1_reference, dw7_reference

    B, H, W, Cc = 1, 5, 7, 36
    x, w, dyl, gx, gwl = cout1_reference(B, H, W, Cc)
    dwl, dx, dyd = gb.v(np.zeros((9, Cc), np.float32), name="dw"), gb.y(B, H, W, Cc, name="dx"), gb.v(dyl)
    TO.conv3x3_cout1_reflect_wgrad(gb.x(x), dyd, dwl)
    TO.conv3x3_cout1_reflect_bwd_data(dyd, gb.v(w.reshape(9, Cc)), dx)
    H7, W7 = 9, 11
    x7, w7, dd, y7, gw7 = dw7_reference(1, H7, W7)
    xd, d4 = gb.v(x7), gb.y(1, H7, W7, 4, pitch=False, name="d4")       # emd_dw7_c1_reflect_f32 takes no pitch: d4 is dense
    TO.dw7_c1_reflect(xd, gb.v(w7.reshape(49)), d4)
    dd4 = np.zeros((1, H7, W7, 4), np.float32)
    dd4[..., 0:1] = dd
    dw49 = gb.v(np.zeros(49, np.float32), name="dw49")
    TO.dw7_c1_reflect_wgrad(xd, gb.x(dd4, pitch=False), dw49)
    gb.finish()
    written(dx.torch(), d4.torch())
    got = d4.torch().cpu().numpy()
    assert np.all(got[..., 1:] == 0)
    show("generator ends", dW=(rel_l2(dwl.cpu().numpy().reshape(3, 3, Cc, 1), gwl), TOL_WGRAD), dx=(rel_l2(dx.torch().cpu().numpy(), gx), TOL_F32),
         d4=(rel_l2(got[..., 0:1], y7), TOL_F32), dW49=(rel_l2(dw49.cpu().numpy().reshape(7, 7, 1, 1), gw7), TOL_WGRAD))


def test_tanh_l1_feature_and_crop_scatter(gb):
    from emdenoise import train_ops as TO
    from oracle import gan_graph as GG

    n = 1003
    y, dyt = np.tanh(rnd((n,), 17)), rnd((n,), 18)
    with gb.vectors():
        g = TO.tanh_bwd(gb.v(dyt), gb.v(y))
    a, b, base = rnd((n,), 10), rnd((n,), 11), rnd((n,), 12)
    at = leaf(a)
    loss = 12.0 * (at - t64(b)).abs().mean()
    (ga,) = torch.autograd.grad(loss, at)
    dy, acc, dy2 = gb.v(base, name="dy"), gb.v(np.zeros(1, np.float32), name="loss"), gb.out((n,), name="dy (overwritten)")
    TO.l1_feature(gb.v(a), gb.v(b), 12.0, dy, True, acc)
    TO.l1_feature(gb.v(a), gb.v(b), 12.0, dy2, False, acc)
    # one crop of 5 x 5 from the padded 12 x 12 image (padding 9), at an offset that mirrors on both axes
    S, nc, y0, x0 = 12, 5, 2, 17
    img = leaf(rnd((1, S, S, 1), 13))
    ridx = torch.from_numpy(GG.reflect_indices(S, (3 * S) // 4))
    gcrop = rnd((1, nc, nc, 1), 14)
    (gi,) = torch.autograd.grad((img[:, ridx][:, :, ridx][:, y0:y0 + nc, x0:x0 + nc] * t64(gcrop)).sum(), img)
    g4 = np.zeros((1, nc, nc, 4), np.float32)
    g4[..., 0:1] = gcrop
    crop = gb.x(g4, name="crop gradient")
    dimg = gb.v(np.zeros((1, S, S, 1), np.float32), name="dimg")
    TO.crop_scatter(crop.torch(), crop.ld, dimg, y0, x0, nc, S)
    gb.finish()
    written(g, dy2)
    show("tanh_bwd", g=(rel_l2(g.cpu().numpy(), dyt * (1 - y.astype(np.float64) ** 2)), 1e-6))
    show("l1_feature", loss=(abs(float(acc[0]) - 2 * float(loss)) / (2 * float(loss)), 1e-5), dy=(rel_l2(dy.cpu().numpy() - base, ga.numpy()), 1e-5),
         dy2=(rel_l2(dy2.cpu().numpy(), ga.numpy()), 1e-5))
    show("crop_scatter", dimg=(rel_l2(dimg.cpu().numpy(), gi.numpy()), TOL_F32))


def test_gan_head_fc_row_and_bcast_rows(gb):
    from emdenoise import train_ops as TO

    figs = {}
    for mode, label in ((0, 0.95), (0, 0.05), (1, 0.0)):
        l3 = leaf(np.array([0.3, -0.2, 0.7], np.float32))
        out = torch.sigmoid(l3.max())
        loss = -torch.log(torch.clamp(1 - (label - out).abs(), 1e-8, 1 - 1e-8)) if mode == 0 else -torch.log(torch.clamp(out, 1e-8, 1.0))
        (gl,) = torch.autograd.grad(loss, l3)
        with gb.vectors():
            res, dl = TO.gan_head(gb.v(l3.detach().numpy().astype(np.float32)), label, mode, grad_scale=0.5)
        gb.finish()
        written(res, dl)
        figs[f"head{mode}_{label}"] = (max(abs(float(res[0]) - float(out)) / float(out), abs(float(res[1]) - float(loss)) / float(loss),
                                           rel_l2(dl.cpu().numpy(), 0.5 * gl.numpy())), TOL_F32)
    K = 1003
    x, w, base = rnd((K,), 50), rnd((K,), 51), rnd((K,), 52)
    dw, db = gb.v(base, name="dw"), gb.v(np.array([0.25], np.float32), name="db")
    with gb.vectors():
        dx = TO.fc_row_bwd(gb.v(x), gb.v(w), gb.v(np.array([0.7], np.float32)), dw, db)
    v = rnd((36,), 53)
    rows = TO.bcast_rows(gb.v(v), gb.y(2, 3, 5, 36, name="rows"), 0.125)
    gb.finish()
    written(dx, rows.torch())
    f32 = np.float32
    figs.update(fc_dw=(rel_l2(dw.cpu().numpy(), base + x.astype(np.float64) * f32(0.7)), TOL_F32), fc_dx=(rel_l2(dx.cpu().numpy(), w.astype(np.float64) * f32(0.7)), TOL_F32),
                fc_db=(abs(float(db[0]) - (0.25 + float(f32(0.7)))), TOL_F32),
                bcast=(rel_l2(rows.torch().cpu().numpy(), np.broadcast_to(v.astype(np.float64) * 0.125, (2, 3, 5, 36))), TOL_F32))
    show("gan head", **figs)


def test_bn_inference_fold_and_parameter_gradients(gb):
    """bn_infer_fold2, chan_reduce with the leaky mask and bn_infer_grads at (2, 5, 7, 36): the generator's moving-statistics double norm."""
    from emdenoise import ops, train_ops as TO

    B, H, W, Cc, eps = 2, 5, 7, 36, 0.01
    r, dy = rnd((B, H, W, Cc), 60, 1.5), rnd((B, H, W, Cc), 69)
    raw = {"g1": rnd((Cc,), 61, 0.3) + 1, "b1": rnd((Cc,), 62, 0.3), "m1": rnd((Cc,), 63, 0.3), "v1": np.abs(rnd((Cc,), 64)) + 0.5,
           "g2": rnd((Cc,), 65, 0.3) + 1, "b2": rnd((Cc,), 66, 0.3), "m2": rnd((Cc,), 67, 0.3), "v2": np.abs(rnd((Cc,), 68)) + 0.5}
    P = {k: t64(v).requires_grad_(k[0] in "gb") for k, v in raw.items()}
    rt = leaf(r)
    z1 = (rt - P["m1"]) * (P["g1"] / torch.sqrt(P["v1"] + eps)) + P["b1"]
    z = (z1 - P["m2"]) * (P["g2"] / torch.sqrt(P["v2"] + eps)) + P["b2"]
    y = torch.nn.functional.leaky_relu(z, 0.2)
    assert float(z.detach().abs().min()) > 2e-5
    refs = torch.autograd.grad(y, (P["g1"], P["b1"], P["g2"], P["b2"]), t64(dy))
    dv = {k: gb.v(v) for k, v in raw.items()}
    ra, dya, ya = gb.x(r, name="r"), gb.x(dy, name="dy"), gb.y(B, H, W, Cc, name="y")
    grads = [gb.v(np.zeros(Cc, np.float32)) for _ in range(4)]
    s1, t1, t2 = (gb.out((Cc,)) for _ in range(3))
    with gb.vectors():
        f = TO.bn_infer_fold2(dv["g1"], dv["b1"], dv["m1"], dv["v1"], dv["g2"], dv["b2"], dv["m2"], dv["v2"], eps)
    ops.affine_act(ra, f["scale"], f["shift"], ya, act=ops.ACT_LEAKY)
    TO.chan_reduce(dya, s1, ra, f["mprime"], f["rprime"], t2, f["scale"], f["shift"], TO.MASK_LEAKY)
    TO.chan_reduce(dya, s1, ra, f["mean1"], f["rstd1"], t1, f["scale"], f["shift"], TO.MASK_LEAKY)
    TO.bn_infer_grads(s1, t1, t2, f["a2"], *grads)
    gb.finish(ws=2)
    written(ya.torch(), s1, t1, t2, *(f[k] for k in ("scale", "shift", "mprime", "rprime", "rstd1", "a2")))
    show("bn_infer", y=(rel_l2(ya.torch().cpu().numpy(), y.detach().numpy()), TOL_F32),
         **{n: (rel_l2(got.cpu().numpy(), ref.numpy()), 2e-5) for n, got, ref in zip(("dg1", "db1", "dg2", "db2"), grads, refs)})


# ------------------------------------------------------------------------------------------------ one training step of a tower
@pytest.mark.parametrize("S,B", [(32, 1), (96, 1), (32, 3)])
def test_tower_under_guarded_workspaces(monkeypatch, S, B):
    """One step of the D' tower at the sizes where (S / 4)^2 * B is no multiple of 128 (64, 576, 192 rows into the 128-row tiles of the
    statistics epilogues), which the oracle comparisons at 64, 128 and 512 never reach: every workspace of the step comes from the
    substituted allocator; all guards intact; loss and gradients equal to the unguarded run's -- the forward bit for bit, the gradients
    within the run-to-run spread of their float atomics (1e-6, test_gradient_accumulation_run_to_run_spread)."""
    from emdenoise import ops, trainer as TR
    from tests.synth_inputs import synthetic_pair
    from tests.test_train_gpu import weights

    w = weights()
    lq, hq = synthetic_pair(B, S, S, seed=31)
    x, t = torch.from_numpy(lq).to(dev()), torch.from_numpy(hq).to(dev())

    def run():
        tr = TR.DenoiserTrainer(w, dev())
        tr.zero_grad()
        out, res = tr.tower(x, t)
        torch.cuda.synchronize()
        return out.cpu().numpy(), res.cpu().numpy(), tr.grads.detach().cpu().numpy().astype(np.float64), tr.moving.detach().cpu().numpy().copy()

    plain = run()
    ws = G.Workspaces()
    monkeypatch.setattr(ops, "workspace", ws)
    guarded_run = run()
    ws.check(at_least=10)
    sizes = sorted({g.numel * 8 for g in ws.guards})
    spread = rel_l2(guarded_run[2], plain[2])
    print(f"    tower S = {S}, B = {B}: {len(ws.guards)} guarded workspaces of {sizes[0]} .. {sizes[-1]} bytes, gradient spread {spread:.2e}")
    np.testing.assert_array_equal(guarded_run[0], plain[0])
    np.testing.assert_array_equal(guarded_run[1], plain[1])
    np.testing.assert_array_equal(guarded_run[3], plain[3])
    assert np.isfinite(guarded_run[2]).all() and spread < 1e-6
