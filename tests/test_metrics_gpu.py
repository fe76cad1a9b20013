"""GPU tests of the image-quality metrics (csrc/ssim.hip, emdenoise.metrics) against the float64 restatement
of the reference's tf_ssim / tf_ms_ssim (tests/ssim_ref.py).

Tolerances are not literals: the yardstick of every case is the float32 restatement's own distance from the float64 one on the
same inputs, computed here.  The HIP path sums in another order and applies the window as two 1-D passes, so it gets FACTOR = 4
times that distance; means and other scalars (which the kernels accumulate in double) get the same factor over the float32
restatement's scalar error with a floor of 1e-6 absolute.  Every figure is printed before it is asserted.

Figures measured on an MI355X are recorded in DESIGN.md 3.15."""
import ctypes as C

import numpy as np
import pytest
import torch

import emdenoise
from emdenoise import _lib, metrics
from tests import ssim_ref as R
from tests.synth_inputs import synthetic_pair

pytestmark = pytest.mark.gpu

FACTOR = 4.0
FLOOR = 1e-6

SHAPES = [(2, 64, 64), (3, 75, 131), (1, 11, 11), (2, 176, 176), (2, 512, 512)]


def dev():
    return torch.device("cuda", 0)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def pair(B, H, W, seed=None):
    x, y = synthetic_pair(B, H, W, seed=1000 + H + W if seed is None else seed)
    return x, y


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def check_field(name, got, ref64, ref32):
    """A map or a gradient: relative L2 against float64 within FACTOR x the float32 restatement's."""
    e, y = rel_l2(got, ref64), rel_l2(ref32, ref64)
    print(f"{name}: rel L2 {e:.3e}; float32 restatement {y:.3e}; bound {FACTOR * y:.3e}")
    assert e <= FACTOR * y, (name, e, y)


def check_scalar(name, got, ref64, ref32):
    got, ref64, ref32 = (np.asarray(v, np.float64) for v in (got, ref64, ref32))
    e, y = float(np.max(np.abs(got - ref64))), float(np.max(np.abs(ref32 - ref64)))
    bound = max(FACTOR * y, FLOOR)
    print(f"{name}: abs error {e:.3e}; float32 restatement {y:.3e}; bound {bound:.3e}")
    assert e <= bound, (name, e, y)


# ---- ssim ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ssim_maps_and_means(shape):
    B, H, W = shape
    x, y = pair(B, H, W)
    r64, r32 = R.ssim(x, y, torch.float64), R.ssim(x, y, torch.float32)
    xd, yd = up(x), up(y)
    smap, cmap = emdenoise.ssim(xd, yd, cs_map=True, mean_metric=False)
    assert smap.shape == (B, H - 10, W - 10, 1) and cmap.shape == smap.shape and smap.is_cuda
    tag = f"ssim {shape}"
    check_field(tag + " ssim_map", smap.cpu().numpy()[..., 0], r64["ssim_map"], r32["ssim_map"])
    check_field(tag + " cs_map", cmap.cpu().numpy()[..., 0], r64["cs_map"], r32["cs_map"])
    ms, mc = emdenoise.ssim(xd, yd, cs_map=True, per_image=True)
    check_scalar(tag + " per-image mean ssim", ms.cpu().numpy(), r64["means"][:, 0], r32["means"][:, 0])
    check_scalar(tag + " per-image mean cs", mc.cpu().numpy(), r64["means"][:, 1], r32["means"][:, 1])
    bs, bc = emdenoise.ssim(xd, yd, cs_map=True)
    assert bs.is_cuda and bs.dim() == 0
    check_scalar(tag + " batch mean ssim", bs.item(), r64["batch"][0], r32["batch"][0])
    check_scalar(tag + " batch mean cs", bc.item(), r64["batch"][1], r32["batch"][1])
    # the reference's name and argument list; numpy in -> float out; the means alone (no map written) are the same bits
    v = emdenoise.tf_ssim(x, y)
    assert isinstance(v, float) and np.float32(v) == np.float32(bs.item())
    only = emdenoise.ssim(xd, yd, mean_metric=False)
    assert torch.equal(only, smap)


@pytest.mark.parametrize("size", [3, 7, 11, 15])
def test_ssim_window_sizes(size):
    B, H, W = 2, 75, 131
    x, y = pair(B, H, W, seed=40 + size)
    r64, r32 = R.ssim(x, y, torch.float64, size=size), R.ssim(x, y, torch.float32, size=size)
    smap, cmap = emdenoise.ssim(up(x), up(y), cs_map=True, mean_metric=False, size=size)
    assert smap.shape == (B, H - size + 1, W - size + 1, 1)
    check_field(f"size {size} ssim_map", smap.cpu().numpy()[..., 0], r64["ssim_map"], r32["ssim_map"])
    check_field(f"size {size} cs_map", cmap.cpu().numpy()[..., 0], r64["cs_map"], r32["cs_map"])
    check_scalar(f"size {size} batch mean", emdenoise.ssim(up(x), up(y), size=size).item(), r64["batch"][0], r32["batch"][0])
    # another sigma reaches the kernel through the taps
    r64s, r32s = R.ssim(x, y, torch.float64, size=size, sigma=0.8), R.ssim(x, y, torch.float32, size=size, sigma=0.8)
    check_scalar(f"size {size} sigma 0.8 batch mean", emdenoise.ssim(up(x), up(y), size=size, sigma=0.8).item(), r64s["batch"][0],
                 r32s["batch"][0])


def test_ssim_unaligned_images_take_the_scalar_loads():
    """W % 4 == 0 but the images start 4 bytes off a 16-byte boundary: the float4 path must not be taken (and results agree)."""
    B, H, W = 2, 40, 64
    x, y = pair(B, H, W, seed=77)
    buf_x = torch.zeros(B * H * W + 1, dtype=torch.float32, device=dev())
    buf_y = torch.zeros(B * H * W + 1, dtype=torch.float32, device=dev())
    xv, yv = buf_x[1:].view(B, H, W), buf_y[1:].view(B, H, W)
    xv.copy_(up(x)[..., 0])
    yv.copy_(up(y)[..., 0])
    assert xv.data_ptr() % 16 == 4 and xv.is_contiguous()
    a = emdenoise.ssim(xv, yv, mean_metric=False)
    b = emdenoise.ssim(up(x), up(y), mean_metric=False)
    assert torch.equal(a, b)


# ---- ms-ssim -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(2, 176, 176), (2, 512, 512), (1, 203, 181)], ids=lambda s: "x".join(map(str, s)))
def test_ms_ssim(shape):
    B, H, W = shape
    x, y = pair(B, H, W)
    v64, s64, c64 = R.ms_ssim(x, y, torch.float64)
    v32, s32, c32 = R.ms_ssim(x, y, torch.float32)
    assert (c64 > 0).all()                      # the fractional powers are defined
    v, lm = emdenoise.ms_ssim(up(x), up(y), return_levels=True)
    assert v.is_cuda and v.dim() == 0 and lm.shape == (5, B + 1, 2)
    lm = lm.cpu().numpy()
    tag = f"ms_ssim {shape}"
    check_scalar(tag + " level mean ssim", lm[:, B, 0], s64, s32)
    check_scalar(tag + " level mean cs", lm[:, B, 1], c64, c32)
    check_scalar(tag + " value", v.item(), v64, v32)
    p64, ps64, pc64 = R.ms_ssim(x, y, torch.float64, per_image=True)
    p32 = R.ms_ssim(x, y, torch.float32, per_image=True)[0]
    if (pc64 > 0).all():
        check_scalar(tag + " per-image value", emdenoise.ms_ssim(up(x), up(y), per_image=True).cpu().numpy(), p64, p32)
    v3 = emdenoise.ms_ssim(up(x), up(y), level=3)
    check_scalar(tag + " level=3 value", v3.item(), R.ms_ssim(x, y, torch.float64, level=3)[0], R.ms_ssim(x, y, torch.float32, level=3)[0])
    assert np.float32(emdenoise.tf_ms_ssim(x, y)) == np.float32(v.item())


def test_ms_ssim_negative_cs_is_nan_as_in_the_reference():
    x, _ = pair(1, 176, 176, seed=9)
    y = (1.0 - x).astype(np.float32)
    v64, _, c64 = R.ms_ssim(x, y, torch.float64)
    assert (c64[:4] < 0).any() and np.isnan(v64)          # NaN in the restatement ...
    v = emdenoise.ms_ssim(up(x), up(y))
    assert torch.isnan(v).item()                          # ... NaN here: nothing is clamped
    assert np.isnan(emdenoise.ms_ssim(x, y))


def test_avg_pool_same_odd_extents():
    x = np.arange(2 * 5 * 7, dtype=np.float32).reshape(2, 5, 7, 1)
    got = metrics.avg_pool2x2_same(up(x)).cpu().numpy()
    want = R.avg_pool_same_t(torch.from_numpy(x.astype(np.float64))[..., 0][:, None])[:, 0].numpy()
    assert got.shape == (2, 3, 4, 1)
    np.testing.assert_array_equal(got[..., 0], want.astype(np.float32))     # small integers and halves: exact
    a, _ = pair(3, 203, 181)
    got = metrics.avg_pool2x2_same(up(a)).cpu().numpy()[..., 0]
    want = R.avg_pool_same_t(torch.from_numpy(a.astype(np.float64))[..., 0][:, None])[:, 0].numpy()
    assert got.shape == (3, 102, 91)
    # a sum of at most four float32 values and one multiplication: a few roundings of 2^-24 relative
    np.testing.assert_allclose(got, want, rtol=4 * 2.0 ** -24, atol=0)


# ---- psnr ----------------------------------------------------------------------------------------------------------------

def test_psnr():
    """Against numpy float64.  Bound: the kernel forms x - y in float32 (relative 2^-24 per element, so at most 2^-23 relative on
    the mse, 10 / ln 10 * 2^-23 = 5.2e-7 dB), sums in double, and rounds the result to float32 (half an ulp: 1.9e-6 dB below
    32 dB, 3.8e-6 below 64 dB): 5e-6 dB."""
    for (B, H, W) in [(2, 64, 64), (3, 75, 131), (2, 512, 512)]:
        x, y = pair(B, H, W)
        got = emdenoise.psnr(up(x), up(y), per_image=True).cpu().numpy()
        want = R.psnr(x, y, per_image=True)
        print(f"psnr {(B, H, W)}: {got} dB, abs error {np.abs(got - want).max():.2e}")
        assert np.abs(got - want).max() <= 5e-6
        assert abs(emdenoise.psnr(up(x), up(y)).item() - R.psnr(x, y)) <= 5e-6
        assert abs(emdenoise.psnr(up(x) * 255, up(y) * 255, data_range=255.0).item() - R.psnr(x * 255.0, y * 255.0, 255.0)) <= 1e-5
        p, m = emdenoise.psnr(x, y, return_mse=True)
        assert isinstance(p, float) and abs(m - ((x.astype(np.float64) - y) ** 2).mean()) <= 2.0 ** -22 * m
    x, _ = pair(2, 64, 64)
    assert torch.isinf(emdenoise.psnr(up(x), up(x))).item() and emdenoise.psnr(up(x), up(x)).item() > 0
    assert np.isinf(emdenoise.psnr(x, x, per_image=True)).all()


# ---- the loss and its gradient -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ssim_loss_value_and_gradient(shape):
    B, H, W = shape
    x, y = pair(B, H, W)
    xd, yd = up(x), up(y)
    for per_image in (False, True):
        l64, g64 = R.ssim_loss(x, y, torch.float64, per_image)
        l32, g32 = R.ssim_loss(x, y, torch.float32, per_image)
        dout = torch.zeros_like(xd)
        loss = emdenoise.ssim_loss(xd, yd, dout, per_image=per_image)
        assert loss.is_cuda and loss.shape == ((B,) if per_image else ())
        tag = f"ssim_loss {shape} per_image={per_image}"
        check_scalar(tag + " loss", loss.cpu().numpy(), l64, l32)
        check_field(tag + " gradient", dout.cpu().numpy()[..., 0], g64, g32)
        # the gradient ACCUMULATES, with a scale: dout0 + scale * g
        rng = np.random.default_rng(5)
        d0 = rng.standard_normal((B, H, W, 1)).astype(np.float32) * np.float32(np.abs(g64).max())
        acc = up(d0)
        emdenoise.ssim_loss(xd, yd, acc, scale=-2.5, per_image=per_image)
        g = dout.cpu().numpy().astype(np.float64)
        want = d0.astype(np.float64) - 2.5 * g
        # one product and one sum in float32 on top of the same gradient bits: 2^-23 of the larger operand
        assert np.abs(acc.cpu().numpy() - want).max() <= 2.0 ** -23 * (np.abs(d0).max() + 2.5 * np.abs(g).max())
        # value only (no dout): the same loss bits
        assert torch.equal(emdenoise.ssim_loss(xd, yd, per_image=per_image), loss)
    # per-image scales (a device array of B floats), as the per-image towers use them
    s = np.linspace(0.5, 2.0, B).astype(np.float32)
    l64, g64 = R.ssim_loss(x, y, torch.float64, True)
    l32, g32 = R.ssim_loss(x, y, torch.float32, True)
    dout = torch.zeros_like(xd)
    emdenoise.ssim_loss(xd, yd, dout, scale=up(s), per_image=True)
    check_field(f"ssim_loss {shape} per-image scales", dout.cpu().numpy()[..., 0], g64 * s[:, None, None].astype(np.float64),
                g32 * s[:, None, None])


def test_ssim_loss_accumulates_into_a_result_slot():
    """loss_acc / acc_stride / acc_weight: what the tower uses to make result3's loss the total."""
    B, H, W = 3, 64, 64
    x, y = pair(B, H, W)
    res = up(np.arange(3 * B, dtype=np.float32).reshape(B, 3))
    loss = emdenoise.ssim_loss(up(x), up(y), per_image=True, loss_acc=res.view(-1)[1:], acc_stride=3, acc_weight=0.5)
    want = np.arange(3 * B, dtype=np.float32).reshape(B, 3)
    want[:, 1] += np.float32(0.5) * loss.cpu().numpy()
    np.testing.assert_array_equal(res.cpu().numpy(), want)
    res1 = up(np.array([7.0, 8.0, 9.0], np.float32))
    loss = emdenoise.ssim_loss(up(x), up(y), loss_acc=res1[1:], acc_weight=2.0)
    np.testing.assert_array_equal(res1.cpu().numpy(), np.array([7.0, np.float32(8.0) + np.float32(2.0) * np.float32(loss.item()), 9.0], np.float32))


@pytest.mark.parametrize("shape", [(2, 64, 64), (3, 75, 131), (1, 11, 11)], ids=lambda s: "x".join(map(str, s)))
def test_canaries_nothing_outside_the_output_buffers_is_touched(shape):
    """Every output of the C routines sits inside a larger NaN-filled allocation; the guard regions must stay NaN."""
    B, H, W = shape
    size, G = 11, 4096
    Hm, Wm = H - size + 1, W - size + 1
    x, y = pair(B, H, W)
    xd, yd = up(x), up(y)
    lib = _lib.load()
    taps = metrics.gaussian_taps(size, 1.5)
    tp = taps.ctypes.data_as(C.c_void_p)

    def guarded(n, fill=None):
        buf = torch.full((G + n + G,), float("nan"), dtype=torch.float32, device=dev())
        if fill is not None:
            buf[G:G + n] = fill
        return buf, C.c_void_p(buf.data_ptr() + 4 * G)

    def intact(buf, n, name):
        torch.cuda.synchronize()
        assert torch.isnan(buf[:G]).all().item() and torch.isnan(buf[G + n:]).all().item(), f"{name}: guard region written"
        assert not torch.isnan(buf[G:G + n]).any().item(), f"{name}: output not fully written"

    ptr = lambda t: C.c_void_p(t.data_ptr())
    nb = lib.emd_ssim_workspace_bytes(B, H, W, size)
    ws, wsp = guarded(nb // 4, 0.0)
    means, mp = guarded(2 * (B + 1))
    smap, sp = guarded(B * Hm * Wm)
    cmap, cp = guarded(B * Hm * Wm)
    _lib.check(lib.emd_ssim_f32(ptr(xd), ptr(yd), B, H, W, tp, size, mp, sp, cp, wsp, nb, _lib.stream_ptr()))
    for buf, n, name in ((means, 2 * (B + 1), "means"), (smap, B * Hm * Wm, "ssim_map"), (cmap, B * Hm * Wm, "cs_map"), (ws, nb // 4, "workspace")):
        intact(buf, n, name)
    assert torch.equal(smap[G:G + B * Hm * Wm].view(B, Hm, Wm, 1), emdenoise.ssim(xd, yd, mean_metric=False))

    nb = lib.emd_ssim_loss_workspace_bytes(B, H, W, size)
    ws, wsp = guarded(nb // 4, 0.0)
    res, rp = guarded(2 * (B + 1))
    dout, dp = guarded(B * H * W, 0.0)
    _lib.check(lib.emd_ssim_loss_f32(ptr(xd), ptr(yd), B, H, W, tp, size, 0, 1.0, None, dp, rp, None, 1, 0.0, wsp, nb, _lib.stream_ptr()))
    for buf, n, name in ((res, 2 * (B + 1), "result"), (dout, B * H * W, "dout"), (ws, nb // 4, "loss workspace")):
        intact(buf, n, name)
    ref = torch.zeros_like(xd)
    emdenoise.ssim_loss(xd, yd, ref)
    assert torch.equal(dout[G:G + B * H * W].view(B, H, W, 1), ref)

    nb = lib.emd_psnr_workspace_bytes(B, H * W)
    ws, wsp = guarded(nb // 4, 0.0)
    out, op = guarded(2 * (B + 1))
    _lib.check(lib.emd_psnr_f32(ptr(xd), ptr(yd), B, H * W, 1.0, op, wsp, nb, _lib.stream_ptr()))
    intact(out, 2 * (B + 1), "psnr out")
    intact(ws, nb // 4, "psnr workspace")

    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    pooled, pp = guarded(B * Ho * Wo)
    _lib.check(lib.emd_avgpool2x2_same_c1_f32(ptr(xd), pp, B, H, W, _lib.stream_ptr()))
    intact(pooled, B * Ho * Wo, "pooled")


def test_canaries_ms_ssim():
    B, H, W, G = 1, 203, 181, 4096
    x, y = pair(B, H, W)
    xd, yd = up(x), up(y)
    lib = _lib.load()
    taps = metrics.gaussian_taps(11, 1.5)
    nb = lib.emd_ms_ssim_workspace_bytes(B, H, W, 5, 11)
    bufs = {}
    for name, n in (("ws", nb // 4), ("value", B + 1), ("levels", 5 * (B + 1) * 2)):
        buf = torch.full((G + n + G,), float("nan"), dtype=torch.float32, device=dev())
        bufs[name] = (buf, n, C.c_void_p(buf.data_ptr() + 4 * G))
    _lib.check(lib.emd_ms_ssim_f32(C.c_void_p(xd.data_ptr()), C.c_void_p(yd.data_ptr()), B, H, W, 5, taps.ctypes.data_as(C.c_void_p), 11,
                                   bufs["value"][2], bufs["levels"][2], bufs["ws"][2], nb, _lib.stream_ptr()))
    torch.cuda.synchronize()
    for name, (buf, n, _) in bufs.items():
        assert torch.isnan(buf[:G]).all().item() and torch.isnan(buf[G + n:]).all().item(), f"{name}: guard region written"
    assert not torch.isnan(bufs["value"][0][G:G + B + 1]).any().item()
    assert bufs["value"][0][G + B].item() == emdenoise.ms_ssim(xd, yd).item()


# ---- reproducibility and graph capture --------------------------------------------------------------------------------

def _all_results(xd, yd):
    dout = torch.zeros_like(xd)
    dout2 = torch.zeros_like(xd)
    out = [*emdenoise.ssim(xd, yd, cs_map=True, mean_metric=False), *emdenoise.ssim(xd, yd, cs_map=True, per_image=True),
           emdenoise.ssim(xd, yd), emdenoise.ms_ssim(xd, yd), emdenoise.ms_ssim(xd, yd, per_image=True), emdenoise.psnr(xd, yd, per_image=True),
           emdenoise.psnr(xd, yd), emdenoise.ssim_loss(xd, yd, dout), emdenoise.ssim_loss(xd, yd, dout2, per_image=True), dout, dout2]
    return out


def test_bitwise_reproducible_and_graph_replay_equals_eager():
    x, y = pair(2, 176, 208, seed=31)
    xd, yd = up(x), up(y)
    a = [t.clone() for t in _all_results(xd, yd)]
    b = _all_results(xd, yd)
    torch.cuda.synchronize()
    for k, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u, v), f"result {k} differs between two calls"
    # the same calls captured into a hipGraph (no synchronisation, no allocation inside the C routines) and replayed on new inputs
    sx, sy = torch.zeros_like(xd), torch.zeros_like(yd)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _all_results(sx, sy)
    torch.cuda.current_stream().wait_stream(s)
    with torch.cuda.graph(g):
        outs = _all_results(sx, sy)
    sx.copy_(xd)
    sy.copy_(yd)
    g.replay()
    torch.cuda.synchronize()
    for k, (u, v) in enumerate(zip(a, outs)):
        assert torch.equal(u, v), f"result {k}: captured-graph replay differs from the eager call"


# ---- the trainer -------------------------------------------------------------------------------------------------------

def _trainer(ssim_weight=0.0):
    from emdenoise import trainer as TR
    from tests.test_train_gpu import weights

    return TR.DenoiserTrainer(weights(smooth=True), dev(), ssim_weight=ssim_weight)


@pytest.mark.parametrize("per_image", [False, True], ids=["plain", "per_image"])
def test_tower_with_the_ssim_term(per_image):
    """Teacher-forced on the trainer's OWN output (the forward pass does not depend on the weight and is bit-identical run to
    run): last["ssim"], the total loss and the head gradient last["dout"] against the float64 restatement evaluated on that
    output."""
    B, S, w, gs = 2, 64, 1.0, 0.5
    lq, hq = synthetic_pair(B, S, S, seed=5)
    x, t = up(lq), up(hq)
    tr0 = _trainer()
    tr0.zero_grad()
    out0, res0 = tr0.tower(x, t, grad_scale=gs, per_image=per_image)
    dout0 = tr0.last["dout"].cpu().numpy().astype(np.float64)
    assert tr0.last["ssim"] is None
    tr1 = _trainer()
    tr1.zero_grad()
    out1, res1 = tr1.tower(x, t, grad_scale=gs, per_image=per_image, ssim_weight=w)
    torch.cuda.synchronize()
    assert torch.equal(out0, out1)
    out = out1.cpu().numpy()
    l64, g64 = R.ssim_loss(out, hq, torch.float64, per_image)
    l32, g32 = R.ssim_loss(out, hq, torch.float32, per_image)
    tag = f"tower per_image={per_image}"
    assert tr1.last["ssim"].shape == ((B,) if per_image else ())
    check_scalar(tag + " last['ssim']", tr1.last["ssim"].cpu().numpy(), 1.0 - l64, 1.0 - l32)
    r0, r1 = res0.cpu().numpy().astype(np.float64), res1.cpu().numpy().astype(np.float64)
    np.testing.assert_array_equal(r0[..., 0], r1[..., 0])          # mse
    np.testing.assert_array_equal(r0[..., 2], r1[..., 2])          # dloss/dout factor of the mse term
    # total loss: one float32 sum on top of the ssim term's error
    e = np.abs(r1[..., 1] - (r0[..., 1] + w * l64)).max()
    bound = max(FACTOR * np.abs(l32 - l64).max(), FLOOR) + 2.0 ** -23 * np.abs(r1[..., 1]).max()
    print(f"{tag} total loss {r1[..., 1]}: abs error {e:.3e}; bound {bound:.3e}")
    assert e <= bound
    # head gradient: dout_mse + w * grad_scale * g64; the ssim part carries FACTOR x the float32 restatement's error, the sum one
    # float32 rounding
    want = dout0 + w * gs * g64[..., None]
    got = tr1.last["dout"].cpu().numpy().astype(np.float64)
    err = np.linalg.norm(got - want)
    y32 = np.linalg.norm(w * gs * (g32.astype(np.float64) - g64))
    bound = FACTOR * y32 + 2.0 ** -23 * np.linalg.norm(want)
    print(f"{tag} dout: L2 error {err:.3e} (|dout| {np.linalg.norm(want):.3e}, ssim part {np.linalg.norm(w * gs * g64):.3e}); bound {bound:.3e}")
    assert err <= bound
    assert np.linalg.norm(got - dout0) > 0.5 * np.linalg.norm(w * gs * g64)


def test_tower_gradient_is_linear_in_the_weight_and_zero_weight_is_todays_path():
    """The forward pass and its relu masks do not depend on the weight, so the accumulated parameter gradient g(w) is affine in
    w: g(2) - g(0) = 2 (g(1) - g(0)) up to rounding.  Bound: each g carries float32 reassociation noise of at most 1e-6 relative
    (the bound of test_gradient_accumulation_run_to_run_spread; measured ~1e-7) and enters with coefficients 1, 2, 1, and the
    split-bf16 products of the backward GEMMs are linear to ~2^-24: 1e-5 of the largest |g|."""
    B, S = 2, 64
    lq, hq = synthetic_pair(B, S, S, seed=5)
    x, t = up(lq), up(hq)
    g, heads = {}, {}
    for w in (None, 0.0, 1.0, 2.0):
        tr = _trainer()
        tr.zero_grad()
        out, res = tr.tower(x, t) if w is None else tr.tower(x, t, ssim_weight=w)
        torch.cuda.synchronize()
        g[w] = tr.grads.detach().cpu().numpy().astype(np.float64)
        heads[w] = (out.clone(), res.clone(), tr.last["dout"].clone(), tr.last["ssim"])
    # ssim_weight = 0: bit-identical to calling tower without the keyword (the accumulated gradient only up to its atomics' order)
    for k in range(3):
        assert torch.equal(heads[None][k], heads[0.0][k])
    assert heads[0.0][3] is None and heads[None][3] is None
    assert rel_l2(g[0.0], g[None]) < 1e-6
    n = max(np.linalg.norm(v) for v in g.values())
    d1, d2 = g[1.0] - g[0.0], g[2.0] - g[0.0]
    dev_ = np.linalg.norm(d2 - 2.0 * d1)
    print(f"linearity: |g(2) - g(0) - 2 (g(1) - g(0))| = {dev_:.3e}; |g(0)| {np.linalg.norm(g[0.0]):.3e}, |g(1) - g(0)| {np.linalg.norm(d1):.3e}; "
          f"bound {1e-5 * n:.3e}")
    assert dev_ <= 1e-5 * n
    assert np.linalg.norm(d1) > 1e-3 * np.linalg.norm(g[0.0])      # g(1) != g(0): the term reaches the parameters


def test_train_step_graph_equals_eager_with_the_term_on():
    """One optimizer step with ssim_weight = 1, eager and as a captured hipGraph: same per-tower results, same update (up to the
    order of the gradient atomics: the bounds of test_streams_and_graph_match_eager's first step)."""
    from tests.test_train_gpu import flat, weights

    w = weights(smooth=True)
    names = [n for n in w if not n.endswith(("/moving_mean", "/moving_variance"))]
    p0 = flat(w, names)
    lq, hq = synthetic_pair(4, 64, 64, seed=200)
    runs = {}
    for mode, kw in (("eager", {}), ("graph", {"graph": True}), ("batched_graph", {"graph": True, "batched": True}),
                     ("batched_eager", {"batched": True}), ("off", {"ssim_weight": 0.0})):
        tr = _trainer(ssim_weight=1.0)
        res = tr.train_step(up(lq), up(hq), tower_batch=1, learning_rate=0.003, **kw)
        torch.cuda.synchronize()
        if kw.get("graph"):
            assert len(tr._graphs) == 1 and all(v is not None for v in tr._graphs.values()), "capture fell back to eager launches"
        runs[mode] = (res.cpu().numpy(), flat(tr.state_dict(), names))
    for a, b in (("graph", "eager"), ("batched_graph", "batched_eager")):
        np.testing.assert_array_equal(runs[a][0], runs[b][0])        # forward, losses: deterministic
        e = rel_l2(runs[a][1] - p0, runs[b][1] - p0)
        print(f"train_step {a} vs {b}: update rel L2 {e:.2e}")
        assert e < 1e-5
    # the term is on: the loss entry is larger than the mse term's alone, and the update differs
    assert (runs["eager"][0][:, 1] > runs["off"][0][:, 1]).all()
    np.testing.assert_array_equal(runs["eager"][0][:, 0], runs["off"][0][:, 0])
    assert rel_l2(runs["eager"][1] - p0, runs["off"][1] - p0) > 1e-3


def test_score_helpers():
    x, y = pair(2, 64, 64)
    p = emdenoise.KernelParams.initial(1, 3)
    m = emdenoise.Micrograph_Autoencoder(depth=1, width=3, params=p)
    s = m.score(up(x), up(y))
    pred = m.denoise_batch(up(x))
    assert set(s) == {"mse", "psnr", "ssim"} and all(v.is_cuda for v in s.values())
    assert s["ssim"].item() == emdenoise.ssim(pred, up(y)).item() and s["psnr"].item() == emdenoise.psnr(pred, up(y)).item()
    assert abs(s["mse"].item() - float(((pred.cpu().numpy().astype(np.float64) - y) ** 2).mean())) <= 2.0 ** -22 * s["mse"].item()
    sn = m.score(x, y)
    assert isinstance(sn["ssim"], float) and np.float32(sn["ssim"]) == np.float32(s["ssim"].item())
