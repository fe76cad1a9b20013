"""GPU tests of whole-micrograph denoising on the device (emdenoise.tiling, csrc/tile_ops.hip).

1. the tiling kernels against float64 numpy restatements, with random predictions (no network in the loop);
2. denoise_images end to end against each class's host denoise() on seeded synthetic micrographs;
3. stacks pooled into batches smaller than one image's tile count against per-image calls;
4. containers and determinism."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import emdenoise  # noqa: E402
from emdenoise import autoencoder as AE  # noqa: E402
from emdenoise import tiling  # noqa: E402
from tests.synth_inputs import synthetic_lq  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def lq(H, W, seed):
    return synthetic_lq(1, H, W, seed=seed)[0, :, :, 0]


@pytest.fixture(scope="module")
def d_model():
    return emdenoise.Denoiser()


@pytest.fixture(scope="module")
def s_model():
    return AE.Micrograph_Autoencoder(encoding_features=16)


def k_model(depth, width, seed):
    rng = np.random.default_rng(seed)
    n = len(emdenoise.kernel_denoiser.sym_pairs(width))
    w = [rng.normal(1.0 / (width * width), 0.05, n) for _ in range(depth)]
    b = [np.zeros(n)] + [rng.normal(0, 0.3, n) for _ in range(depth - 1)]
    s = [1.0] + list(rng.uniform(0.5, 1.5, depth - 1))
    return emdenoise.Micrograph_Autoencoder(depth=depth, width=width, params=emdenoise.KernelParams.from_symmetric(w, b, s, width))


# ---- 1. kernels ----------------------------------------------------------------------------------------------------------------
def _gather(src_np, plan, rescale):
    src = torch.from_numpy(src_np).to(DEV)
    N = src_np.shape[0]
    T = N * plan.tiles_per_image
    keep, dp = plan.device_arrays(DEV)
    out = torch.full((T, plan.cs, plan.cs), -7.0, device=DEV)
    cst = torch.empty((T, 2), device=DEV) if rescale else None
    tiling.gather(src, plan, dp, 0, T, out, cst)
    torch.cuda.synchronize()
    return out.cpu().numpy(), (cst.cpu().numpy() if rescale else None)


def _host_crops(src_np, plan):
    crops = []
    for img in src_np:
        padded = np.pad(img, plan.pad, mode="reflect")
        crops += [padded[y:y + plan.cs, x:x + plan.cs] for y in plan.ys for x in plan.xs]
    return np.stack(crops)


@pytest.mark.parametrize("case", ["d", "s", "s_wide_pad"])
def test_gather_copy_is_bitwise_reflect_slicing(case):
    rng = np.random.default_rng(1)
    if case == "d":
        src = rng.standard_normal((2, 600, 700)).astype(np.float32)
        plan = tiling.d_plan(600, 700, 512, 80)
    elif case == "s":
        src = rng.standard_normal((2, 230, 301)).astype(np.float32)
        plan = tiling.s_plan(230, 301, 160, 25, 1)
    else:  # pad wider than the image: numpy reflects repeatedly
        src = rng.standard_normal((1, 20, 33)).astype(np.float32)
        plan = tiling.TilePlan(20, 33, 64, 50, 0, [0, 36, 56], [0, 40, 69])
    got, _ = _gather(src, plan, rescale=False)
    np.testing.assert_array_equal(got, _host_crops(src, plan))


def test_gather_rescale_within_one_ulp():
    rng = np.random.default_rng(2)
    src = (rng.random((2, 230, 301)) * 40 - 5).astype(np.float32)
    src[1, :, :] = 3.25                                               # image 1: every crop flat
    plan = tiling.s_plan(230, 301, 160, 25, 1)
    got, cst = _gather(src, plan, rescale=True)
    crops = _host_crops(src, plan)
    off64 = crops.min(axis=(1, 2)).astype(np.float64)
    mean64 = crops.astype(np.float64).mean(axis=(1, 2))
    np.testing.assert_array_equal(cst[:, 0], off64.astype(np.float32))
    ulp = np.spacing(np.maximum(np.abs(mean64), np.abs(mean64 - off64)).astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(cst[:, 1] - (mean64 - off64)) <= ulp)
    flat = cst[:, 1] == 0
    assert flat.sum() == plan.tiles_per_image and flat[plan.tiles_per_image:].all()
    ref = (crops - cst[:, 0, None, None]) / np.where(flat, 1.0, cst[:, 1]).astype(np.float32)[:, None, None]
    ref[flat] = 1.0
    np.testing.assert_array_equal(got, ref)                           # the same float32 ops on the kernel's (off, scale)
    ref64 = (crops - off64[:, None, None]) / np.where(flat, 1.0, mean64 - off64)[:, None, None]
    ref64[flat] = 1.0
    assert np.max(np.abs(got - ref64) / np.maximum(np.abs(ref64), 1.0)) < 4 * np.finfo(np.float32).eps


@pytest.mark.parametrize("mode", ["d", "d_clip", "s"])
def test_blend_matches_float64_overlap_add(mode):
    rng = np.random.default_rng(3)
    N = 2
    if mode.startswith("d"):
        plan = tiling.d_plan(600, 1031, 512, 80)
    else:
        plan = tiling.s_plan(230, 301, 160, 25, 1)
    T = N * plan.tiles_per_image
    preds = (rng.standard_normal((T, plan.cs, plan.cs)) * 0.4 + 0.5).astype(np.float32)
    cst = None
    if mode == "s":
        cst = np.stack([rng.random(T) * 3, rng.random(T) + 0.5], axis=1).astype(np.float32)
        cst[3, 1] = 0.0                                               # a flat crop
    keep, dp = plan.device_arrays(DEV)
    out = tiling.blend(torch.from_numpy(preds).to(DEV), plan, dp, N, None if cst is None else torch.from_numpy(cst).to(DEV),
                       clip=mode == "d_clip").cpu().numpy()
    Hp, Wp = plan.H + 2 * plan.pad, plan.W + 2 * plan.pad
    m, cs = plan.m, plan.cs
    for n in range(N):
        acc, cnt = np.zeros((Hp, Wp)), np.zeros((Hp, Wp))
        t = n * plan.tiles_per_image
        for y in plan.ys:
            for x in plan.xs:
                p = preds[t] if cst is None else preds[t] * cst[t, 1] + cst[t, 0]
                acc[y + m:y + cs - m, x + m:x + cs - m] += p[m:cs - m, m:cs - m]
                cnt[y + m:y + cs - m, x + m:x + cs - m] += 1
                t += 1
        core = (slice(plan.pad, plan.pad + plan.H), slice(plan.pad, plan.pad + plan.W))
        ref = acc[core] / cnt[core]
        if mode == "d_clip":
            ref = ref.clip(0.0, 1.0)
        assert np.max(np.abs(out[n] - ref) / np.maximum(np.abs(ref), 1e-3)) <= 1e-6


def _nasty(img):
    img = img.copy()
    img[3, 5] = np.nan
    img[10, 20] = np.inf
    img[-2, -7] = -np.inf
    return img


def test_prep_s_matches_host_preprocess(s_model):
    imgs = np.stack([lq(230, 301, 5) * 17 + 3, _nasty(lq(230, 301, 6)), np.full((230, 301), 2.0, np.float32)])
    got, _ = tiling.prepare(torch.from_numpy(imgs).to(DEV), tiling.PREP_S)
    got = got.cpu().numpy()
    for g, img in zip(got, imgs):
        ref = s_model.preprocess(img)[..., 0]
        np.testing.assert_allclose(g, ref, rtol=2e-6, atol=1e-7)


@pytest.mark.parametrize("width", [3, 5, 15])
def test_prep_k_matches_host_statistics(width):
    p = width // 2
    imgs = np.stack([lq(40, 57, 7) * 233 - 4, _nasty(lq(40, 57, 8) * 9), np.full((40, 57), -1.5, np.float32)])
    x = torch.from_numpy(imgs).to(DEV)
    got, st = tiling.prepare(x, tiling.PREP_K, p)
    got, st = got.cpu().numpy(), st.cpu().numpy()
    for g, s, img in zip(got, st, imgs):
        clean = np.where(np.isfinite(img), img, 0).astype(np.float32)
        padded = np.pad(clean.astype(np.float64), p, mode="reflect")
        off = padded.min()
        assert s[0] == off
        if padded.max() == off:
            assert s[1] == 0 and s[2] == 1 and np.all(g == 1.0)
            continue
        mean64 = padded.mean()
        assert s[2] == 0 and abs(s[1] - (mean64 - off)) <= np.spacing(np.float32(mean64)) + 1e-12 * abs(mean64)
        ref = (clean - np.float32(off)) / np.float32(s[1])
        np.testing.assert_array_equal(g, ref)
        np.testing.assert_allclose(g, (clean - off) / (mean64 - off), rtol=4e-7, atol=4e-7)


@pytest.mark.parametrize("shape", [(512, 512), (600, 700), (300, 260)])
def test_prep_d_matches_host_preprocess(d_model, shape):
    H, W = shape
    base = lq(H, W, 9)
    inf_only = base.copy()
    inf_only[7, 9] = np.inf
    one_nan = base.copy()
    one_nan[H - 1, 0] = np.nan
    imgs = np.stack([base * 5 + 1, inf_only, one_nan, np.full((H, W), 0.25, np.float32)])
    got, _ = tiling.prepare(torch.from_numpy(imgs).to(DEV), tiling.PREP_D, 512)
    got = got.cpu().numpy()
    for g, img in zip(got, imgs):
        ref = d_model.preprocess(img)[0, :, :, 0]
        assert np.max(np.abs(g - ref)) <= 1e-6
    # numpy's NaN semantics: one NaN anywhere makes the whole image 0.5
    assert np.all(got[2] == 0.5) and np.all(got[3] == 0.5)


def test_affine_inverse():
    rng = np.random.default_rng(4)
    x = rng.standard_normal((3, 17, 19)).astype(np.float32)
    st = np.array([[1.5, 0.25, 0.0], [-2.0, 3.0, 0.0], [4.0, 0.0, 1.0]])
    y = tiling.affine(torch.from_numpy(x).to(DEV), torch.from_numpy(st).to(DEV), out=torch.empty((3, 17, 19), device=DEV)).cpu().numpy()
    x64 = x.astype(np.float64)                                              # the host's den is float64
    ref = np.stack([x64[0] * 0.25 + 1.5, x64[1] * 3.0 - 2.0, x64[2] * 4.0])
    np.testing.assert_array_equal(y, ref.astype(np.float32))


# ---- 2. end to end against the host denoise() ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(512, 512), (600, 700), (1031, 2047), (2048, 2048)])
def test_d_end_to_end(d_model, shape):
    img = lq(*shape, seed=sum(shape))
    ref = d_model.denoise(img, preprocess=False, overlap=80)
    got = d_model.denoise_images(img, preprocess=False, overlap=80)
    assert got.dtype == np.float32 and got.shape == img.shape
    assert np.max(np.abs(got - ref)) <= 1e-6


def test_d_end_to_end_preprocess_nonfinite(d_model):
    imgs = [_nasty(lq(600, 700, 21)), lq(700, 600, 22) * 3]
    imgs[1][100, 200] = np.inf
    for img in imgs:
        ref = d_model.denoise(img, preprocess=True, postprocess=True)
        got = d_model.denoise_images(img, preprocess=True, postprocess=True)
        assert got.shape == (512, 512) and np.max(np.abs(got - ref)) <= 1e-5


def test_d_too_small_raises(d_model):
    with pytest.raises(ValueError):
        d_model.denoise_images(np.zeros((500, 600), np.float32), preprocess=False)


@pytest.mark.parametrize("shape", [(110, 110), (230, 301), (2048, 2048)])
@pytest.mark.parametrize("ov", [(25, 1), (25, 25), (10, 3)])
def test_s_end_to_end(s_model, shape, ov):
    if min(shape) + 2 * ov[0] < 160:
        with pytest.raises(ValueError):
            s_model.denoise(lq(*shape, seed=1), overlap=ov[0], used_overlap=ov[1])
        with pytest.raises(ValueError):
            s_model.denoise_images(lq(*shape, seed=1), overlap=ov[0], used_overlap=ov[1])
        return
    img = lq(*shape, seed=shape[0] + 3 * ov[1])
    ref = s_model.denoise(img, overlap=ov[0], used_overlap=ov[1])
    got = s_model.denoise_images(img, overlap=ov[0], used_overlap=ov[1])
    assert got.dtype == np.float32 and got.shape == img.shape
    # 1e-5 is the network's own floor here: a 1-ulp change of every input crop moves graph S's output by 9.9e-6 rel L2, and
    # numpy's float32 means are an ulp off the correctly rounded ones the kernels compute (measured up to 1.06e-5)
    assert rel_l2(got, ref) <= 2e-5
    # against the host method restated with correctly rounded means, the device path is exact up to the blend's rounding
    assert rel_l2(got, s_host_exact_means(s_model, img, *ov)) <= 1e-6


def s_host_exact_means(nn, img, overlap, used_overlap):
    """autoencoder.Micrograph_Autoencoder.denoise with every mean accumulated in float64 and rounded to float32 once."""
    cs = nn.cropsize
    overlap = max(overlap, used_overlap)
    x = np.where(np.isfinite(img), img, 0).astype(np.float32)
    x = AE.scale0to1(x)
    x = x / np.float32(x.astype(np.float64).mean())
    padded = np.pad(x, overlap, mode="reflect")
    pos = [(y, xx) for y in tiling.s_starts(padded.shape[0], cs, overlap) for xx in tiling.s_starts(padded.shape[1], cs, overlap)]
    crops = np.stack([padded[y:y + cs, xx:xx + cs] for (y, xx) in pos])
    offs = crops.min(axis=(1, 2))
    scales = crops.astype(np.float64).mean(axis=(1, 2)).astype(np.float32) - offs
    flat = scales == 0
    norm = (crops - offs[:, None, None]) / np.where(flat, 1.0, scales).astype(np.float32)[:, None, None]
    norm[flat] = 1.0
    preds = np.concatenate([nn._run(norm[i:i + 64]) for i in range(0, len(pos), 64)])
    preds = preds * np.where(flat, 0.0, scales).astype(np.float32)[:, None, None] + offs[:, None, None]
    H, W = padded.shape
    acc, cnt = np.zeros((H, W)), np.zeros((H, W))
    m = overlap - used_overlap
    for (y, xx), pr in zip(pos, preds):
        acc[y + m:y + cs - m, xx + m:xx + cs - m] += pr[m:cs - m, m:cs - m]
        cnt[y + m:y + cs - m, xx + m:xx + cs - m] += 1
    core = (slice(overlap, H - overlap), slice(overlap, W - overlap))
    return (acc[core] / cnt[core]).astype(np.float32)


@pytest.mark.parametrize("preprocess", [True, False])
def test_s_end_to_end_flat_image(s_model, preprocess):
    img = np.full((230, 301), 0.75, np.float32)
    ref = s_model.denoise(img, preprocess=preprocess)
    got = s_model.denoise_images(img, preprocess=preprocess)
    assert rel_l2(got, ref) <= 1e-5


@pytest.mark.parametrize("dw", [(1, 3), (2, 3), (3, 5)])
def test_k_end_to_end(dw):
    d, w = dw
    nn = k_model(d, w, seed=10 * d + w)
    for img in (lq(300, 257, d + w) * 40 + 2, _nasty(lq(64, 90, 5))):
        for pre, post in ((True, True), (True, False), (False, True)):
            ref = nn.denoise(img, preprocess=pre, postprocess=post)
            got = nn.denoise_images(img, preprocess=pre, postprocess=post)
            assert got.dtype == np.float32 and got.shape == img.shape
            if not pre:
                ok = np.isfinite(ref)
                assert np.array_equal(ok, np.isfinite(got)) and rel_l2(got[ok], ref[ok]) <= 1e-6
            else:
                assert rel_l2(got, ref) <= 1e-6
    flat = np.full((33, 40), 2.5, np.float32)
    assert rel_l2(nn.denoise_images(flat), nn.denoise(flat)) <= 1e-6


# ---- 3. stacks and chunking ----------------------------------------------------------------------------------------------------
def test_d_stack_chunked_is_bitwise_per_image(d_model):
    stack = np.stack([lq(600, 700, 31 + i) for i in range(3)])
    got = d_model.denoise_images(stack, preprocess=False, max_batch=7)      # 4 tiles per image: chunks straddle images
    assert got.shape == stack.shape
    for i in range(3):
        np.testing.assert_array_equal(got[i], d_model.denoise_images(stack[i], preprocess=False))


def test_s_stack_chunked_matches_per_image(s_model):
    stack = np.stack([lq(230, 301, 41 + i) for i in range(3)])
    got = s_model.denoise_images(stack, max_batch=7)                        # 12 crops per image
    for i in range(3):
        assert rel_l2(got[i], s_model.denoise_images(stack[i])) <= 1e-6


def test_k_stack_matches_per_image():
    nn = k_model(2, 3, seed=5)
    stack = np.stack([lq(64, 90, 51 + i) * (i + 1) for i in range(4)])
    got = nn.denoise_images(stack)
    for i in range(4):
        assert rel_l2(got[i], nn.denoise_images(stack[i])) <= 1e-6


# ---- 4. containers and determinism -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["d", "s", "k"])
def test_containers_and_determinism(d_model, s_model, cls):
    if cls == "d":
        img = lq(600, 700, 61)
        call = lambda v: d_model.denoise_images(v, preprocess=False)  # noqa: E731
    elif cls == "s":
        img = lq(230, 301, 62)
        call = s_model.denoise_images
    else:
        img = lq(64, 90, 63)
        call = k_model(2, 3, seed=6).denoise_images
    a = call(img)
    assert isinstance(a, np.ndarray) and a.dtype == np.float32 and a.shape == img.shape
    np.testing.assert_array_equal(call(img), a)                             # two identical calls: the same bits
    x = torch.from_numpy(img).to(DEV)
    before = x.clone()
    y = call(x)
    assert isinstance(y, torch.Tensor) and y.is_cuda and y.dtype == torch.float32 and y.shape == x.shape
    assert torch.equal(x, before)                                           # the input is not modified
    np.testing.assert_array_equal(y.cpu().numpy(), a)
    c = call(torch.from_numpy(img[None].copy()))
    assert isinstance(c, torch.Tensor) and not c.is_cuda and c.shape == (1, *img.shape)
    np.testing.assert_array_equal(c[0].numpy(), a)


def test_k_too_small_fails_as_the_host_does():
    """The filter's REFLECT padding needs width // 2 < min(H, W): the host denoise's launch refuses smaller images with EmdError,
    with or without preprocess (its np.pad succeeds, the filter launch does not); denoise_images raises the same error."""
    nn = k_model(1, 7, seed=3)
    img = lq(3, 40, 71)
    for pre in (True, False):
        with pytest.raises(emdenoise._lib.EmdError):
            nn.denoise(img, preprocess=pre)
        with pytest.raises(emdenoise._lib.EmdError):
            nn.denoise_images(img, preprocess=pre)
