"""GPU tests of graph K's paired training (csrc/k_pair.hip through emdenoise.k_trainer) against the float64 restatement
tests/k_pair_ref.py (pinned by tests/test_k_pair.py): loss and gradients under both border modes, the tie to the unpaired
kernel, the sqrt rule, Adam trajectories at the paired preset, determinism, recovery of a known kernel, the pair maker, distill
against Micrograph_Autoencoder.denoise_crop, and the four-step pipeline end to end."""
import numpy as np
import pytest
import torch

import emdenoise
from emdenoise import autoencoder
from emdenoise import k_trainer as KT
from emdenoise.kernel_denoiser import KernelParams, Micrograph_Autoencoder
from oracle import kernel_denoiser as KO

from . import k_pair_ref as R
from .synth_inputs import synthetic_lq

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
BAR = 2e-5        # the gradient bound of tests/test_k_train_gpu.py
TRAJ_BAR = 1e-4   # its trajectory bound on theta


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def rand_params(depth, width, seed):
    return KernelParams(*KO.full_maps(KO.random_params(depth, width, seed=seed)))


def pair_batch(shape, seed, scale=1.0, mix=0.0):
    """x: positive, mean-normalised patches; truth = scale (mix x + (1 - mix) y) with y another such image."""
    def one(s):
        v = synthetic_lq(shape[0], shape[1], shape[2], seed=s)[..., 0].astype(np.float64)
        return v / np.maximum(v.mean(axis=(1, 2), keepdims=True), 1e-9)
    x = one(seed)
    return x.astype(np.float32), (scale * (mix * x + (1.0 - mix) * one(seed + 7919))).astype(np.float32)


def check_grad(shape, depth, width, pad, rule=True, bar=BAR, near_output=None):
    """near_output = a: truth is the oracle's own F(x) (in float64, from the same parameters) plus a times the second image, so
    that the MSE is about a^2 E[y^2] whatever the random filter returns -- chosen on the CPU, before the device runs."""
    x, t = pair_batch(shape, 2000 + depth * 17 + width)
    p = rand_params(depth, width, seed=depth * 100 + width)
    if near_output is not None:
        o = width // 2 if pad == "valid" else 0
        fx = R.pair_forward(torch.from_numpy(x).double(), torch.from_numpy(KT.theta_from_params(p)).double(), depth, width, pad).numpy()
        base = np.zeros(shape)
        base[:, o:shape[1] - o, o:shape[2] - o] = fx
        t = (base + near_output * t).astype(np.float32)
    tr = emdenoise.KernelDenoiserTrainer([(depth, width)], device=DEV, initial=[p], beta1=0.5)
    L, g = tr.loss_and_grad_pair(x, t, pad=pad, sqrt_above_1=rule)
    Lr, gr, mse = R.pair_loss_and_grad(x, t, KT.theta_from_params(p), depth, width, pad, rule)
    print(f"{shape} d{depth} w{width} {pad} rule={rule}: mse {mse:.4g} loss {L:.7g} vs {Lr:.7g}, grad rel L2 {rel_l2(g, gr):.2e}")
    assert abs(L - Lr) <= bar * abs(Lr), (L, Lr)
    assert rel_l2(g, gr) <= bar, rel_l2(g, gr)
    assert float(tr.evaluate_pair(x, t, pad=pad, sqrt_above_1=rule)[0]) == pytest.approx(L, rel=1e-6)
    return L, g, mse


@pytest.mark.parametrize("B", [1, 32])
@pytest.mark.parametrize("width", [3, 5, 7, 15])
@pytest.mark.parametrize("depth", [1, 2, 3])
def test_grad_valid_20x20(depth, width, B):
    check_grad((B, 20, 20), depth, width, "valid")


@pytest.mark.parametrize("depth,width", [(1, 3), (2, 5), (3, 7), (2, 15)])
def test_grad_valid_nonsquare_3x17x29(depth, width):
    check_grad((3, 17, 29), depth, width, "valid")


@pytest.mark.parametrize("depth,width", [(1, 3), (2, 7), (3, 15)])
def test_grad_valid_one_output_pixel_per_image(depth, width):
    """width == min(H, W) == H == W: the interior is a single pixel."""
    check_grad((5, width, width), depth, width, "valid")


@pytest.mark.parametrize("pad", ["valid", "reflect"])
def test_grad_2x512x512(pad):
    check_grad((2, 512, 512), 2, 3, pad)


@pytest.mark.parametrize("depth,width,shape", [(2, 3, (4, 33, 20)), (3, 5, (32, 20, 20)), (1, 7, (2, 512, 512))])
def test_reflect_with_truth_equal_x_is_the_unpaired_image_loss(depth, width, shape):
    x, _ = pair_batch(shape, 31)
    p = rand_params(depth, width, seed=5)
    tr = emdenoise.KernelDenoiserTrainer([(depth, width)], device=DEV, loss="image", initial=[p])
    L0, g0 = tr.loss_and_grad(x)
    L1, g1 = tr.loss_and_grad_pair(x, x, pad="reflect", sqrt_above_1=False)
    print(f"unpaired {L0:.9g} paired {L1:.9g} grad rel L2 {rel_l2(g1, g0):.2e}")
    assert abs(L1 - L0) <= 1e-6 * abs(L0) and rel_l2(g1, g0) <= 1e-6


@pytest.mark.parametrize("depth,width", [(1, 3), (2, 5)])
def test_sqrt_rule(depth, width):
    # truth = F(x) + 3 y: the oracle's MSE is about 9 E[y^2], far above 1; F(x) + 0.4 y: about 0.16 E[y^2], far below
    L_on, g_on, mse = check_grad((4, 20, 20), depth, width, "valid", rule=True, near_output=3.0)
    assert mse > 2.0, mse
    L_off, g_off, _ = check_grad((4, 20, 20), depth, width, "valid", rule=False, near_output=3.0)
    assert abs(L_off - mse) <= BAR * mse and abs(L_on - np.sqrt(mse)) <= BAR * np.sqrt(mse)   # flag off: the plain MSE
    assert rel_l2(g_on * 2 * np.sqrt(mse), g_off) <= BAR
    a = check_grad((4, 20, 20), depth, width, "valid", rule=True, near_output=0.4)
    assert a[2] < 0.5, a[2]
    b = check_grad((4, 20, 20), depth, width, "valid", rule=False, near_output=0.4)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])   # below 1 the flag changes nothing, bit for bit


def test_adam_trajectory_matches_float64_tf_adam():
    """50 steps of the paired preset's Adam (beta1 = 0.5, lr = 0.01 (1 - t/10001)) on fixed pair batches; the first two batches'
    truth is scaled so that the oracle's MSE exceeds 1 there (asserted): those steps take the sqrt branch."""
    configs = [(1, 3), (2, 5)]
    batches = [pair_batch((8, 20, 20), 60 + k, scale=5.0 if k < 2 else 1.0, mix=0.0 if k < 2 else 0.8) for k in range(5)]
    tr = emdenoise.KernelDenoiserTrainer(configs, device=DEV, seed=7, lr0=0.01, total_steps=10000, beta1=0.5)
    th0 = [KT.theta_from_params(tr.params(c)).astype(np.float64) for c in configs]
    got = np.array([tr.train_step_pair(*batches[t % 5]) for t in range(50)])
    for i, (d, w) in enumerate(configs):
        th, losses, mses = R.pair_adam(th0[i], batches, 50, d, w)
        assert mses[0] > 2.0 and np.sum(mses > 2.0) >= 2 and np.any(mses < 0.5), mses[:6]   # both branches, clearly
        assert np.abs(mses - 1.0).min() > 1e-3   # no step where float32 rounding could pick the other branch
        err = np.abs(tr.filters[i].theta.cpu().numpy() - th).max()
        print(f"({d},{w}): sqrt steps {int(np.sum(mses > 1.0))}, theta err {err:.2e}, loss rel {np.abs(got[:, i] / losses - 1).max():.2e}")
        assert err <= TRAJ_BAR, err
        assert np.abs(got[:, i] / losses - 1).max() <= 1e-3
    assert np.array_equal(tr.packed_params((2, 5)).cpu().numpy(), tr.params((2, 5)).packed())
    assert all(int(f.step.item()) == 50 for f in tr.filters)


def test_paired_step_is_bitwise_deterministic():
    x, t = pair_batch((8, 64, 64), 3, scale=3.0)   # the first steps are on the sqrt branch
    runs = []
    for _ in range(2):
        tr = emdenoise.KernelDenoiserTrainer([(3, 5), (1, 7)], device=DEV, seed=4, lr0=0.01, total_steps=10000, beta1=0.5)
        lg = tr.loss_and_grad_pair(x, t, (3, 5))
        losses = [tr.train_step_pair(x, t) for _ in range(5)] + [tr.train_step_pair(x, t, pad="reflect")]
        runs.append((lg, losses, [[a.cpu().numpy() for a in (f.theta, f.m, f.v)] for f in tr.filters]))
    (l0, g0), L0, S0 = runs[0]
    (l1, g1), L1, S1 = runs[1]
    assert l0 == l1 and np.array_equal(g0, g1)
    assert all(np.array_equal(a, b) for a, b in zip(L0, L1))
    assert all(np.array_equal(a, b) for fa, fb in zip(S0, S1) for a, b in zip(fa, fb))


RECOVERY_STEPS = 160


def recovery_pairs(n=64, seed=2024):
    rng = np.random.default_rng(seed)
    x = rng.random((n, 20, 20))
    x = x - x.min(axis=(1, 2), keepdims=True)
    x = (x / x.mean(axis=(1, 2), keepdims=True)).astype(np.float32)   # minimum 0, mean 1, as make_pairs leaves a patch
    t = np.zeros((n, 20, 20), np.float32)
    t[:, 1:-1, 1:-1] = R.apply_valid_3x3(x, R.d4_kernel(0.4, 0.1, 0.05)).astype(np.float32)
    return x, t


def test_recovers_a_known_kernel():
    """t = a known D4-symmetric 3 x 3 kernel (centre 0.4, edge 0.1, corner 0.05) applied to random x, VALID; (1,3) trained with
    the preset, one pair per step, from the box filter.

    Measured on the CPU with the float64 trainer of k_pair_ref (pair_adam) on these pairs: max |theta - kernel| is 1.9e-2
    after 50 steps, 2.1e-4 after 100, 1.5e-6 after 150, 5.4e-7 after 160 and 2.8e-6 after 170.  Once the residual is at
    rounding level Adam's normalised step m / sqrt(v) is no longer small, and the float64 trainer itself leaves the optimum in
    bursts (1.7e-3 at step 190, 2.4e-3 at 200, back to 4.7e-8 at 250, 5.4e-4 at 350, ...), so more steps do not mean closer.
    160 steps is what the oracle needs; there its distance is 5.4e-7 (asserted below 1e-5: five digits of every tap), and a
    float32 emulation of the same loop stays within 5.3e-8 of it at steps 140-170 (3.3e-7 at 170), so the existing 1e-4
    trajectory bound on theta holds unscaled."""
    x, t = recovery_pairs()
    kernel = np.array([0.4, 0.1, 0.05])
    tr = emdenoise.KernelDenoiserTrainer([(1, 3)], device=DEV, lr0=0.01, total_steps=10000, beta1=0.5,
                                         initial=[KernelParams.initial(1, 3)])
    hist = tr.train_pairs(x, t, RECOVERY_STEPS)["loss"][:, 0]
    got = tr.filters[0].theta.cpu().numpy().astype(np.float64)
    th, losses, _ = R.pair_adam(np.full(3, 1.0 / 9.0), [(x[i:i + 1], t[i:i + 1]) for i in range(len(x))], RECOVERY_STEPS, 1, 3)
    print(f"oracle distance {np.abs(th - kernel).max():.2e}, device distance {np.abs(got - kernel).max():.2e}, "
          f"device - oracle {np.abs(got - th).max():.2e}, loss {hist[0]:.3g} -> {hist[-1]:.3g}")
    assert np.abs(th - kernel).max() <= 1e-5
    assert np.abs(got - th).max() <= TRAJ_BAR
    assert np.abs(got - kernel).max() <= TRAJ_BAR + 1e-5
    assert np.abs(hist[:20] / losses[:20] - 1).max() <= 1e-3


# ---- the pair maker
def pair_stacks(N=12, S=160, seed=5):
    a = synthetic_lq(N, S, S, seed=seed)[..., 0].astype(np.float32) * 37.0 + 3.0
    b = synthetic_lq(N, S, S, seed=seed + 1)[..., 0].astype(np.float32) * 11.0 - 2.0
    return a, b


def test_make_pairs_matches_float64_and_draws_stay_in_the_window():
    a, b = pair_stacks(40)
    x, t, draws = emdenoise.make_pairs(a, b, seed=9, return_draws=True, device=DEV)
    d = draws.cpu().numpy()
    assert d.shape == (40, 2) and d.min() >= 20 and d.max() < 120 and len({tuple(v) for v in d}) > 30
    xr, tr_ = R.make_pairs_ref(a, b, d)
    assert x.shape == (40, 20, 20) and rel_l2(x.cpu().numpy(), xr) <= 1e-6 and rel_l2(t.cpu().numpy(), tr_) <= 1e-6
    # another window and patch; both stacks see the same draw
    x2, t2, d2 = emdenoise.make_pairs(a, a, patch=8, lo=0, hi=153, seed=9, return_draws=True, device=DEV)
    d2 = d2.cpu().numpy()
    assert d2.min() >= 0 and d2.max() <= 152 and d2.max() > 120 and torch.equal(x2, t2)
    assert rel_l2(x2.cpu().numpy(), R.make_pairs_ref(a, a, d2, 8)[0]) <= 1e-6
    # same seed -> same bits; another first_index -> other draws, and index n + k of one call is index n of the call at k
    x3, t3, d3 = emdenoise.make_pairs(a, b, seed=9, return_draws=True, device=DEV)
    assert torch.equal(x, x3) and torch.equal(t, t3) and torch.equal(draws, d3)
    d4 = emdenoise.make_pairs(a, b, seed=9, first_index=5, return_draws=True, device=DEV)[2].cpu().numpy()
    assert not np.array_equal(d4, d) and np.array_equal(d4[:35], d[5:])
    assert not np.array_equal(emdenoise.make_pairs(a, b, seed=10, return_draws=True, device=DEV)[2].cpu().numpy(), d)
    with pytest.raises(ValueError):
        emdenoise.make_pairs(a, b, hi=20, device=DEV)


def test_make_pairs_nonfinite_and_flat_images():
    a, b = pair_stacks(6)
    d = emdenoise.make_pairs(a, b, seed=1, return_draws=True, device=DEV)[2].cpu().numpy()
    a[0, d[0, 0] + 3, d[0, 1] + 4] = np.nan          # a NaN inside the drawn window
    b[1, (d[1, 0] + 60) % 160, 0] = np.nan           # a NaN outside it: np.min is NaN, the whole image rescales to NaN
    assert not (d[1, 1] <= 0 < d[1, 1] + 20)
    a[2] = 4.25                                      # a flat image: m == 0
    b[3, 0, 0] = np.inf                              # +Inf outside the window: mean = inf, (img - c) / inf = 0 in the window
    x, t, d1 = emdenoise.make_pairs(a, b, seed=1, return_draws=True, device=DEV)
    assert np.array_equal(d1.cpu().numpy(), d)
    x, t = x.cpu().numpy(), t.cpu().numpy()
    xr, tr_ = R.make_pairs_ref(a, b, d)
    for n in (0, 1, 2):
        assert np.all(x[n] == 0.5) and np.all(t[n] == 0.5) and np.all(xr[n] == 0.5) and np.all(tr_[n] == 0.5)
    assert np.all(t[3] == 0.0) and np.all(tr_[3] == 0.0) and rel_l2(x[3], xr[3]) <= 1e-6
    assert np.isfinite(x).all() and np.isfinite(t).all()
    assert rel_l2(x[4:], xr[4:]) <= 1e-6 and rel_l2(t[4:], tr_[4:]) <= 1e-6


# ---- distill
def denoise_crop_exact_means(nn, crop):
    """Micrograph_Autoencoder.denoise_crop at its default arguments with every mean accumulated in float64 and rounded to
    float32 once (numpy's float32 pairwise mean is an ulp off that, and graph S amplifies it: DESIGN.md 3.13)."""
    mean32 = lambda v: np.float32(np.asarray(v, np.float64).mean())
    crop = np.array(crop, np.float32, copy=True)
    offset = np.float32(crop.min())
    scale = np.float32(mean32(crop) - offset)
    crop = (crop - offset) / scale if scale else np.ones_like(crop)
    crop[~np.isfinite(crop)] = 0.0
    lo, hi = crop.min(), crop.max()
    crop = np.full_like(crop, 0.5) if lo == hi else ((crop - lo) / (hi - lo)).astype(np.float32)
    crop = (crop / mean32(crop)).astype(np.float32)
    pred = nn._run(crop[None])[0]
    return scale * pred + offset if scale else pred * offset / mean32(pred)


@pytest.mark.parametrize("enc", [16, 1])
def test_distill_teacher_outputs_match_denoise_crop(enc):
    nn = autoencoder.Micrograph_Autoencoder(encoding_features=enc)
    stack = synthetic_lq(5, 171, 171, seed=40 + enc)[..., 0].astype(np.float32) * 900.0 + 50.0
    stack[3] = 7.5   # a flat crop: denoise_crop's other branch
    crops, outs = KT.teacher_crops(nn, stack, max_batch=2)
    assert np.array_equal(crops.cpu().numpy(), stack[:, :160, :160])
    outs = outs.cpu().numpy()
    for n in range(5):
        host = nn.denoise_crop(stack[n, :160, :160])
        exact = denoise_crop_exact_means(nn, stack[n, :160, :160])
        print(f"enc {enc} image {n}: vs denoise_crop {rel_l2(outs[n], host):.2e}, vs exact means {rel_l2(outs[n], exact):.2e}")
        assert rel_l2(outs[n], host) <= 2e-5
        assert rel_l2(outs[n], exact) <= 1e-6
    # distill = teacher_crops + make_pairs with the same draws
    x, t, d = emdenoise.distill(nn, stack, seed=3, max_batch=3, return_draws=True)
    x2, t2, d2 = emdenoise.make_pairs(crops, torch.from_numpy(outs).to(DEV), seed=3, return_draws=True)
    assert x.shape == (5, 20, 20) and torch.equal(d, d2) and torch.equal(x, x2)
    assert rel_l2(t.cpu().numpy(), t2.cpu().numpy()) <= 1e-6   # the engine's batches differ (3 against 2 per launch)
    with pytest.raises(ValueError):
        emdenoise.distill(nn, stack[:, :150])
    with pytest.raises(ValueError):
        emdenoise.distill(nn, stack, lo=130)


def test_end_to_end_pipeline(tmp_path):
    """autoencoder.py -> autoencoder_train-val-test.py -> noise_removal_kernels_duplicate.py -> apply_kernels+MLPs.py."""
    stack = synthetic_lq(24, 171, 171, seed=77)[..., 0].astype(np.float32)
    s_tr = emdenoise.AutoencoderTrainer(4, device=DEV, seed=1)
    s_tr.train(stack, 3, batch_size=4)
    s_dir = str(tmp_path / "s")
    s_tr.save_checkpoint(s_dir)
    teacher = autoencoder.Micrograph_Autoencoder(checkpoint_loc=s_dir, encoding_features=4)
    x, t = emdenoise.distill(teacher, stack, seed=2)
    assert x.shape == (24, 20, 20) and bool(torch.isfinite(x).all()) and bool(torch.isfinite(t).all())
    tr = emdenoise.KernelDenoiserTrainer(device=DEV, seed=1, **emdenoise.PAIR_PRESET)
    # every step sees the whole stack (batch_size = 24), so the loss of step 1 and the loss at the end are of the same pairs; with
    # one pair per step they are of different pairs and the comparison would be of the pairs, not of the filters
    first = tr.evaluate_pair(x, t)
    hist = tr.train_pairs(x, t, 300, batch_size=24, val_x=x[:8], val_t=t[:8], val_skip_n=100, save_every=200,
                          directory=str(tmp_path / "k"))
    last = tr.evaluate_pair(x, t)
    print("paired loss over the stack, widths 3/5/7:", first, "->", last, " step-1 loss", hist["loss"][0], "step-300", hist["loss"][-1])
    assert hist["loss"].shape == (300, 3) and hist["val_step"].tolist() == [100, 200, 300]
    assert np.array_equal(first, hist["loss"][0])
    assert np.all(last < hist["loss"][0]) and np.all(hist["loss"][-1] < hist["loss"][0])
    k_dir = str(tmp_path / "k")
    assert tr.save_checkpoint(k_dir).endswith("-300")
    img = synthetic_lq(1, 96, 120, seed=5)[0, ..., 0].astype(np.float32)
    for w in (3, 5, 7):
        nn = Micrograph_Autoencoder(k_dir, depth=1, width=w)
        host = Micrograph_Autoencoder(params=tr.params((1, w)), depth=1, width=w)   # the filter rebuilt from the trainer's maps
        got = nn.denoise_images(img)
        assert np.array_equal(nn.params.packed(), tr.params((1, w)).packed())
        assert got.shape == img.shape and np.isfinite(got).all() and np.array_equal(got, host.denoise_images(img))
        assert rel_l2(got, host.denoise(img)) <= 1e-6
    r = emdenoise.KernelDenoiserTrainer(device=DEV, **emdenoise.PAIR_PRESET)
    assert r.restore(k_dir).endswith("-300") and r.step == 300 and r.beta1 == 0.5
    a, b = tr.train_step_pair(x[:4], t[:4]), r.train_step_pair(x[:4], t[:4])
    assert np.array_equal(a, b) and all(torch.equal(fa.theta, fb.theta) for fa, fb in zip(tr.filters, r.filters))
