"""GPU tests of graph K training (csrc/k_train.hip through emdenoise.k_trainer) against the float64 restatement of the
reference's objective (tests/k_train_ref.py, tied to the oracle by tests/test_k_train.py): loss and gradients, Adam
trajectories against a float64 restatement of TF's AdamOptimizer, determinism, the device crop sampler against
k_record_parser's arithmetic, and train() -> checkpoint -> Micrograph_Autoencoder end to end."""
import numpy as np
import pytest
import torch

import emdenoise
from emdenoise import k_trainer as KT
from emdenoise.kernel_denoiser import KernelParams, Micrograph_Autoencoder, kernel_denoise
from oracle import kernel_denoiser as KO

from .k_train_ref import ref_loss_and_grad
from .synth_inputs import synthetic_lq

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
BAR = 2e-5


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def rand_params(depth, width, seed):
    return KernelParams(*KO.full_maps(KO.random_params(depth, width, seed=seed)))


def batch(shape, seed):
    """Positive, mean-normalised crops like the input path produces."""
    x = synthetic_lq(shape[0], shape[1], shape[2], seed=seed)[..., 0].astype(np.float64)
    x = x / np.maximum(x.mean(axis=(1, 2), keepdims=True), 1e-9)
    return x.astype(np.float32)


def check_grad(shape, depth, width, loss, bar=BAR, seed=0):
    x = batch(shape, seed=1000 + depth * 17 + width)
    p = rand_params(depth, width, seed=depth * 100 + width + seed)
    tr = emdenoise.KernelDenoiserTrainer([(depth, width)], device=DEV, loss=loss, initial=[p])
    L, g = tr.loss_and_grad(x)
    xd = torch.from_numpy(x).to(DEV, torch.float64)
    Lr, gr = ref_loss_and_grad(xd, KT.theta_from_params(p), depth, width, loss)
    assert abs(L - Lr) <= bar * abs(Lr), (L, Lr)
    assert rel_l2(g, gr) <= bar, rel_l2(g, gr)


@pytest.mark.parametrize("loss", ["reference", "image"])
@pytest.mark.parametrize("width", [3, 5, 7, 15])
@pytest.mark.parametrize("depth", [1, 2, 3, 4, 5])
def test_grad_32x10x10(depth, width, loss):
    check_grad((32, 10, 10), depth, width, loss)


@pytest.mark.parametrize("width", [3, 5, 7])
@pytest.mark.parametrize("depth", [1, 2, 3, 4, 5])
def test_grad_nonsquare_3x7x13(depth, width):
    check_grad((3, 7, 13), depth, width, "image")


@pytest.mark.parametrize("loss", ["reference", "image"])
@pytest.mark.parametrize("width", [3, 5, 7, 15])
@pytest.mark.parametrize("depth", [1, 2, 3, 4, 5])
def test_grad_2x512x512(depth, width, loss):
    check_grad((2, 512, 512), depth, width, loss)


def test_grad_32x512x512_reference_config():
    check_grad((32, 512, 512), 2, 3, "reference", bar=1e-4)


def test_kat_box_filter_on_a_constant_image():
    """depth 1 at the initial weights is a w x w box mean (KAT #1): a constant image is a fixed point, loss 0, gradient 0."""
    for width in (3, 7, 15):
        tr = emdenoise.KernelDenoiserTrainer([(1, width)], device=DEV, initial=[KernelParams.initial(1, width)])
        L, g = tr.loss_and_grad(np.ones((4, 16, 16), np.float32))
        # exact up to float32: O is a float32 sum of w^2 terms fl(1/w^2); their representation and the w^2 roundings of the
        # sum each stay within 2^-24, so |O - 1| <= 2 w^2 2^-24 = e; the loss is at most e^2 and a scalar's gradient,
        # 2 (O - 1) summed over its <= 8 taps, at most 16 e
        e = 2 * width * width * 2.0 ** -24
        assert abs(L) <= e * e and np.abs(g).max() <= 16 * e, (width, L, np.abs(g).max())


def test_step_is_bitwise_deterministic():
    x = batch((8, 171, 171), seed=3)
    runs = []
    for _ in range(2):
        tr = emdenoise.KernelDenoiserTrainer([(3, 5), (2, 3)], device=DEV, seed=4)
        lg = tr.loss_and_grad(x, (3, 5))
        losses = [tr.train_step(x) for _ in range(5)]
        runs.append((lg, losses, [f.theta.cpu().numpy() for f in tr.filters]))
    (l0, g0), L0, T0 = runs[0]
    (l1, g1), L1, T1 = runs[1]
    assert l0 == l1 and np.array_equal(g0, g1)
    assert all(np.array_equal(a, b) for a, b in zip(L0, L1))
    assert all(np.array_equal(a, b) for a, b in zip(T0, T1))


def test_device_params_block_matches_the_host_expansion():
    tr = emdenoise.KernelDenoiserTrainer([(3, 7)], device=DEV, seed=1)
    tr.train_step(batch((4, 20, 20), seed=9))
    assert np.array_equal(tr.packed_params().cpu().numpy(), tr.params().packed())


def test_adam_trajectory_matches_float64_tf_adam():
    """50 steps on fixed batches, two filters with their own Adam on the same batches, against TF's AdamOptimizer restated in
    float64 (lr = lr0 (1 - t/(T+1)), lr_t = lr sqrt(1-b2^t)/(1-b1^t), m/(sqrt(v)+eps))."""
    configs = [(2, 3), (3, 5)]
    batches = [batch((32, 10, 10), seed=50 + k) for k in range(5)]
    tr = emdenoise.KernelDenoiserTrainer(configs, device=DEV, seed=7)
    th0 = [KT.theta_from_params(tr.params(c)).astype(np.float64) for c in configs]
    got = np.array([tr.train_step(batches[t % 5]) for t in range(50)])
    for i, (d, w) in enumerate(configs):
        th, m, v = th0[i].copy(), np.zeros_like(th0[i]), np.zeros_like(th0[i])
        want = []
        for t in range(1, 51):
            L, g = ref_loss_and_grad(torch.from_numpy(batches[(t - 1) % 5]).double(), th, d, w, "reference")
            want.append(L)
            lr_t = KT.adam_lr_t(KT.lr_schedule(t, 0.005, 20000), t, 0.9, 0.999)
            m = 0.9 * m + 0.1 * g
            v = 0.999 * v + 0.001 * g * g
            th = th - lr_t * m / (np.sqrt(v) + 1e-8)
        want = np.array(want)
        assert np.max(np.abs(got[:, i] - want) / want) <= 1e-4, np.max(np.abs(got[:, i] - want) / want)
        assert rel_l2(KT.theta_from_params(tr.params((d, w))), th) <= 1e-4
        assert want[-1] < want[0]


def test_sampler_matches_k_record_parser():
    N, H, W, crop, B = 6, 40, 37, 10, 4096
    rng = np.random.default_rng(21)
    stack = rng.random((N, H, W)).astype(np.float32) * 3.0
    stack[1] = 3.0                                          # constant image: every crop -> 0.5 -> 1.0
    stack[2, 5, 5], stack[2, 20, 30], stack[2, 33, 2] = np.nan, np.inf, -np.inf   # NaN / Inf -> 0
    stack[3, 15, 15], stack[3, 16, 16] = 3e38, -3e38       # crops holding both overflow: all zeros
    sd = torch.from_numpy(stack).to(DEV)
    draws = torch.empty((B, 4), dtype=torch.int32, device=DEV)
    crops = KT.sample_crops(sd, B, crop, seed=5, first_index=0, draws=draws).cpu().numpy()
    again = KT.sample_crops(sd, B, crop, seed=5, first_index=0).cpu().numpy()
    assert np.array_equal(crops, again)
    dr = draws.cpu().numpy()
    nzero = 0
    with np.errstate(over="ignore", invalid="ignore"):
        for b in range(B):
            n, x, y, ch = (int(v) for v in dr[b])
            want = KT.k_crop(stack[n], x, y, ch, crop)
            if not want.any():
                nzero += 1
                assert not crops[b].any(), b
            else:
                np.testing.assert_allclose(crops[b], want, rtol=2e-6, atol=1e-6, err_msg=str(dr[b]))
    assert nzero > 0
    assert set(dr[:, 0].tolist()) == set(range(N))
    assert set(dr[:, 1].tolist()) == set(range(H - crop))
    assert set(dr[:, 2].tolist()) == set(range(W - crop))
    assert set(dr[:, 3].tolist()) == set(range(8))
    # the stream is keyed by the crop's index: batch t of size 32 is crops t*32 .. t*32+31 of one long stream
    part = KT.sample_crops(sd, 32, crop, seed=5, first_index=64).cpu().numpy()
    assert np.array_equal(part, crops[64:96])


def test_train_end_to_end_checkpoint_apply_and_resume(tmp_path):
    stack = synthetic_lq(8, 48, 48, seed=31)[..., 0]
    val = synthetic_lq(4, 48, 48, seed=32)[..., 0]
    tr = emdenoise.KernelDenoiserTrainer([(2, 3), (1, 5)], device=DEV, seed=3)
    res = tr.train(stack, 500, batch_size=32, crop=10, val_stack=val, chunk=200)
    assert res["loss"].shape == (500, 2) and np.all(np.isfinite(res["loss"]))
    assert list(res["val_step"]) == list(range(10, 501, 10))
    vl = res["val_loss"]
    assert np.all(vl[-5:].mean(axis=0) < vl[:5].mean(axis=0)), vl
    prefix = tr.save_checkpoint(str(tmp_path))
    assert prefix.endswith("-500")
    # the apply side reads the TF checkpoint
    x = torch.from_numpy(synthetic_lq(2, 64, 64, seed=33)).to(DEV)
    for (d, w) in [(2, 3), (1, 5)]:
        ma = Micrograph_Autoencoder(ckpt_loc=str(tmp_path), depth=d, width=w)
        p = tr.params((d, w))
        want = kernel_denoise(x, torch.from_numpy(p.packed()).to(DEV), w, d, p.symmetric)
        assert torch.equal(ma.denoise_batch(x), want)
    # resume: restore + 10 steps == 10 more uninterrupted steps
    cont = tr.train(stack, 10, batch_size=32, crop=10)["loss"]
    tr2 = emdenoise.KernelDenoiserTrainer([(2, 3), (1, 5)], device=DEV, seed=3)
    tr2.restore(str(tmp_path))
    assert tr2.step == 500
    res2 = tr2.train(stack, 10, batch_size=32, crop=10)["loss"]
    assert np.array_equal(cont, res2)
    for c in [(2, 3), (1, 5)]:
        assert np.array_equal(tr.params(c).packed(), tr2.params(c).packed())
        assert np.array_equal(tr._filter(c).m.cpu().numpy(), tr2._filter(c).m.cpu().numpy())


# ---- (c) the fused small-batch launch
def test_fused_trajectory_matches_tf_adam_and_the_eager_form():
    """50 fused steps on the fixed batches of the eager trajectory test: against the float64 TF-Adam restatement (1e-4) and
    against the eager form (a) (sums in another order: agreement to rounding, not bits)."""
    configs = [(2, 3), (3, 5)]
    batches = np.stack([batch((32, 10, 10), seed=50 + k) for k in range(5)])
    fz = emdenoise.KernelDenoiserTrainer(configs, device=DEV, seed=7)
    ea = emdenoise.KernelDenoiserTrainer(configs, device=DEV, seed=7)
    th0 = [KT.theta_from_params(fz.params(c)).astype(np.float64) for c in configs]
    got = np.concatenate([fz.train_fused(batches, 30), fz.train_fused(batches, 20)])   # two launches: the batch cycle continues
    eag = np.array([ea.train_step(batches[t % 5]) for t in range(50)])
    assert fz.step == 50 and int(fz.filters[0].step.item()) == 50
    for i, (d, w) in enumerate(configs):
        th, m, v = th0[i].copy(), np.zeros_like(th0[i]), np.zeros_like(th0[i])
        want = []
        for t in range(1, 51):
            L, g = ref_loss_and_grad(torch.from_numpy(batches[(t - 1) % 5]).double(), th, d, w, "reference")
            want.append(L)
            lr_t = KT.adam_lr_t(KT.lr_schedule(t, 0.005, 20000), t, 0.9, 0.999)
            m = 0.9 * m + 0.1 * g
            v = 0.999 * v + 0.001 * g * g
            th = th - lr_t * m / (np.sqrt(v) + 1e-8)
        want = np.array(want)
        assert np.max(np.abs(got[:, i] - want) / want) <= 1e-4
        assert rel_l2(KT.theta_from_params(fz.params((d, w))), th) <= 1e-4
        assert np.max(np.abs(got[:, i] - eag[:, i]) / eag[:, i]) <= 1e-4
        assert rel_l2(KT.theta_from_params(fz.params((d, w))), KT.theta_from_params(ea.params((d, w)))) <= 1e-4
        # the packed inference block written by the fused launch is the expansion of its theta
        assert np.array_equal(fz.packed_params((d, w)).cpu().numpy(), fz.params((d, w)).packed())


def test_fused_is_bitwise_deterministic_and_agrees_with_sampler_plus_step():
    stack = synthetic_lq(6, 40, 40, seed=41)[..., 0]
    configs = [(2, 3), (4, 7), (1, 5)]
    runs = []
    for _ in range(2):
        tr = emdenoise.KernelDenoiserTrainer(configs, device=DEV, seed=9)
        res = tr.train(stack, 40, fused=True)
        runs.append((res["loss"], [tr.params(c).packed() for c in configs]))
    assert np.array_equal(runs[0][0], runs[1][0])
    assert all(np.array_equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
    ea = emdenoise.KernelDenoiserTrainer(configs, device=DEV, seed=9)
    le = ea.train(stack, 40, fused=False)["loss"]
    assert np.max(np.abs(runs[0][0] - le) / le) <= 1e-4
    for k, c in enumerate(configs):
        assert rel_l2(runs[0][1][k], ea.params(c).packed()) <= 1e-4


def test_fused_train_validation_cadence_and_resume(tmp_path):
    stack = synthetic_lq(6, 40, 40, seed=42)[..., 0]
    val = synthetic_lq(3, 40, 40, seed=43)[..., 0]
    tr = emdenoise.KernelDenoiserTrainer([(2, 3)], device=DEV, seed=5)
    res = tr.train(stack, 35, val_stack=val, val_skip_n=10, fused=True)
    assert list(res["val_step"]) == [10, 20, 30] and res["loss"].shape == (35, 1)
    tr.save_checkpoint(str(tmp_path))
    cont = tr.train(stack, 12, fused=True)["loss"]
    tr2 = emdenoise.KernelDenoiserTrainer([(2, 3)], device=DEV, seed=5)
    tr2.restore(str(tmp_path))
    assert np.array_equal(tr2.train(stack, 12, fused=True)["loss"], cont)
