"""CPU tests of graph K training (emdenoise.k_trainer, csrc/k_train.hip's entry points) that need no GPU:
the float64 restatement of filter_fn and both losses used as the gradient reference of the GPU tests, tied here to the
oracle; the host input path k_record_parser (misc_py/noise-removal-kernels.py:450-538); the learning-rate schedule and
Adam's lr_t; the TF checkpoint written for a trained filter; argument validation of the new entry points."""
import ctypes
import os

import numpy as np
import pytest
import torch

import emdenoise
from emdenoise import _lib, k_trainer as KT, tf_checkpoint
from emdenoise.kernel_denoiser import KernelParams, load_kernel_params
from oracle import kernel_denoiser as KO

from .k_train_ref import ref_forward, ref_loss, ref_loss_and_grad


def theta_of(params):
    """oracle params dict -> theta (float64)."""
    d = params["depth"]
    return np.concatenate([np.asarray(params["w"][l], np.float64) for l in range(d)]
                          + [np.asarray(params["b"][l], np.float64) for l in range(1, d)]
                          + [np.asarray(params["s"][1:], np.float64)])


@pytest.mark.parametrize("depth,width,shape", [(1, 3, (2, 9, 9)), (2, 3, (2, 10, 10)), (3, 5, (1, 11, 8)),
                                               (5, 7, (2, 12, 12)), (4, 15, (1, 16, 17))])
def test_float64_restatement_matches_the_oracle(depth, width, shape):
    params = KO.random_params(depth, width, seed=depth * 31 + width, dtype=np.float64)
    x = np.random.default_rng(5).random(shape)
    got = ref_forward(torch.from_numpy(x), torch.from_numpy(theta_of(params)), depth, width).numpy()
    want = KO.denoise(x[..., None], params, np.float64)[..., 0]
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
    # the reference's loss compares the transposed output with the input (:421-424, :438): for a D4-symmetric filter that is
    # F(x^T) - x, not F(x) - x
    if shape[1] == shape[2]:
        th = torch.from_numpy(theta_of(params))
        lr = float(ref_loss(ref_forward(torch.from_numpy(x), th, depth, width), torch.from_numpy(x), "reference"))
        wantT = KO.denoise(np.ascontiguousarray(x.transpose(0, 2, 1))[..., None], params, np.float64)[..., 0]
        assert abs(lr - float(np.mean((wantT - x) ** 2))) < 1e-12
        li = float(ref_loss(ref_forward(torch.from_numpy(x), th, depth, width), torch.from_numpy(x), "image"))
        assert abs(li - float(np.mean((want - x) ** 2))) < 1e-12


@pytest.mark.parametrize("loss", ["reference", "image"])
def test_per_tap_gradient_equals_whole_graph_autograd(loss):
    depth, width = 3, 5
    params = KO.random_params(depth, width, seed=7, dtype=np.float64)
    x = torch.from_numpy(np.random.default_rng(2).random((2, 9, 9)))
    th = torch.from_numpy(theta_of(params)).requires_grad_(True)
    L = ref_loss(ref_forward(x, th, depth, width), x, loss)
    L.backward()
    l2, g2 = ref_loss_and_grad(x, theta_of(params), depth, width, loss)
    assert abs(float(L.detach()) - l2) < 1e-14
    np.testing.assert_allclose(g2, th.grad.numpy(), rtol=1e-10, atol=1e-14)


# ---- the host input path
def test_k_flip_rotate_elements():
    a = np.arange(12, dtype=np.float32).reshape(3, 4)[:, :3]
    n = 3
    for ch, f in [(0, lambda i, j: a[i, j]), (1, lambda i, j: a[j, n - 1 - i]), (2, lambda i, j: a[n - 1 - i, n - 1 - j]),
                  (3, lambda i, j: a[n - 1 - j, i]), (4, lambda i, j: a[n - 1 - i, j]), (5, lambda i, j: a[i, n - 1 - j]),
                  (6, lambda i, j: a[j, i]), (7, lambda i, j: a[n - 1 - j, n - 1 - i])]:
        want = np.array([[f(i, j) for j in range(n)] for i in range(n)])
        np.testing.assert_array_equal(KT.k_flip_rotate(a, ch), want)
    with pytest.raises(ValueError):
        KT.k_flip_rotate(a, 8)


def test_k_record_parser_draws_and_bounds():
    img = np.random.default_rng(0).random((14, 13)).astype(np.float32)
    crop = 10
    for seed in range(40):
        rng = np.random.default_rng(seed)
        r2 = np.random.default_rng(seed)
        x, y, ch = int(r2.integers(0, 4)), int(r2.integers(0, 3)), int(r2.integers(0, 8))
        got = KT.k_record_parser(img, rng, crop)
        c = KT.k_flip_rotate(img[x:x + crop, y:y + crop], ch)
        c = (c - c.min()) / (c.max() - c.min())
        np.testing.assert_allclose(got, c / c.mean(), rtol=2e-6)
    # randint(0, H - crop) has an exclusive upper bound: every offset in [0, H-crop) occurs, H - crop never does
    xs = set()
    for seed in range(300):
        rng = np.random.default_rng(seed)
        xs.add(int(rng.integers(0, 14 - crop)))
    assert xs == {0, 1, 2, 3}
    with pytest.raises(ValueError):
        KT.k_record_parser(np.zeros((10, 20), np.float32), np.random.default_rng(0), crop)   # H == crop


def test_k_preprocess_special_values():
    # NaN / Inf -> 0 (not the 0.5 of the D' pipeline)
    c = np.full((4, 4), 2.0, np.float32)
    c[0, 0], c[1, 1], c[2, 2] = np.nan, np.inf, -np.inf
    c[3, 3] = 4.0
    out = KT.k_preprocess(c)
    base = np.array(c)
    base[0, 0] = base[1, 1] = base[2, 2] = 0.0
    s = base / 4.0
    np.testing.assert_allclose(out, s / s.mean(), rtol=1e-6)
    # a constant crop: 0.5 after scale0to1, 1.0 after the division by its mean
    np.testing.assert_array_equal(KT.k_preprocess(np.full((5, 5), 3.0, np.float32)), np.ones((5, 5), np.float32))
    np.testing.assert_array_equal(KT.k_crop(np.full((12, 12), 7.0, np.float32), 1, 1, 3, 10), np.ones((10, 10), np.float32))
    # a crop whose range overflows float32 becomes non-finite and record_parser replaces it with zeros
    big = np.random.default_rng(1).random((12, 12)).astype(np.float32)
    big[2, 2], big[3, 3] = 3e38, -3e38
    with np.errstate(over="ignore", invalid="ignore"):
        np.testing.assert_array_equal(KT.k_crop(big, 0, 0, 0, 10), np.zeros((10, 10), np.float32))


# ---- schedule
def test_lr_schedule_and_adam_lr_t():
    assert KT.lr_schedule(1) == pytest.approx(0.005 * (1 - 1 / 20001), rel=1e-15)
    assert KT.lr_schedule(20000) == pytest.approx(0.005 / 20001, rel=1e-12)
    assert KT.lr_schedule(50, lr0=0.01, total_steps=99) == pytest.approx(0.01 * 0.5, rel=1e-15)
    assert KT.adam_lr_t(1.0, 1) == pytest.approx(np.sqrt(0.001) / 0.1, rel=1e-14)
    t = 37
    assert KT.adam_lr_t(0.003, t) == pytest.approx(0.003 * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t), rel=1e-14)
    assert KT.adam_lr_t(0.003, t, 0.5, 0.9) == pytest.approx(0.003 * np.sqrt(1 - 0.9 ** t) / (1 - 0.5 ** t), rel=1e-14)


# ---- parameters and checkpoints
def test_theta_round_trip_and_initial_values():
    p = KT.initial_params(4, 7, np.random.default_rng(3))
    assert p.symmetric
    np.testing.assert_array_equal(p.wmaps, np.full((4, 7, 7), 1 / 49, np.float32))
    np.testing.assert_array_equal(p.bmaps, 0)
    assert p.s[0] == 1 and np.all(np.abs(p.s[1:]) <= np.sqrt(3)) and len(set(p.s[1:].tolist())) == 3
    th = KT.theta_from_params(p)
    assert th.shape == (KT.scalar_count(4, 7),) == (7 * 10 + 3,)
    np.testing.assert_array_equal(KT.params_from_theta(th, 4, 7).packed(), p.packed())
    w = np.arange(9, dtype=np.float32).reshape(1, 3, 3)
    with pytest.raises(ValueError):
        KT.theta_from_params(KernelParams(w, np.zeros_like(w), np.ones(1, np.float32)))


def test_checkpoint_bundle_round_trip_and_npz_equivalence(tmp_path):
    rng = np.random.default_rng(11)
    filters = []
    for (d, w) in [(2, 3), (3, 5)]:
        n = KT.scalar_count(d, w)
        filters.append((d, w, rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32),
                        rng.random(n).astype(np.float32)))
    sd = KT.kernel_state_dict(filters, step=123)
    prefix = os.path.join(str(tmp_path / "model"), "") + "-123"
    tf_checkpoint.write_checkpoint(prefix, sd)
    assert tf_checkpoint.latest_checkpoint(str(tmp_path / "model")) == prefix
    back = tf_checkpoint.read_checkpoint(prefix)
    assert set(back) == set(sd)
    for k in sd:
        assert back[k].dtype == np.float32 and back[k].shape == np.asarray(sd[k]).shape
        np.testing.assert_array_equal(back[k], sd[k])
    assert back["depth-2_size-3/fully_connected/weights"].shape == (1, 1)
    assert "depth-3_size-5/fully_connected_1/weights/Adam_1" in back
    assert back["beta1_power"] == np.float32(0.9 ** 123) and back["beta2_power_1"] == np.float32(0.999 ** 123)
    # the apply side: the bundle and an .npz of the same names give identical maps
    for (d, w, theta, _, _) in filters:
        names = KT.tf_names(d, w)
        npz_dir = tmp_path / f"npz_{d}_{w}"
        npz_dir.mkdir()
        np.savez(npz_dir / f"kernel_params_depth-{d}_size-{w}.npz", **{n: sd[n] for n in names})
        a = load_kernel_params(str(tmp_path / "model"), d, w)
        b = load_kernel_params(str(npz_dir), d, w)
        np.testing.assert_array_equal(a.packed(), b.packed())
        np.testing.assert_array_equal(a.packed(), KT.params_from_theta(theta, d, w).packed())
    with pytest.raises(FileNotFoundError):
        load_kernel_params(str(tmp_path / "nothing"), 2, 3)


# ---- argument validation (before any launch: runs without a GPU)
def test_trainer_rejects_bad_configs():
    for cfg in [(2, 17), (6, 3), (0, 3), (2, 4), (2, 1)]:
        with pytest.raises(ValueError):
            emdenoise.KernelDenoiserTrainer(configs=[cfg])
    with pytest.raises(ValueError):
        emdenoise.KernelDenoiserTrainer(configs=[(2, 3)], loss="l1")
    with pytest.raises(ValueError):
        emdenoise.KernelDenoiserTrainer(configs=[(2, 3), (2, 3)])


def test_entry_points_validate_arguments_without_a_gpu():
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    null = ctypes.c_void_p(0)
    assert lib.emd_k_train_scalar_count(3, 2) == 10
    assert lib.emd_k_train_scalar_count(15, 5) == 9 * 36 + 4
    assert lib.emd_k_train_scalar_count(17, 2) == 0 and lib.emd_k_train_scalar_count(3, 6) == 0
    ws = lib.emd_k_train_workspace_bytes(32, 10, 10, 3, 2)
    assert ws == 4 * 11 * 4   # 3200 pixels: four chunks of 1024, 10 scalars + the loss each
    assert lib.emd_k_train_workspace_bytes(32, 512, 512, 3, 2) == 1024 * 11 * 4

    def step(x=p, B=32, H=10, W=10, width=3, depth=2, mode=0, theta=p, m=p, v=p, stepc=p, flags=1, wsp=p, wsb=1 << 20):
        return lib.emd_k_train_step_f32(x, B, H, W, width, depth, mode, theta, m, v, stepc, ctypes.c_double(0.005), 20000,
                                        0.9, 0.999, 1e-8, flags, None, None, None, wsp, wsb, null)

    for kw, what in [(dict(width=17), b"width"), (dict(depth=6), b"depth"), (dict(depth=0), b"depth"), (dict(width=4), b"width"),
                     (dict(x=null), b"null"), (dict(theta=null), b"null"), (dict(wsp=null), b"null"), (dict(m=null), b"null"),
                     (dict(stepc=null), b"null"), (dict(H=10, W=12), b"square"), (dict(mode=2), b"loss"),
                     (dict(H=1, W=1), b"REFLECT"), (dict(wsb=16), b"workspace"), (dict(flags=3), b"gradient"),
                     (dict(flags=8), b"flag"), (dict(B=0), b"shape")]:
        assert step(**kw) == -1, kw
        assert what in lib.emd_last_error(), (kw, lib.emd_last_error())
    # without UPDATE the Adam state may be NULL; the image loss takes non-square batches -- these get past validation
    # only up to the workspace check here (16 bytes), which proves they were not refused for those reasons
    assert step(H=10, W=12, mode=1, wsb=16) == -1 and b"workspace" in lib.emd_last_error()
    assert step(m=null, v=null, stepc=null, flags=0, wsb=16) == -1 and b"workspace" in lib.emd_last_error()

    def sample(stack=p, N=4, H=20, W=20, crops=p, B=32, crop=10):
        return lib.emd_k_sample_crops_f32(stack, N, H, W, crops, B, crop, 1, 0, None, null)

    for kw, what in [(dict(crop=20), b"crop"), (dict(crop=25), b"crop"), (dict(W=10), b"crop"), (dict(stack=null), b"null"),
                     (dict(crops=null), b"null"), (dict(N=0), b"shape"), (dict(B=0), b"shape")]:
        assert sample(**kw) == -1, kw
        assert what in lib.emd_last_error(), (kw, lib.emd_last_error())


def test_fused_entry_point_validates_arguments_without_a_gpu():
    lib = _lib.load()
    p = 4096
    null = ctypes.c_void_p(0)

    def call(width=3, depth=2, njobs=1, jobs_null=False, B=32, crop=10, H=20, W=20, nsteps=10, stack=p, mode=0, theta=p):
        jobs = (_lib.KFusedJob * 1)(_lib.KFusedJob(theta, p, p, p, 0, p, width, depth))
        return lib.emd_k_train_fused_f32(None if jobs_null else jobs, njobs, ctypes.c_void_p(stack), 4, H, W, None, 0, B, crop,
                                         1, nsteps, mode, ctypes.c_double(0.005), 20000, 0.9, 0.999, 1e-8, null)

    for kw, what in [(dict(jobs_null=True), b"null"), (dict(njobs=0), b"jobs"), (dict(nsteps=0), b"nsteps"),
                     (dict(nsteps=1001), b"nsteps"), (dict(B=33, crop=16), b"LDS"), (dict(width=17), b"width"),
                     (dict(depth=6), b"depth"), (dict(crop=20), b"crop"), (dict(stack=0), b"null"), (dict(theta=0), b"null"),
                     (dict(mode=3), b"loss"), (dict(width=15, crop=7, H=10, W=10), b"REFLECT")]:
        assert call(**kw) < 0, kw
        assert what in lib.emd_last_error(), (kw, lib.emd_last_error())
    assert KT.KernelDenoiserTrainer.fused_allowed(32, 16) and not KT.KernelDenoiserTrainer.fused_allowed(33, 16)


def test_trainer_host_checks_before_any_launch(tmp_path):
    """Checks that run before anything reaches the device (a CPU-resident trainer: no launch is made)."""
    tr = emdenoise.KernelDenoiserTrainer([(2, 3)], device="cpu", total_steps=100)
    stack = np.random.default_rng(0).random((2, 20, 20)).astype(np.float32)
    with pytest.raises(ValueError, match="val_skip_n"):
        tr.train(stack, 5, val_stack=stack, val_skip_n=0)
    with pytest.raises(ValueError, match="total_steps"):
        tr.train(stack, 101)
    with pytest.raises(ValueError, match="global_step"):
        tr.save_checkpoint(str(tmp_path / "a"), 7)
    assert tr.step == 0


def test_restore_takes_the_step_from_the_beta_powers(tmp_path):
    assert KT.step_from_beta_powers(0.9 ** 123, 0.999 ** 123) == 123
    assert KT.step_from_beta_powers(0.0, float(np.float32(0.999 ** 20000))) == 20000
    assert KT.step_from_beta_powers(0.0, 0.0) is None
    with pytest.raises(ValueError):
        KT.step_from_beta_powers(0.9 ** 10, 0.999 ** 123)
    n = KT.scalar_count(2, 3)
    rng = np.random.default_rng(1)
    sd = KT.kernel_state_dict([(2, 3, rng.random(n), rng.random(n), rng.random(n))], step=123)
    tf_checkpoint.write_checkpoint(os.path.join(str(tmp_path / "ok"), "") + "-123", sd)
    tr = emdenoise.KernelDenoiserTrainer([(2, 3)], device="cpu")
    tr.restore(str(tmp_path / "ok"))
    assert tr.step == 123 and int(tr.filters[0].step[0]) == 123
    np.testing.assert_array_equal(tr.filters[0].theta.numpy(), np.asarray(sd["depth-2_size-3/w0/var_x-0_y-0/v"]).reshape(-1)[:1].tolist()
                                  + [float(np.asarray(sd[k]).reshape(-1)[0]) for k in KT.tf_names(2, 3)[1:]])
    tf_checkpoint.write_checkpoint(os.path.join(str(tmp_path / "bad"), "") + "-124", sd)   # name and Adam state disagree
    with pytest.raises(ValueError, match="beta powers"):
        tr.restore(str(tmp_path / "bad"))
