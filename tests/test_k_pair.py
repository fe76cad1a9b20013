"""CPU tests of graph K's paired training surface (emdenoise.k_trainer: train_pairs, make_pairs, distill, PAIR_PRESET): the
float64 restatement (tests/k_pair_ref.py) pinned by a literal per-pixel loop, train_pairs' walking order on a mock step, the
preset's schedule, checkpoints at beta1 = 0.5, and the argument checks that run before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import emdenoise
from emdenoise import _lib
from emdenoise import k_trainer as KT
from emdenoise.kernel_denoiser import KernelParams
from oracle import kernel_denoiser as KO

from . import k_pair_ref as R

CPU = torch.device("cpu")


def rand_theta(depth, width, seed):
    return KT.theta_from_params(KernelParams(*KO.full_maps(KO.random_params(depth, width, seed=seed)))).astype(np.float64)


@pytest.mark.parametrize("pad", ["valid", "reflect"])
@pytest.mark.parametrize("depth,width", [(1, 3), (2, 3), (3, 5)])
def test_restatement_matches_the_literal_loop(depth, width, pad):
    rng = np.random.default_rng(depth * 10 + width)
    x, t = rng.random((2, 7, 9)), rng.random((2, 7, 9))
    th = rand_theta(depth, width, 5)
    for scale in (1.0, 40.0):   # 40: the MSE is far above 1, the sqrt branch
        for rule in (True, False):
            L, g, mse = R.pair_loss_and_grad(x, t * scale, th, depth, width, pad, rule)
            want = R.pair_loss_loop(x, t * scale, th, depth, width, pad, rule)
            assert abs(L - want) <= 1e-12 * abs(want), (L, want)
            assert (mse > 2.0) == (scale == 40.0) and (L == mse) == (not (rule and mse > 1.0))


def test_restatement_gradient_against_central_differences():
    rng = np.random.default_rng(3)
    x, t = rng.random((2, 8, 8)), rng.random((2, 8, 8)) * 30.0
    th = rand_theta(2, 3, 9)
    L, g, mse = R.pair_loss_and_grad(x, t, th, 2, 3, "valid", True)
    assert mse > 2.0
    for k in range(len(th)):
        e = np.zeros_like(th)
        e[k] = 1e-6
        num = (R.pair_loss_loop(x, t, th + e, 2, 3) - R.pair_loss_loop(x, t, th - e, 2, 3)) / 2e-6
        assert abs(num - g[k]) <= 1e-7 * max(1.0, abs(g[k])), (k, num, g[k])


def test_valid_interior_is_the_centre_of_the_reflect_output():
    rng = np.random.default_rng(1)
    x = torch.from_numpy(rng.random((1, 9, 11)))
    th = torch.from_numpy(rand_theta(2, 5, 2))
    full = R.pair_forward(x, th, 2, 5, "reflect")
    assert torch.allclose(R.pair_forward(x, th, 2, 5, "valid"), full[:, 2:-2, 2:-2], rtol=0, atol=1e-15)


def test_pair_order_walks_in_order_and_wraps():
    assert KT.pair_order(5, 0, 7).ravel().tolist() == [0, 1, 2, 3, 4, 0, 1]
    assert KT.pair_order(5, 3, 3).ravel().tolist() == [3, 4, 0]
    assert KT.pair_order(5, 1, 3, batch_size=2).tolist() == [[2, 3], [4, 0], [1, 2]]


def _mock_trainer(monkeypatch, **kw):
    tr = emdenoise.KernelDenoiserTrainer(device=CPU, **kw)
    seen = []

    def step(x, truth, pad_mode, flags, buf, k):
        seen.append((x.clone().numpy(), truth.clone().numpy(), pad_mode, flags))
        buf[k] = float(len(seen))

    monkeypatch.setattr(tr, "_pair_step", step)
    monkeypatch.setattr(tr, "save_checkpoint", lambda d: seen.append(("save", d, tr.step)))
    return tr, seen


def test_train_pairs_walking_order_on_a_mock_step(monkeypatch):
    tr, seen = _mock_trainer(monkeypatch, **KT.PAIR_PRESET)
    xs = np.arange(5, dtype=np.float32)[:, None, None] * np.ones((5, 20, 20), np.float32)
    ts = xs + 100
    res = tr.train_pairs(xs, ts, 7, chunk=3)
    assert [s[0][0, 0, 0] for s in seen] == [0, 1, 2, 3, 4, 0, 1] and [s[1][0, 0, 0] for s in seen] == [100, 101, 102, 103, 104, 100, 101]
    assert all(s[0].shape == (1, 20, 20) for s in seen)
    assert all(s[2] == KT.EMD_K_PAD_VALID and s[3] == KT.EMD_K_TRAIN_UPDATE | KT.EMD_K_TRAIN_SQRT_ABOVE_1 for s in seen)
    assert res["loss"].shape == (7, 3) and res["loss"][:, 0].tolist() == [1, 2, 3, 4, 5, 6, 7] and tr.step == 7
    # a second call goes on where the first stopped; a batch that wraps round the end is gathered
    del seen[:]
    tr.train_pairs(xs, ts, 2, batch_size=2, pad="reflect", sqrt_above_1=False)
    assert [s[0][:, 0, 0].tolist() for s in seen] == [[4, 0], [1, 2]] and [s[1][:, 0, 0].tolist() for s in seen] == [[104, 100], [101, 102]]
    assert all(s[2] == KT.EMD_K_PAD_REFLECT and s[3] == KT.EMD_K_TRAIN_UPDATE for s in seen)


def test_train_pairs_validation_saves_and_shuffle(monkeypatch):
    tr, seen = _mock_trainer(monkeypatch, **KT.PAIR_PRESET)
    xs = np.arange(4, dtype=np.float32)[:, None, None] * np.ones((4, 20, 20), np.float32)
    res = tr.train_pairs(xs, xs, 6, val_x=xs[:2] + 50, val_t=xs[:2], val_skip_n=3, save_every=4, directory="d")
    is_save = lambda s: isinstance(s[0], str)
    kinds = ["save" if is_save(s) else ("val" if s[0][0, 0, 0] >= 50 else "train") for s in seen]
    assert kinds == ["train"] * 3 + ["val", "train", "save", "train", "train", "val"]
    assert res["val_step"].tolist() == [3, 6] and res["val_loss"].shape == (2, 3)
    assert [s for s in seen if is_save(s)] == [("save", "d", 4)]
    assert all(s[3] == KT.EMD_K_TRAIN_LOSS_ONLY | KT.EMD_K_TRAIN_SQRT_ABOVE_1 for s in seen if not is_save(s) and s[0][0, 0, 0] >= 50)
    # shuffle: one fixed permutation, every pair once per round
    tr2, seen2 = _mock_trainer(monkeypatch, seed=3, **KT.PAIR_PRESET)
    tr2.train_pairs(xs, xs, 8, shuffle=True)
    order = [int(s[0][0, 0, 0]) for s in seen2]
    assert sorted(order[:4]) == [0, 1, 2, 3] and order[4:] == order[:4]


def test_preset_schedule_values():
    p = KT.PAIR_PRESET
    assert p["configs"] == ((1, 3), (1, 5), (1, 7)) and p["beta1"] == 0.5 and KT.PAIR_PATCH == 20
    for t in (1, 5000, 10000):
        assert KT.lr_schedule(t, p["lr0"], p["total_steps"]) == pytest.approx(0.01 * (1 - t / 10001), rel=1e-15)
    assert KT.lr_schedule(10000, p["lr0"], p["total_steps"]) > 0
    tr = emdenoise.KernelDenoiserTrainer(device=CPU, **p)
    assert (tr.lr0, tr.total_steps, tr.beta1, tr.configs) == (0.01, 10000, 0.5, [(1, 3), (1, 5), (1, 7)])
    with pytest.raises(ValueError):
        tr.step = 10000
        tr.train_pairs(np.zeros((2, 20, 20), np.float32), np.zeros((2, 20, 20), np.float32), 1)


@pytest.mark.parametrize("step", [1, 50, 126, 127, 149, 150, 200, 5000, 10000])
def test_checkpoint_round_trip_at_beta1_half(tmp_path, step):
    """beta1^t at beta1 = 0.5 leaves float32's normal range at t = 127 and is zero from t = 150: the step then comes from beta2^t."""
    assert KT.step_from_beta_powers(float(np.float32(0.5 ** step)), float(np.float32(0.999 ** step)), 0.5, 0.999) == step
    tr = emdenoise.KernelDenoiserTrainer(device=CPU, seed=2, **KT.PAIR_PRESET)
    tr.step = step
    for f in tr.filters:
        f.m.uniform_(-1, 1)
        f.v.uniform_(0, 1)
        f.theta.uniform_(-1, 1)
    d = str(tmp_path / "ck")
    assert tr.save_checkpoint(d).endswith(f"-{step}")
    r = emdenoise.KernelDenoiserTrainer(device=CPU, **KT.PAIR_PRESET)
    r.restore(d)
    assert r.step == step and all(int(f.step.item()) == step for f in r.filters)
    for a, b in zip(tr.filters, r.filters):
        assert torch.equal(a.theta, b.theta) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v)
    # a trainer that assumes another beta1 refuses the checkpoint while the beta1 power still says something
    if step in (50, 126):
        with pytest.raises(ValueError):
            emdenoise.KernelDenoiserTrainer(device=CPU, configs=KT.PAIR_PRESET["configs"]).restore(d)


def test_python_argument_checks():
    tr = emdenoise.KernelDenoiserTrainer(device=CPU, configs=((1, 3), (1, 7)), lr0=0.01, total_steps=10000, beta1=0.5)
    z = lambda *s: np.zeros(s, np.float32)
    with pytest.raises(ValueError, match="width <= min"):       # width 7 > min(H, W) = 6 under VALID
        tr.train_step_pair(z(1, 6, 9), z(1, 6, 9))
    with pytest.raises(ValueError, match="width <= min"):
        tr.loss_and_grad_pair(z(1, 6, 9), z(1, 6, 9), (1, 7))
    with pytest.raises(ValueError, match="differ in shape"):
        tr.evaluate_pair(z(1, 8, 8), z(1, 8, 9))
    with pytest.raises(ValueError, match="pad must be"):
        tr.train_step_pair(z(1, 8, 8), z(1, 8, 8), pad="same")
    with pytest.raises(ValueError, match="3 and 4 pairs"):      # stacks of unequal length
        tr.train_pairs(z(3, 20, 20), z(4, 20, 20), 1)
    with pytest.raises(ValueError, match="save_every"):
        tr.train_pairs(z(3, 20, 20), z(3, 20, 20), 1, save_every=5)
    with pytest.raises(ValueError, match="come together"):
        tr.train_pairs(z(3, 20, 20), z(3, 20, 20), 1, val_x=z(1, 20, 20))
    assert tr.step == 0
    # the patch window
    assert KT.check_pair_window(160, 20, 20, None) == 120          # randint(20, 160 - 20 - 20)
    with pytest.raises(ValueError, match="empty"):
        KT.check_pair_window(160, 20, 20, 20)                       # hi <= lo
    with pytest.raises(ValueError, match="empty"):
        KT.check_pair_window(50, 20, 20, None)                      # the default hi = 10 <= lo
    with pytest.raises(ValueError, match="does not fit"):
        KT.check_pair_window(160, 20, 20, 142)
    assert KT.check_pair_window(160, 20, 0, 141) == 141


def test_library_argument_checks_need_no_gpu():
    lib = _lib.load()
    one, null = ctypes.c_void_p(16), ctypes.c_void_p(0)
    big = ctypes.c_size_t(1 << 30)

    def step(H, W, width, pad, flags=0, truth=one):
        return lib.emd_k_train_pair_step_f32(one, truth, 1, H, W, width, 1, pad, one, one, one, one, ctypes.c_double(0.01), 10000, 0.5,
                                             0.999, 1e-8, flags, null, null, null, one, big, null)

    assert step(6, 9, 7, KT.EMD_K_PAD_VALID) != 0 and b"VALID needs width" in lib.emd_last_error()
    assert step(3, 9, 7, KT.EMD_K_PAD_REFLECT) != 0 and b"REFLECT" in lib.emd_last_error()
    assert step(9, 9, 3, 2) != 0 and b"border mode" in lib.emd_last_error()
    assert step(9, 9, 3, KT.EMD_K_PAD_VALID, flags=8) != 0 and b"unknown flag" in lib.emd_last_error()
    assert step(9, 9, 3, KT.EMD_K_PAD_VALID, flags=3) != 0
    assert step(9, 9, 3, KT.EMD_K_PAD_VALID, truth=null) != 0 and b"null pointer" in lib.emd_last_error()

    def pairs(S, patch, lo, hi):
        return lib.emd_k_make_pairs_f32(one, one, 1, S, S, patch, lo, hi, 0, 0, one, one, null, null)

    assert pairs(160, 20, 20, 20) != 0 and b"empty" in lib.emd_last_error()
    assert pairs(160, 20, 20, 142) != 0 and b"does not fit" in lib.emd_last_error()
    assert pairs(160, 20, -1, 100) != 0
    assert lib.emd_s_crop_unscale_f32(one, null, 1, 4, one, null) != 0
