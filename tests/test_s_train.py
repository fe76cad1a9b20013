"""Graph S training, CPU side: the learning-rate schedule, checkpoint names and their round trip through
autoencoder.load_weights, the host input path, and the set of exactly-zero gradients (float64 autograd)."""
import numpy as np
import pytest

import emdenoise
from emdenoise import AutoencoderTrainer, autoencoder, s_record_parser, tf_checkpoint  # noqa: F401
from emdenoise import autoencoder_trainer as AT
from emdenoise.k_trainer import k_crop
from tests import s_train_ref as R


def test_schedule():
    want = {1: 0.01, 49999: 0.01, 50000: 0.01 * 0.5 ** 1.5, 99999: 0.01 * 0.5 ** 1.5, 100000: 0.0}
    for t, v in want.items():
        assert AT.lr_schedule(t) == pytest.approx(v, rel=1e-15, abs=0.0)
    assert AT.lr_schedule(100000) == 0.0
    assert AT.adam_lr_t(0.01, 1) == pytest.approx(0.01 * np.sqrt(1 - 0.999) / (1 - 0.9))


@pytest.mark.parametrize("enc", [1, 4, 16])
def test_checkpoint_names(enc):
    specs = autoencoder.variable_specs(enc)
    trainable = [n for n in specs if not n.endswith(("/moving_mean", "/moving_variance"))]
    want = set(specs) | {n + s for n in trainable for s in ("/Adam", "/Adam_1")} | {"beta1_power", "beta2_power"}
    w = AT.initial_weights(enc, seed=3)
    zeros = {n: np.zeros(specs[n], np.float32) for n in trainable}
    sd = AT.s_state_dict(w, zeros, zeros, 7, enc)
    assert set(sd) == want == set(AT.state_dict_names(enc))
    for n, shape in specs.items():
        assert sd[n].shape == tuple(shape), n
    assert float(sd["beta1_power"]) == np.float32(0.9 ** 7)


@pytest.mark.parametrize("enc", [1, 16])
def test_checkpoint_loads_through_load_weights(tmp_path, enc):
    specs = autoencoder.variable_specs(enc)
    w = AT.initial_weights(enc, seed=5)
    w["Conv2d_transpose_2/biases"] = np.linspace(-1, 1, specs["Conv2d_transpose_2/biases"][0]).astype(np.float32)
    trainable = [n for n in specs if not n.endswith(("/moving_mean", "/moving_variance"))]
    m = {n: np.full(specs[n], 0.5, np.float32) for n in trainable}
    prefix = str(tmp_path / "-12")
    tf_checkpoint.write_checkpoint(prefix, AT.s_state_dict(w, m, m, 12, enc))
    got = autoencoder.load_weights(prefix, enc)
    assert list(got) == list(specs)
    for n in specs:
        np.testing.assert_array_equal(got[n], w[n])


def test_initial_weights():
    w = AT.initial_weights(16, seed=1)
    assert list(w) == list(autoencoder.variable_specs(16))
    for n, a in w.items():
        leaf = n.rsplit("/", 1)[1]
        if leaf in ("gamma", "moving_variance"):
            assert np.all(a == 1)
        elif leaf in ("beta", "biases", "moving_mean"):
            assert np.all(a == 0)
        else:
            rf = a.shape[0] * a.shape[1]
            assert np.abs(a).max() <= np.sqrt(6.0 / (rf * a.shape[2] + rf * a.shape[3]))
    np.testing.assert_array_equal(AT.initial_weights(16, seed=1)["Conv/weights"], w["Conv/weights"])


def test_s_record_parser_fallback_is_ones():
    rng = np.random.default_rng(0)
    img = np.full((171, 171), np.nan, np.float32)
    np.testing.assert_array_equal(s_record_parser(img, rng), np.ones((160, 160), np.float32))
    # a crop whose range overflows float32 is non-finite after scale0to1: graph S writes ones where graph K writes zeros
    big = rng.random((171, 171)).astype(np.float32)
    big[::2] = 3e38
    big[1::2] = -3e38
    np.testing.assert_array_equal(s_record_parser(big, np.random.default_rng(1)), np.ones((160, 160), np.float32))
    np.testing.assert_array_equal(k_crop(big, 0, 0, 0, 160), np.zeros((160, 160), np.float32))


def test_s_record_parser_draw_order():
    img = np.random.default_rng(2).random((171, 175)).astype(np.float32)
    rng, rng2 = np.random.default_rng(9), np.random.default_rng(9)
    got = s_record_parser(img, rng)
    x, y, ch = int(rng2.integers(0, 11)), int(rng2.integers(0, 15)), int(rng2.integers(0, 8))
    np.testing.assert_array_equal(got, AT.s_crop(img, x, y, ch, 160))
    assert abs(float(got.mean()) - 1.0) < 1e-5


def _nonzero_weights(enc, seed):
    """Weights with nonzero betas and biases (the zero set must not rely on zero-initialised values)."""
    return autoencoder.synthetic_weights(enc, seed)


@pytest.mark.parametrize("enc", [4, 16])
def test_zero_gradient_set(enc):
    rng = np.random.default_rng(enc)
    batch = rng.random((2, 32, 32)) + 0.5
    _, g = R.loss_and_grads(batch, _nonzero_weights(enc, 11), enc)
    scale = max(np.linalg.norm(v) for v in g.values())
    rel = {n: np.linalg.norm(v) / scale for n, v in g.items()}
    zero = set(AT.zero_gradient_names(enc))
    assert {n for n, r in rel.items() if r <= 1e-12} == zero, sorted((r, n) for n, r in rel.items())[:8]
    assert rel["Conv2d_transpose_2/biases"] > 1e-6
    assert rel["SeparableConv2d/BatchNorm/gamma"] > 1e-9
    for n in rel:
        if n not in zero:
            assert rel[n] > 1e-9, (n, rel[n])


def test_abi_surface():
    """The graph-S entry points are declared in include/emdenoise.h and bound by _lib (the library exports them: load() checks)."""
    import os

    from emdenoise import _lib

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "emdenoise.h")).read()
    for name in ("emd_s_sample_crops_f32", "emd_s_head_bwd_f32", "emd_s_head_bwd_workspace_bytes", "emd_s_mse_loss_f32",
                 "emd_s_mse_loss_workspace_bytes", "emd_relu_mask_bwd_f32"):
        assert name + "(" in hdr and name in _lib.SIGNATURES, name
    lib = _lib.load()
    assert lib.emd_s_head_bwd_workspace_bytes(32, 160, 160, 64) == 32 * 20 * 5 * (10 * 64 + 4) * 4 + 50 * (10 * 64 + 1) * 8
    assert lib.emd_s_head_bwd_workspace_bytes(0, 160, 160, 64) == 0
