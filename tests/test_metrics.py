"""CPU tests of the image-quality metrics: pins of the float64 restatement of the reference's tf_ssim /
tf_ms_ssim (tests/ssim_ref.py) that need no TensorFlow, and the surface of emdenoise.metrics and of the C entry points, whose
argument validation runs before any launch.  No GPU here; the device results are checked in tests/test_metrics_gpu.py."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import emdenoise
from emdenoise import _lib
from tests import ssim_ref as R
from tests.synth_inputs import synthetic_pair

C1, C2 = 0.01 ** 2, 0.03 ** 2


# ---- pins of the restatement -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size,sigma", [(11, 1.5), (3, 1.5), (15, 2.0)])
def test_window_sums_to_one_is_symmetric_and_separable(size, sigma):
    g = R.fspecial_gauss(size, sigma).numpy()
    assert g.shape == (size, size)
    assert abs(g.sum() - 1.0) < 1e-14
    np.testing.assert_array_equal(g, g.T)
    np.testing.assert_array_equal(g, g[::-1, ::-1])
    assert g[size // 2, size // 2] == g.max()
    # the 1-D taps the device routines take: their outer product is the reference's window
    t = emdenoise.metrics.gaussian_taps(size, sigma).astype(np.float64)
    assert t.shape == (size,) and np.array_equal(t, t[::-1])
    np.testing.assert_allclose(np.outer(t, t), g, rtol=0, atol=2e-8)


def test_identical_images_score_one():
    a, _ = synthetic_pair(2, 176, 176, seed=3)
    r = R.ssim(a, a)
    np.testing.assert_allclose(r["ssim_map"], 1.0, rtol=0, atol=1e-12)
    np.testing.assert_allclose(r["cs_map"], 1.0, rtol=0, atol=1e-12)
    v, mssim, mcs = R.ms_ssim(a, a)
    assert abs(float(v) - 1.0) < 1e-12 and mssim.shape == (5,) and mcs.shape == (5,)


def test_constant_images_closed_form():
    c1, c2 = 0.3, 0.7
    a = np.full((1, 20, 24, 1), c1)
    b = np.full((1, 20, 24, 1), c2)
    r = R.ssim(a, b)
    assert r["ssim_map"].shape == (1, 10, 14)
    np.testing.assert_allclose(r["ssim_map"], (2 * c1 * c2 + C1) / (c1 * c1 + c2 * c2 + C1), rtol=1e-12)
    np.testing.assert_allclose(r["cs_map"], 1.0, rtol=1e-10)   # no variance: C2 / C2


def test_autograd_gradient_matches_central_differences():
    x, y = synthetic_pair(1, 24, 28, seed=7)
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    loss, g = R.ssim_loss(x64, y64)
    assert g.shape == (1, 24, 28) and 0.0 < float(loss) < 1.0

    def L(xx):
        return float(1.0 - R.ssim(xx, y64)["batch"][0])

    h = 1e-6
    # a corner, two edge pixels, the pixel next to the corner and interior pixels
    for (i, j) in [(0, 0), (23, 27), (0, 13), (12, 0), (1, 1), (12, 14), (9, 20)]:
        xp, xm = x64.copy(), x64.copy()
        xp[0, i, j, 0] += h
        xm[0, i, j, 0] -= h
        fd = (L(xp) - L(xm)) / (2 * h)
        assert abs(fd - g[0, i, j]) <= 1e-6 * abs(g[0, i, j]) + 1e-9, (i, j, fd, g[0, i, j])   # h^2 truncation + 1e-16 / h roundoff
    # a border pixel is covered by one map element only: its gradient is much smaller than an interior pixel's, and not zero
    assert g[0, 0, 0] != 0.0


def test_odd_extent_pooling_rule_by_hand():
    """tf.nn.avg_pool 2x2 / 2 SAME on 5 x 7: output 3 x 4; the last row's windows hold one row, the last column's one column,
    the corner a single element -- each divided by the number of valid elements."""
    x = np.arange(35, dtype=np.float64).reshape(5, 7)
    got = R.avg_pool_same_t(torch.from_numpy(x)[None, None])[0, 0].numpy()
    want = np.array([
        [(0 + 1 + 7 + 8) / 4, (2 + 3 + 9 + 10) / 4, (4 + 5 + 11 + 12) / 4, (6 + 13) / 2],
        [(14 + 15 + 21 + 22) / 4, (16 + 17 + 23 + 24) / 4, (18 + 19 + 25 + 26) / 4, (20 + 27) / 2],
        [(28 + 29) / 2, (30 + 31) / 2, (32 + 33) / 2, 34.0],
    ])
    np.testing.assert_array_equal(got, want)


def test_ms_ssim_formula_from_level_means():
    a, b = synthetic_pair(1, 176, 176, seed=2)
    v, mssim, mcs = R.ms_ssim(a, b)
    w = np.array(R.WEIGHTS)
    assert (mcs > 0).all()
    np.testing.assert_allclose(float(v), np.prod(mcs[:4] ** w[:4]) * mssim[4] ** w[4], rtol=1e-13)
    v3, mssim3, mcs3 = R.ms_ssim(a, b, level=3)     # the first `level` weights, as the reference's slicing does
    np.testing.assert_allclose(float(v3), np.prod(mcs3[:2] ** w[:2]) * mssim3[2] ** w[2], rtol=1e-13)
    np.testing.assert_allclose(mcs3, mcs[:3], rtol=1e-13)


# ---- the surface ---------------------------------------------------------------------------------------------------------

def test_names_and_the_reference_argument_lists():
    for name in ("ssim", "ms_ssim", "psnr", "ssim_loss", "tf_ssim", "tf_ms_ssim"):
        assert name in emdenoise.__all__ and callable(getattr(emdenoise, name))
    args = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    assert args(emdenoise.tf_ssim) == [("img1", E), ("img2", E), ("cs_map", False), ("mean_metric", True), ("size", 11), ("sigma", 1.5)]
    assert args(emdenoise.tf_ms_ssim) == [("img1", E), ("img2", E), ("mean_metric", True), ("level", 5)]
    assert args(emdenoise.ssim)[:7] == [("a", E), ("b", E), ("cs_map", False), ("mean_metric", True), ("size", 11), ("sigma", 1.5),
                                        ("per_image", False)]
    assert args(emdenoise.ms_ssim)[:5] == [("a", E), ("b", E), ("mean_metric", True), ("level", 5), ("per_image", False)]
    assert args(emdenoise.psnr)[:4] == [("a", E), ("b", E), ("data_range", 1.0), ("per_image", False)]
    assert args(emdenoise.ssim_loss)[:4] == [("x", E), ("y", E), ("dout", None), ("scale", 1.0)]
    assert inspect.signature(emdenoise.DenoiserTrainer.__init__).parameters["ssim_weight"].default == 0.0
    for fn in ("tower", "local_gradients", "train_step"):
        assert "ssim_weight" in inspect.signature(getattr(emdenoise.DenoiserTrainer, fn)).parameters
    from emdenoise import autoencoder, kernel_denoiser

    for cls in (emdenoise.Denoiser, autoencoder.Micrograph_Autoencoder, kernel_denoiser.Micrograph_Autoencoder):
        assert list(inspect.signature(cls.score).parameters) == ["self", "lq", "truth"]


def test_python_surface_refuses_bad_arguments_without_a_gpu():
    a = np.zeros((1, 160, 160, 1), np.float32)
    with pytest.raises(ValueError, match="at least 176"):
        emdenoise.ms_ssim(a, a)
    with pytest.raises(ValueError, match="level"):
        emdenoise.ms_ssim(a, a, level=6)
    with pytest.raises(ValueError, match="odd"):
        emdenoise.ssim(a, a, size=10)
    with pytest.raises(ValueError, match="odd"):
        emdenoise.ssim(a, a, size=17)
    with pytest.raises(ValueError, match="smaller than"):
        emdenoise.ssim(np.zeros((1, 10, 64, 1), np.float32), np.zeros((1, 10, 64, 1), np.float32))
    with pytest.raises(ValueError, match="smaller than"):
        emdenoise.ssim_loss(np.zeros((8, 8), np.float32), np.zeros((8, 8), np.float32))


def test_c_entry_points_validate_before_any_launch():
    lib = _lib.load()
    null, one, two, three = (ctypes.c_void_p(v) for v in (0, 4096, 1 << 20, 1 << 21))
    ws, big = ctypes.c_void_p(1 << 22), 1 << 30
    taps = emdenoise.metrics.gaussian_taps(11, 1.5)
    tp = taps.ctypes.data_as(ctypes.c_void_p)
    err = lambda: lib.emd_last_error()

    assert lib.emd_ssim_f32(null, two, 1, 64, 64, tp, 11, three, null, null, ws, big, null) == -1 and b"null" in err()
    assert lib.emd_ssim_f32(one, two, 1, 64, 64, null, 11, three, null, null, ws, big, null) == -1 and b"null" in err()
    assert lib.emd_ssim_f32(one, two, 1, 64, 64, tp, 10, three, null, null, ws, big, null) == -1 and b"odd" in err()
    assert lib.emd_ssim_f32(one, two, 1, 64, 64, tp, 17, three, null, null, ws, big, null) == -1 and b"odd" in err()
    assert lib.emd_ssim_f32(one, two, 1, 10, 64, tp, 11, three, null, null, ws, big, null) == -1 and b"smaller" in err()
    assert lib.emd_ssim_f32(one, two, 1, 64, 10, tp, 11, three, null, null, ws, big, null) == -1 and b"smaller" in err()
    assert lib.emd_ssim_f32(one, two, 1, 64, 64, tp, 11, three, null, null, ws, 8, null) == -1 and b"workspace" in err()
    assert lib.emd_ssim_f32(one, two, 0, 64, 64, tp, 11, three, null, null, ws, 0, null) == 0          # empty batch: no-op
    assert lib.emd_ssim_workspace_bytes(2, 64, 64, 11) > 0 and lib.emd_ssim_workspace_bytes(2, 8, 64, 11) == 0

    L = lambda x, y, B, H, W, size, dout, res: lib.emd_ssim_loss_f32(x, y, B, H, W, tp, size, 0, 1.0, null, dout, res, null, 1, 0.0,
                                                                      ws, big, null)
    assert L(one, two, 1, 64, 64, 11, three, null) == -1 and b"null" in err()
    assert L(one, two, 1, 64, 64, 12, three, ws) == -1 and b"odd" in err()
    assert L(one, two, 1, 5, 64, 11, three, ws) == -1 and b"smaller" in err()
    assert L(one, two, 1, 64, 64, 11, one, three) == -1 and b"alias" in err()                          # dout aliases x
    assert L(one, two, 1, 64, 64, 11, two, three) == -1 and b"alias" in err()                          # dout aliases y
    assert L(one, two, 0, 64, 64, 11, three, ws) == 0
    skew = taps.copy()
    skew[0] *= 2
    assert lib.emd_ssim_loss_f32(one, two, 1, 64, 64, skew.ctypes.data_as(ctypes.c_void_p), 11, 0, 1.0, null, three, ws, null, 1, 0.0,
                                 ws, big, null) == -1 and b"symmetric" in err()

    M = lambda H, W, level: lib.emd_ms_ssim_f32(one, two, 1, H, W, level, tp, 11, three, null, ws, big, null)
    assert M(160, 160, 5) == -1 and b"too small" in err() and b"176" in err()
    assert M(176, 175, 5) == -1 and b"too small" in err()
    assert M(176, 176, 0) == -1 and b"level" in err()
    assert M(176, 176, 6) == -1 and b"level" in err()
    assert lib.emd_ms_ssim_f32(one, two, 0, 176, 176, 5, tp, 11, three, null, ws, 0, null) == 0
    assert lib.emd_ms_ssim_workspace_bytes(2, 176, 176, 5, 11) > 0 and lib.emd_ms_ssim_workspace_bytes(2, 160, 160, 5, 11) == 0

    assert lib.emd_psnr_f32(one, null, 1, 64, 1.0, three, ws, big, null) == -1 and b"null" in err()
    assert lib.emd_psnr_f32(one, two, 1, 0, 1.0, three, ws, big, null) == -1
    assert lib.emd_psnr_f32(one, two, 1, 64, 0.0, three, ws, big, null) == -1 and b"data_range" in err()
    assert lib.emd_psnr_f32(one, two, 0, 64, 1.0, three, ws, 0, null) == 0
    assert lib.emd_avgpool2x2_same_c1_f32(null, two, 1, 5, 7, null) == -1 and b"null" in err()
    assert lib.emd_avgpool2x2_same_c1_f32(one, one, 1, 5, 7, null) == -1 and b"alias" in err()
    assert lib.emd_avgpool2x2_same_c1_f32(one, two, 1, 0, 7, null) == -1
    assert lib.emd_avgpool2x2_same_c1_f32(one, two, 0, 5, 7, null) == 0
