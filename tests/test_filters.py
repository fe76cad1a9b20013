"""CPU tests of the classical baseline filters (emdenoise.filters, csrc/filters.hip): the restatements the GPU
tests lean on (tests/filters_ref.py), the argument validation of every entry point through the C ABI (it runs before any
launch, so null and made-up pointers are enough), and baseline_table's label order and shape logic with the filters replaced
by host stand-ins.  Nothing here touches a GPU."""
import ctypes

import numpy as np
import pytest

from emdenoise import _lib, filters
from tests import filters_ref as R
from tests.synth_inputs import synthetic_lq


def images(B=2, H=37, W=53, seed=5):
    return synthetic_lq(B, H, W, seed=seed)[..., 0].astype(np.float64)


# ---- the restatements ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [3, 5, 9])
def test_bilateral_without_range_term_is_the_disc_gaussian(d):
    x = images()
    got = R.bilateral(x, d=d, sigma_color=1e6, sigma_space=1.5)
    assert np.max(np.abs(got - R.disc_gaussian(x, d=d, sigma_space=1.5))) < 1e-12


def test_chambolle_one_iteration_returns_x():
    x = images()
    assert np.array_equal(R.tv_chambolle(x, 0.1, 1), x)


def test_chambolle_leaves_a_constant_image_constant():
    x = np.full((1, 20, 31), 0.37)
    assert np.array_equal(R.tv_chambolle(x, 0.2, 30), x)


def test_chambolle_does_not_increase_total_variation():
    rng = np.random.default_rng(2)
    x = np.zeros((40, 56))
    x[:, 28:] = 0.8
    x += 0.05 * rng.standard_normal(x.shape)
    assert R.total_variation(R.tv_chambolle(x, 0.1, 30)) <= R.total_variation(R.tv_chambolle(x, 0.1, 1))


def test_float32_yardsticks_restate_scipy():
    """The spelled-out Gaussian and Wiener (the float32 yardsticks of the GPU tests) are scipy's results when run in float64."""
    x = images()
    for k, s in ((3, 1.5), (11, 1.5), (15, 3.0)):
        assert np.max(np.abs(R.gaussian_restated(x, s, k) - R.gaussian(x, s, k))) < 1e-12
    for k in (3, 5, 9):
        for n in (None, 0.004):
            assert np.max(np.abs(R.wiener_restated(x, k, n) - R.wiener(x, k, n))) < 1e-12


# ---- the C ABI's argument validation ----------------------------------------------------------------------------------------

def test_argument_validation_needs_no_gpu():
    lib = _lib.load()
    null, one, two, ws = ctypes.c_void_p(0), ctypes.c_void_p(16), ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 30)
    taps = (ctypes.c_float * 15)(*([1.0 / 15] * 15))
    f = ctypes.c_float
    big = 1 << 40

    def bad(rc, word=None):
        assert rc == -1, rc
        if word is not None:
            assert word in lib.emd_last_error(), lib.emd_last_error()

    # null pointers
    bad(lib.emd_filter_gaussian_f32(null, two, 1, 8, 8, taps, 3, null), b"null")
    bad(lib.emd_filter_gaussian_f32(one, two, 1, 8, 8, null, 3, null), b"null")
    bad(lib.emd_filter_median_f32(one, null, 1, 8, 8, 3, null), b"null")
    bad(lib.emd_filter_bilateral_f32(null, two, 1, 8, 8, 5, f(0.1), f(1.5), null), b"null")
    bad(lib.emd_filter_wiener_f32(null, two, 1, 8, 8, 5, f(0.01), null, null, 0, null), b"null")
    bad(lib.emd_filter_wiener_f32(one, two, 1, 8, 8, 5, f(-1.0), null, null, 0, null), b"null")      # the estimate needs a workspace
    bad(lib.emd_filter_tv_f32(one, two, 1, 8, 8, f(0.1), 5, null, 0, null), b"null")
    bad(lib.emd_filter_clip01_f32(null, two, 64, null), b"null")
    # out aliases x
    bad(lib.emd_filter_gaussian_f32(one, one, 1, 8, 8, taps, 3, null), b"alias")
    bad(lib.emd_filter_median_f32(one, ctypes.c_void_p(16 + 64), 1, 8, 8, 3, null), b"alias")       # a partial overlap
    bad(lib.emd_filter_tv_f32(one, one, 1, 8, 8, f(0.1), 5, ws, big, null), b"alias")
    # window sizes: even, out of range, 7 for the median, d = 11
    bad(lib.emd_filter_gaussian_f32(one, two, 1, 32, 32, taps, 4, null), b"ksize")
    bad(lib.emd_filter_gaussian_f32(one, two, 1, 32, 32, taps, 17, null), b"ksize")
    bad(lib.emd_filter_median_f32(one, two, 1, 32, 32, 4, null), b"ksize")
    bad(lib.emd_filter_median_f32(one, two, 1, 32, 32, 7, null), b"ksize")
    bad(lib.emd_filter_bilateral_f32(one, two, 1, 32, 32, 4, f(0.1), f(1.5), null), b"odd")
    bad(lib.emd_filter_bilateral_f32(one, two, 1, 32, 32, 11, f(0.1), f(1.5), null), b"3..9")
    bad(lib.emd_filter_bilateral_f32(one, two, 1, 32, 32, 5, f(0.0), f(1.5), null), b"sigma")
    bad(lib.emd_filter_wiener_f32(one, two, 1, 32, 32, 4, f(0.01), null, null, 0, null), b"ksize")
    bad(lib.emd_filter_wiener_f32(one, two, 1, 32, 32, 11, f(0.01), null, null, 0, null), b"ksize")
    # the mirror border needs radius < min(H, W)
    bad(lib.emd_filter_gaussian_f32(one, two, 1, 7, 200, taps, 15, null), b"mirror")
    bad(lib.emd_filter_gaussian_f32(one, two, 1, 200, 1, taps, 3, null), b"mirror")
    bad(lib.emd_filter_median_f32(one, two, 1, 2, 200, 5, null), b"mirror")
    bad(lib.emd_filter_bilateral_f32(one, two, 1, 200, 4, 9, f(0.1), f(1.5), null), b"mirror")
    # Chambolle: n_iter < 1, weight <= 0
    bad(lib.emd_filter_tv_f32(one, two, 1, 8, 8, f(0.1), 0, ws, big, null), b"n_iter")
    bad(lib.emd_filter_tv_f32(one, two, 1, 8, 8, f(0.0), 5, ws, big, null), b"weight")
    bad(lib.emd_filter_tv_f32(one, two, 1, 8, 8, f(-1.0), 5, ws, big, null), b"weight")
    # workspaces that are too small (one byte short of the advertised size)
    need = lib.emd_filter_tv_workspace_bytes(2, 70, 131)
    assert need >= 4 * 2 * 70 * 131 * 4
    bad(lib.emd_filter_tv_f32(one, two, 2, 70, 131, f(0.1), 5, ws, need - 1, null), b"workspace too small")
    need = lib.emd_filter_wiener_workspace_bytes(2, 70, 131)
    assert need > 0
    bad(lib.emd_filter_wiener_f32(one, two, 2, 70, 131, 5, f(-1.0), null, ws, need - 1, null), b"workspace too small")
    # the sizes of refused arguments are 0; bad shapes
    assert lib.emd_filter_tv_workspace_bytes(0, 8, 8) == 0 and lib.emd_filter_wiener_workspace_bytes(1, 0, 8) == 0
    bad(lib.emd_filter_median_f32(one, two, -1, 8, 8, 3, null), b"shape")
    bad(lib.emd_filter_median_f32(one, two, 70000, 8, 8, 3, null), b"shape")
    # an empty batch is a no-op
    assert lib.emd_filter_gaussian_f32(one, two, 0, 8, 8, taps, 3, null) == 0
    assert lib.emd_filter_median_f32(one, two, 0, 8, 8, 3, null) == 0
    assert lib.emd_filter_bilateral_f32(one, two, 0, 8, 8, 5, f(0.1), f(1.5), null) == 0
    assert lib.emd_filter_wiener_f32(one, two, 0, 8, 8, 5, f(-1.0), null, ws, 0, null) == 0
    assert lib.emd_filter_tv_f32(one, two, 0, 8, 8, f(0.1), 5, ws, 0, null) == 0
    assert lib.emd_filter_clip01_f32(one, one, 0, null) == 0


def test_python_wrappers_refuse_bad_arguments_before_any_device_work():
    x = np.zeros((1, 8, 8), np.float32)
    with pytest.raises(ValueError, match="ksize"):
        filters.median(x, 7)
    with pytest.raises(ValueError, match="odd"):
        filters.bilateral(x, d=11)
    with pytest.raises(ValueError, match="ksize"):
        filters.wiener(x, ksize=4)
    with pytest.raises(ValueError, match="noise"):
        filters.wiener(x, noise=-0.5)
    with pytest.raises(ValueError, match="n_iter"):
        filters.tv_chambolle(x, n_iter=0)
    with pytest.raises(ValueError, match="weight"):
        filters.tv_chambolle(x, weight=0.0)
    with pytest.raises(ValueError, match="window size"):
        filters.gaussian(x, ksize=4)
    thin = np.zeros((1, 4, 200), np.float32)                 # the mirror border: checked on the shape, before any upload
    with pytest.raises(ValueError, match="mirror"):
        filters.gaussian(thin, ksize=9)
    with pytest.raises(ValueError, match="mirror"):
        filters.bilateral(thin[0].T, d=9)
    with pytest.raises(ValueError, match="mirror"):
        filters.median(np.zeros((2, 200), np.float32), 5)


# ---- baseline_table's host logic ---------------------------------------------------------------------------------------------

def test_baseline_table_labels_and_shape(monkeypatch):
    """The filters and the scoring replaced by host stand-ins: the order of the rows is the reference's, extra rows follow, every
    method's own output is what gets scored, filter arguments reach their filter, and clip is off unless asked for."""
    calls = {}

    def stand_in(name, offset):
        def fn(a, **kw):
            calls[name] = kw
            return np.asarray(a) + np.float32(offset)
        return fn

    for i, name in enumerate(["gaussian", "bilateral", "median", "wiener", "tv_chambolle"]):
        monkeypatch.setattr(filters, name, stand_in(name, i + 1))
    monkeypatch.setattr(filters, "_mse_ssim", lambda p, t: (((np.asarray(p) - np.asarray(t)) ** 2).mean(axis=(1, 2, 3)),
                                                             np.asarray(p).mean(axis=(1, 2, 3))))
    monkeypatch.setattr(filters, "_clip01", lambda y: np.clip(y, 0.0, 1.0))
    monkeypatch.setattr(filters, "_upload", lambda a, device=None: (np.asarray(a), True))     # no device here
    lq = np.full((4, 6, 5, 1), 0.25, np.float32)
    truth = np.zeros_like(lq)
    data, labels = filters.baseline_table(lq, truth, extra={"K": lambda a: a + np.float32(6), "D": lambda a: a + np.float32(7)},
                                          gaussian={"sigma": 2.0, "ksize": 5}, tv_chambolle={"n_iter": 7})
    assert labels == ["Unfiltered", "Gaussian", "Bilateral", "Median", "Wiener", "Chambolle", "K", "D"]
    assert labels[:6] == filters.LABELS
    assert data.shape == (4, 8, 2)
    want = 0.25 + np.arange(8, dtype=np.float64)
    np.testing.assert_allclose(data[:, :, 1], np.tile(want, (4, 1)), rtol=1e-6)          # each row scores its own method's output
    np.testing.assert_allclose(data[:, :, 0], np.tile(want ** 2, (4, 1)), rtol=1e-6)
    assert calls["gaussian"] == {"sigma": 2.0, "ksize": 5} and calls["tv_chambolle"] == {"n_iter": 7} and calls["median"] == {}
    clipped, _ = filters.baseline_table(lq, truth, clip=True)
    assert clipped.shape == (4, 6, 2)
    np.testing.assert_allclose(clipped[0, :, 1], [0.25, 1, 1, 1, 1, 1], rtol=1e-6)        # the input itself is never clipped
    with pytest.raises(TypeError, match="unknown filter"):
        filters.baseline_table(lq, truth, wavelet={})
    with pytest.raises(ValueError, match="taken"):
        filters.baseline_table(lq, truth, extra={"Median": lambda a: a})
    with pytest.raises(ValueError, match="shape"):
        filters.baseline_table(lq, truth, extra={"K": lambda a: a[:, :-1]})


def test_exported_from_the_package_and_the_shim():
    import emdenoise

    assert emdenoise.filters is filters and emdenoise.baseline_table is filters.baseline_table
    for name in ("gaussian", "median", "bilateral", "wiener", "tv_chambolle", "baseline_table"):
        assert callable(getattr(emdenoise.filters, name))
