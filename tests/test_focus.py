"""CPU tests of emdenoise.focus: the restatement of tests/focus_ref.py against scipy and numpy, the hand-written
border cases, and every refusal -- of the Python layer (before anything moves to a device) and of the C entry points (before any
launch).  No GPU is used."""
import ctypes as C

import numpy as np
import pytest
import scipy.interpolate
import scipy.stats

import emdenoise
from emdenoise import _lib, focus
from tests import focus_ref as R


def test_focus_is_exported():
    assert "focus" in emdenoise.__all__ and emdenoise.focus is focus
    assert focus.MOMENT_NAMES == ["mean_laplacian", "n", "mean", "m2", "m4", "kurtosis"] and focus.NMOMENTS == 6


def test_laplacian_border_by_hand():
    for x, k1, k3 in ((R.HAND_2X2, R.HAND_2X2_K1, R.HAND_2X2_K3), (R.HAND_3X3, R.HAND_3X3_K1, R.HAND_3X3_K3)):
        assert np.array_equal(R.laplacian(x, 1), k1)
        assert np.array_equal(R.laplacian(x, 3), k3)
    # a kernel that sums to zero: a constant image gives exact zeros, a ramp is annihilated away from the border
    assert not R.laplacian(np.full((5, 7), 3.25, np.float32), 3).any()
    ramp = np.add.outer(np.arange(6, dtype=np.float32), 2 * np.arange(9, dtype=np.float32))
    assert not R.laplacian(ramp, 1)[1:-1, 1:-1].any() and not R.laplacian(ramp, 3)[1:-1, 1:-1].any()


@pytest.mark.parametrize("rectify", [True, False])
def test_moments_restatement_equals_scipy_kurtosis(rectify):
    rng = np.random.default_rng(5)
    for img in (rng.standard_normal((40, 70)).astype(np.float32), rng.poisson(12.0, (17, 33)).astype(np.float32)):
        flat = R.laplacian(img, 3).ravel().astype(np.float64)
        row, margin = R.moments_of(flat, rectify)
        chosen = flat[flat >= flat.mean()] if rectify else flat
        assert row[1] == chosen.size and margin > 0
        want = scipy.stats.kurtosis(chosen)
        assert abs(row[5] - want) <= 1e-12 * max(1.0, abs(want)), (row[5], want)
        assert abs(row[3] - chosen.var()) <= 1e-12 * chosen.var()
    row, _ = R.moments_of(np.zeros(12), rectify)
    assert row[3] == 0 and row[4] == 0 and np.isnan(row[5]) and np.isnan(scipy.stats.kurtosis(np.zeros(12)))


def edge_values(bins):
    one = np.float32(1)
    v = [0.0, 1.0, one - np.float32(2.0 ** -24), np.nextafter(one, np.float32(2)), -0.0, -1e-30, -0.25, 1.5, np.nan, np.inf, -np.inf]
    v += [k / bins for k in range(bins + 1)]
    v += [np.nextafter(np.float32(k / bins), np.float32(0)) for k in range(1, bins + 1, max(1, bins // 64))]
    return np.array(v, np.float32)


@pytest.mark.parametrize("bins", [2, 16, 256, 4096])
def test_histogram_rule_equals_numpy(bins):
    rng = np.random.default_rng(bins)
    x = np.concatenate([edge_values(bins), rng.uniform(-0.2, 1.2, 20000).astype(np.float32)])
    finite = x[np.isfinite(x)]                                  # numpy refuses a range test on non-finite data in some versions
    want = np.histogram(finite, bins, range=(0, 1))[0]
    assert np.array_equal(R.histogram01(x, bins), want)
    assert np.array_equal(R.histogram01(x.astype(np.float64), bins), want)
    assert R.bin01(np.array([np.nan, -0.0, 1.0, 2.0], np.float32), bins).tolist() == [-1, 0, bins - 1, -1]


def test_entropy_restatement_equals_scipy():
    rng = np.random.default_rng(3)
    for bins in (2, 256, 4096):
        counts = rng.integers(0, 50, bins) * (rng.uniform(size=bins) < 0.7)
        want = scipy.stats.entropy(counts + 1e-6, base=2)
        assert abs(R.entropy(counts, 1e-6) - want) <= 1e-13 * want
    assert R.entropy(np.array([5, 5]), 0.0) == 1.0


@pytest.mark.parametrize("N", [4, 5, 9, 21, 64])
def test_notaknot_restatement_equals_scipy(N):
    rng = np.random.default_rng(N)
    for z in (np.linspace(-3.0, 5.0, N), np.cumsum(rng.uniform(0.2, 1.7, N))):
        y = rng.standard_normal(N) + 0.3 * (z - z.mean()) ** 2
        g = R.grid(z, 10)
        assert g.size == 10 * N and g[0] == z[0] and g[-1] == z[-1]
        mine = R.spline_eval(z, y, g)
        ius = scipy.interpolate.InterpolatedUnivariateSpline(z, y)(g)
        cs = scipy.interpolate.CubicSpline(z, y, bc_type="not-a-knot")(g)
        top = np.abs(ius).max()
        assert np.abs(mine - ius).max() <= 1e-11 * top and np.abs(cs - ius).max() <= 1e-11 * top
        zbest, curve, i = R.optimal_focus(z, y, 10)
        assert zbest == g[i] and curve[i] == curve.min()


def test_python_refusals_name_the_function():
    img = np.zeros((8, 8), np.float32)
    z4 = np.arange(4.0)
    bad = [
        (lambda: focus.laplacian(np.zeros((2, 3, 4, 5), np.float32)), "laplacian"),                    # rank
        (lambda: focus.laplacian(np.zeros(7, np.float32)), "laplacian"),
        (lambda: focus.laplacian(img.astype(np.float64)), "laplacian"),                                # dtype
        (lambda: focus.laplacian([[1.0, 2.0], [3.0, 4.0]]), "laplacian"),
        (lambda: focus.laplacian(np.zeros((1, 8), np.float32)), "laplacian"),                          # H < 2
        (lambda: focus.laplacian(np.zeros((3, 8, 1), np.float32)), "laplacian"),                       # W < 2
        (lambda: focus.laplacian(img, ksize=5), "laplacian"),
        (lambda: focus.laplacian_moments(img, ksize=2), "laplacian_moments"),
        (lambda: focus.laplacian_moments(img.astype(np.int32)), "laplacian_moments"),
        (lambda: focus.laplacian_moments(np.zeros((8, 1), np.float32)), "laplacian_moments"),
        (lambda: focus.fresnel_quantifier(img, ksize=0), "fresnel_quantifier"),
        (lambda: focus.fresnel_quantifier(np.zeros((1, 1, 8), np.float32)), "fresnel_quantifier"),
        (lambda: focus.histogram01(img, bins=100), "histogram01"),                                     # not a power of two
        (lambda: focus.histogram01(img, bins=1), "histogram01"),
        (lambda: focus.histogram01(img, bins=8192), "histogram01"),
        (lambda: focus.histogram01(img.astype(np.float16)), "histogram01"),
        (lambda: focus.image_entropy(img, num_bins=255), "image_entropy"),
        (lambda: focus.image_entropy(img, eps=-1.0), "image_entropy"),
        (lambda: focus.image_entropy(np.zeros((2, 2, 2, 2), np.float32)), "image_entropy"),
        (lambda: focus.optimal_focus(np.arange(3.0), np.zeros(3)), "optimal_focus"),                   # N < 4
        (lambda: focus.optimal_focus(np.arange(257.0), np.zeros(257)), "optimal_focus"),
        (lambda: focus.optimal_focus(np.array([0.0, 1.0, 1.0, 2.0]), np.zeros(4)), "optimal_focus"),   # not increasing
        (lambda: focus.optimal_focus(z4[::-1], np.zeros(4)), "optimal_focus"),
        (lambda: focus.optimal_focus(z4, np.zeros(5)), "optimal_focus"),                               # lengths differ
        (lambda: focus.optimal_focus(z4.reshape(2, 2), np.zeros(4)), "optimal_focus"),
        (lambda: focus.optimal_focus(z4, np.zeros((2, 2, 4))), "optimal_focus"),
        (lambda: focus.optimal_focus(z4, np.zeros(4), interp_factor=0), "optimal_focus"),
        (lambda: focus.autofocus(np.zeros((3, 8, 8), np.float32), np.arange(3.0)), "autofocus"),       # N < 4
        (lambda: focus.autofocus(np.zeros((4, 8, 8), np.float32), np.arange(5.0)), "autofocus"),
        (lambda: focus.autofocus(img, z4), "autofocus"),                                               # not a stack
        (lambda: focus.autofocus(np.zeros((4, 8, 8), np.float32), z4, ksize=7), "autofocus"),
        (lambda: focus.autofocus(np.zeros((4, 8, 8), np.float32), np.array([0.0, 2.0, 1.0, 3.0])), "autofocus"),
        (lambda: focus.autofocus(np.zeros((4, 8, 8), np.float64), z4), "autofocus"),
    ]
    for call, name in bad:
        with pytest.raises(ValueError, match=rf"^{name}: "):
            call()


def test_device_tensor_dtypes_are_refused_before_any_launch():
    import torch

    with pytest.raises(ValueError, match="^optimal_focus: z is float64"):
        focus.optimal_focus(torch.arange(4, dtype=torch.float32), np.zeros(4))
    with pytest.raises(ValueError, match="^optimal_focus: scores is float64"):
        focus.optimal_focus(np.arange(4.0), torch.zeros(4, dtype=torch.float32))
    with pytest.raises(ValueError, match="^laplacian: images are float32"):
        focus.laplacian(torch.zeros(4, 4, dtype=torch.float64))


def test_c_refusals_need_no_gpu():
    lib = _lib.load()
    null, a, b, c = C.c_void_p(0), C.c_void_p(4096), C.c_void_p(1 << 20), C.c_void_p(2 << 20)
    err = lib.emd_last_error

    assert lib.emd_laplacian_f32(a, 1, 1, 8, 1, b, null) == -1 and b"emd_laplacian_f32" in err()          # H < 2
    assert lib.emd_laplacian_f32(a, 1, 8, 1, 1, b, null) == -1
    assert lib.emd_laplacian_f32(a, 1, 8, 40000, 1, b, null) == -1
    assert lib.emd_laplacian_f32(a, 1, 8, 8, 5, b, null) == -1 and b"ksize" in err()
    assert lib.emd_laplacian_f32(null, 1, 8, 8, 1, b, null) == -1 and b"null" in err()
    assert lib.emd_laplacian_f32(a, 1, 8, 8, 1, a, null) == -1 and b"overlap" in err()
    assert lib.emd_laplacian_f32(a, -1, 8, 8, 1, b, null) == -1
    assert lib.emd_laplacian_f32(a, 0, 8, 8, 1, b, null) == 0                                              # empty batch: no-op

    need = lib.emd_laplacian_moments_workspace_bytes(2, 40, 70)
    assert need > 0 and need % 256 == 0 and lib.emd_laplacian_moments_workspace_bytes(2, 1, 70) == 0
    assert lib.emd_laplacian_moments_f64(a, 2, 1, 70, 3, 1, b, c, need, null) == -1
    assert lib.emd_laplacian_moments_f64(a, 2, 40, 70, 2, 1, b, c, need, null) == -1 and b"ksize" in err()
    assert lib.emd_laplacian_moments_f64(a, 2, 40, 70, 3, 2, b, c, need, null) == -1 and b"rectify" in err()
    assert lib.emd_laplacian_moments_f64(a, 2, 40, 70, 3, 1, b, c, need - 8, null) == -1 and b"too small" in err()
    assert lib.emd_laplacian_moments_f64(a, 2, 40, 70, 3, 1, null, c, need, null) == -1 and b"null" in err()
    assert lib.emd_laplacian_moments_f64(a, 2, 40, 70, 3, 1, b, C.c_void_p((2 << 20) + 8), need, null) == -3
    assert lib.emd_laplacian_moments_f64(a, 2, 40, 70, 3, 1, b, b, need, null) == -1 and b"overlap" in err()
    assert lib.emd_laplacian_moments_f64(a, 0, 40, 70, 3, 1, b, c, need, null) == 0

    assert lib.emd_histogram01_workspace_bytes(2, 40, 70, 0) == 0
    need = lib.emd_histogram01_workspace_bytes(2, 40, 70, 1)
    assert need > 0
    for bins in (0, 1, 3, 100, 8192):
        assert lib.emd_histogram01_i64(a, 2, 40, 70, bins, 0, b, null, 0, null) == -1 and b"power of two" in err()
    assert lib.emd_histogram01_i64(a, 2, 0, 70, 256, 0, b, null, 0, null) == -1
    assert lib.emd_histogram01_i64(a, 2, 40, 70, 256, 3, b, null, 0, null) == -1 and b"normalize" in err()
    assert lib.emd_histogram01_i64(a, 2, 40, 70, 256, 1, b, null, need, null) == -1 and b"null" in err()   # normalize needs it
    assert lib.emd_histogram01_i64(a, 2, 40, 70, 256, 1, b, c, need - 8, null) == -1 and b"too small" in err()
    assert lib.emd_histogram01_i64(a, 2, 40, 70, 256, 0, null, null, 0, null) == -1
    assert lib.emd_histogram01_i64(a, 0, 40, 70, 256, 0, b, null, 0, null) == 0

    assert lib.emd_hist_entropy_f64(a, 2, 0, 1e-6, b, null) == -1
    assert lib.emd_hist_entropy_f64(a, 2, 256, -1.0, b, null) == -1 and b"eps" in err()
    assert lib.emd_hist_entropy_f64(null, 2, 256, 1e-6, b, null) == -1
    assert lib.emd_hist_entropy_f64(a, 2, 256, 1e-6, a, null) == -1
    assert lib.emd_hist_entropy_f64(a, 0, 256, 1e-6, b, null) == 0

    d = C.c_void_p(3 << 20)
    for N in (3, 257, 0):
        assert lib.emd_spline_argmin_f64(a, b, 1, N, 10, c, null, null, null) == -1 and b"4 <= N <= 256" in err()
    assert lib.emd_spline_argmin_f64(a, b, 1, 9, 0, c, null, null, null) == -1 and b"interp_factor" in err()
    assert lib.emd_spline_argmin_f64(null, b, 1, 9, 10, c, null, null, null) == -1 and b"null" in err()
    assert lib.emd_spline_argmin_f64(a, b, 1, 9, 10, null, null, null, null) == -1
    assert lib.emd_spline_argmin_f64(a, b, 1, 9, 10, C.c_void_p((2 << 20) + 4), null, null, null) == -3
    assert lib.emd_spline_argmin_f64(a, b, 1, 9, 10, c, c, null, null) == -1 and b"overlap" in err()      # curve on zbest
    assert lib.emd_spline_argmin_f64(a, b, 1, 9, 10, c, d, b, null) == -1                                  # index on scores
    assert lib.emd_spline_argmin_f64(a, b, 0, 9, 10, c, null, null, null) == 0
