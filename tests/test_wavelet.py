"""CPU tests of the wavelet transform and wavelet shrinkage (emdenoise.filters wavedec2 / waverec2 / denoise_wavelet,
csrc/wavelet.hip): the restatement the GPU tests lean on (tests/wavelet_ref.py), the argument validation of every
new entry point through the C ABI (it runs before any launch, so null and made-up pointers are enough), the pyramid layout, and
baseline_table's seven-column form with the filters replaced by host stand-ins.  Nothing here touches a GPU."""
import ctypes

import numpy as np
import pytest

from emdenoise import _lib, filters
from tests import wavelet_ref as R
from tests.synth_inputs import synthetic_lq

SHAPES = [(37, 53), (70, 131), (64, 64), (8, 200), (200, 8), (128, 128)]
DB4 = R.daubechies(4)


def image(H, W, seed=5):
    rng = np.random.default_rng(seed + H * 1000 + W)
    return synthetic_lq(1, H, W, seed=seed)[0, :, :, 0].astype(np.float64) + 0.02 * rng.standard_normal((H, W))


def wavelets_for(H, W):
    return ["db1", "db2"] + ([DB4] if min(H, W) >= 14 else [])


# ---- the restatement -------------------------------------------------------------------------------------------------------

def test_db4_by_spectral_factorisation_is_orthogonal():
    for h in (DB4, R.rec_lo_of("db1"), R.rec_lo_of("db2"), R.daubechies(2), R.daubechies(3)):
        assert abs(h.sum() - np.sqrt(2.0)) < 1e-12
        for m in range(len(h) // 2):
            assert abs(np.dot(h[:len(h) - 2 * m], h[2 * m:]) - (1.0 if m == 0 else 0.0)) < 1e-12, m
    assert len(DB4) == 8
    assert np.max(np.abs(R.daubechies(2) - R.rec_lo_of("db2"))) < 1e-12 or np.max(np.abs(R.daubechies(2)[::-1] - R.rec_lo_of("db2"))) < 1e-12
    assert np.max(np.abs(R.daubechies(1) - R.rec_lo_of("haar"))) < 1e-12


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_perfect_reconstruction(shape):
    H, W = shape
    x = image(H, W)
    for wv in wavelets_for(H, W):
        L = len(R.rec_lo_of(wv))
        for levels in [l for l in (1, 2, 3) if l <= R.max_levels(H, W, L)] + [None]:
            c = R.wavedec2(x, wv, levels)
            n = [H], [W]
            for det in c[:0:-1]:                                          # finest first: (N + L - 1) // 2 per level
                n[0].append((n[0][-1] + L - 1) // 2)
                n[1].append((n[1][-1] + L - 1) // 2)
                assert all(det[k].shape == (n[0][-1], n[1][-1]) for k in ("ad", "da", "dd"))
            assert c[0].shape == (n[0][-1], n[1][-1])
            assert np.max(np.abs(R.waverec2(c, wv, (H, W)) - x)) <= 1e-12, (wv, levels)
    xb = np.stack([image(H, W, 1), image(H, W, 2)])                        # a batch: every image on its own
    cb = R.wavedec2(xb, "db2", 1)
    assert np.array_equal(cb[1]["dd"][1], R.wavedec2(xb[1], "db2", 1)[1]["dd"])
    assert np.max(np.abs(R.waverec2(cb, "db2", xb.shape) - xb)) <= 1e-12


def test_haar_hand_values():
    cA, det = R.dwt2(np.array([[1.0, 2.0], [3.0, 4.0]]), R.filter_bank("haar"))
    assert np.allclose([cA[0, 0], det["ad"][0, 0], det["da"][0, 0], det["dd"][0, 0]], [5.0, -1.0, -2.0, 0.0], atol=1e-14)
    # 3 x 3: the third row / column pairs with its own mirror image (the half-sample symmetric border): x2 + x2, x2 - x2
    x = np.array([[1.0, 2.0, 4.0], [3.0, 5.0, 9.0], [6.0, 7.0, 8.0]])
    cA, det = R.dwt2(x, R.filter_bank("db1"))
    assert np.allclose(cA, [[(1 + 2 + 3 + 5) / 2, (4 + 9) * 2 / 2], [(6 + 7) * 2 / 2, 8 * 4 / 2]], atol=1e-14)
    assert np.allclose(det["ad"], [[(1 - 2 + 3 - 5) / 2, 0.0], [(6 - 7) * 2 / 2, 0.0]], atol=1e-14)       # high along W
    assert np.allclose(det["da"], [[(1 + 2 - 3 - 5) / 2, (4 - 9) * 2 / 2], [0.0, 0.0]], atol=1e-14)       # high along H
    assert np.allclose(det["dd"], [[(1 - 2 - 3 + 5) / 2, 0.0], [0.0, 0.0]], atol=1e-14)
    assert det["dd"][1, 1] == 0.0 and det["ad"][0, 1] == 0.0                # exact zeros, in any precision
    assert np.array_equal(R.wavedec2(x.astype(np.float32), "db1", 1, np.float32)[1]["dd"] == 0, det["dd"] == 0)


def test_haar_preserves_energy():
    x = image(64, 64)
    for levels in (1, 3):
        c = R.wavedec2(x, "haar", levels)
        e = (c[0] ** 2).sum() + sum((d[k] ** 2).sum() for d in c[1:] for k in d)
        assert abs(e - (x ** 2).sum()) <= 1e-12 * (x ** 2).sum()


def test_default_levels_rule():
    assert R.default_levels(128, 128, 2) == 4 and R.default_levels(64, 64, 2) == 3 and R.default_levels(37, 53, 4) == 1
    assert R.max_levels(8, 200, 4) == 1 and R.max_levels(5, 200, 4) == 0 and R.max_levels(14, 14, 8) == 1 and R.max_levels(13, 99, 8) == 0
    for (H, W) in SHAPES:
        for L in (2, 4, 8):
            assert filters.wavelet_max_levels(H, W, L) == R.max_levels(H, W, L) == int(np.floor(np.log2(min(H, W) / (L - 1)) + 1e-9))


def test_shrinkage_behaviour():
    x = image(70, 131)
    for method in R.METHODS:
        assert np.max(np.abs(R.denoise_wavelet(x, "db2", 2, method, sigma=0.0) - x)) <= 1e-12       # sigma = 0 returns x
    z, s = R.denoise_wavelet(np.zeros((16, 16)), "db1", None, "BayesShrink", None, return_sigma=True)
    assert s == 0.0 and np.array_equal(z, np.zeros((16, 16)))                                       # no non-zero coefficient
    d = np.full((9, 9), 0.01)
    d[::2] *= -1
    t = R.bayes_threshold(d, 0.01 ** 2)                                    # mean(d^2) <= var: the band comes back all zero
    assert t == 0.01 ** 2 / np.sqrt(float(np.finfo(np.float32).eps)) and np.array_equal(R.soft(d, t), np.zeros_like(d))
    assert abs(R.bayes_threshold(d, 0.25e-4) - 0.25e-4 / np.sqrt(0.75e-4)) < 1e-15
    assert R.visu_threshold(0.05, (70, 131)) == 0.05 * np.sqrt(2.0 * np.log(70.0 * 131.0))
    assert np.array_equal(R.soft(np.array([-3.0, -1.0, 0.0, 0.5, 2.0]), 1.0), [-2.0, 0.0, 0.0, 0.0, 1.0])
    # VisuShrink with a known sigma: every detail band is soft-thresholded by sigma sqrt(2 ln(HW)), cA is left alone (Haar on even
    # extents is a bijection, so the transform of the result shows the thresholded coefficients)
    y = R.denoise_wavelet(image(64, 64), "db1", 2, "VisuShrink", sigma=0.02)
    c, got = R.wavedec2(image(64, 64), "db1", 2), R.wavedec2(y, "db1", 2)
    tv = 0.02 * np.sqrt(2.0 * np.log(64.0 * 64.0))
    assert np.max(np.abs(got[0] - c[0])) < 1e-12
    for a, b in zip(c[1:], got[1:]):
        for k in a:
            assert np.max(np.abs(R.soft(a[k], tv) - b[k])) < 1e-12
    # the noise estimate: the exact zeros are removed before the median
    dd = np.array([[0.0, 0.3, -0.1], [0.0, 0.0, 0.2]])
    assert R.sigma_est(dd) == 0.2 / R.MAD_TO_SIGMA
    assert R.sigma_est(np.array([[0.0, 0.4], [-0.1, 0.2], [0.0, 0.3]])) == np.float64(0.25) / R.MAD_TO_SIGMA


# ---- the C ABI -------------------------------------------------------------------------------------------------------------

def layout(H, W, L, levels):
    bands = (ctypes.c_long * (3 * (1 + 3 * levels)))()
    total = _lib.load().emd_wavelet_pyramid_floats(H, W, L, levels, bands)
    return total, [tuple(bands[3 * i:3 * i + 3]) for i in range(1 + 3 * levels)]


def test_pyramid_layout_tiles_the_pyramid():
    for (H, W) in SHAPES + [(33, 1025)]:
        for L in (2, 4, 6, 8):
            for levels in range(1, R.max_levels(H, W, L) + 1):
                total, bands = layout(H, W, L, levels)
                nH, nW, shapes = H, W, []
                for _ in range(levels):
                    nH, nW = (nH + L - 1) // 2, (nW + L - 1) // 2
                    shapes.insert(0, (nH, nW))
                assert bands[0][1:] == shapes[0]
                assert [b[1:] for b in bands[1:]] == [s for s in shapes for _ in range(3)]
                end = 0
                for off, h, w in bands:                                    # no gap, no overlap
                    assert off == end
                    end += h * w
                assert end == total
                assert _lib.load().emd_wavelet_pyramid_floats(H, W, L, levels, None) == total
    lib = _lib.load()
    assert lib.emd_wavelet_pyramid_floats(8, 200, 4, 2, None) == 0 and lib.emd_wavelet_pyramid_floats(64, 64, 3, 1, None) == 0
    assert lib.emd_wavelet_pyramid_floats(64, 64, 10, 1, None) == 0 and lib.emd_wavelet_pyramid_floats(0, 64, 2, 1, None) == 0
    assert lib.emd_wavelet_pyramid_floats(64, 64, 2, 0, None) == 0


def test_argument_validation_needs_no_gpu():
    lib = _lib.load()
    null, one, two, ws = ctypes.c_void_p(0), ctypes.c_void_p(16), ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 30)
    taps = (ctypes.c_double * 8)(*DB4)
    f = ctypes.c_float
    big = 1 << 40

    def bad(rc, word=None):
        assert rc == -1, rc
        if word is not None:
            assert word in lib.emd_last_error(), lib.emd_last_error()

    fwd = lambda x, p, B, H, W, t, L, lv, w, n: lib.emd_wavelet_forward_f32(x, p, B, H, W, t, L, lv, w, n, null)
    inv = lambda p, o, B, H, W, t, L, lv, w, n: lib.emd_wavelet_inverse_f32(p, o, B, H, W, t, L, lv, w, n, null)
    den = lambda x, o, B, H, W, t, L, lv, m, s, u, w, n: lib.emd_filter_wavelet_f32(x, o, B, H, W, t, L, lv, m, f(s), u, w, n, null)
    for call in (fwd, inv):
        bad(call(null, two, 1, 64, 64, taps, 4, 2, ws, big), b"null")
        bad(call(one, null, 1, 64, 64, taps, 4, 2, ws, big), b"null")
        bad(call(one, two, 1, 64, 64, null, 4, 2, ws, big), b"null")
        bad(call(one, two, 1, 64, 64, taps, 4, 2, null, big), b"null")
        bad(call(one, one, 1, 64, 64, taps, 4, 2, ws, big), b"alias")
        bad(call(one, ctypes.c_void_p(16 + 64), 1, 64, 64, taps, 4, 2, ws, big), b"alias")          # a partial overlap
        bad(call(one, two, 1, 64, 64, taps, 4, 2, two, big), b"alias")                              # the workspace on a buffer
        bad(call(one, two, 1, 64, 64, taps, 3, 1, ws, big), b"tap count")
        bad(call(one, two, 1, 64, 64, taps, 10, 1, ws, big), b"tap count")
        bad(call(one, two, 1, 64, 64, taps, 0, 1, ws, big), b"tap count")
        bad(call(one, two, 1, 64, 64, taps, 4, 0, ws, big), b"levels")
        bad(call(one, two, 1, 64, 64, taps, 4, 5, ws, big), b"levels")                              # floor(log2(64 / 3)) = 4
        bad(call(one, two, 1, 5, 200, taps, 4, 1, ws, big), b"levels")                              # no level fits
        bad(call(one, two, -1, 64, 64, taps, 4, 1, ws, big), b"shape")
        bad(call(one, two, 70000, 64, 64, taps, 4, 1, ws, big), b"shape")
        bad(call(one, two, 1, 0, 64, taps, 4, 1, ws, big), b"shape")
        bad(call(one, two, 1, 64, 40000, taps, 4, 1, ws, big), b"shape")
        need = lib.emd_wavelet_workspace_bytes(2, 70, 131, 4, 2)
        assert need > 0
        bad(call(one, ws, 2, 70, 131, taps, 4, 2, two, need - 1), b"workspace too small")
        assert call(one, two, 0, 64, 64, taps, 4, 2, ws, 0) == 0                                     # an empty batch is a no-op
    bad(den(null, two, 1, 64, 64, taps, 4, 2, 0, -1.0, null, ws, big), b"null")
    bad(den(one, null, 1, 64, 64, taps, 4, 2, 0, -1.0, null, ws, big), b"null")
    bad(den(one, two, 1, 64, 64, null, 4, 2, 0, -1.0, null, ws, big), b"null")
    bad(den(one, two, 1, 64, 64, taps, 4, 2, 0, -1.0, null, null, big), b"null")
    bad(den(one, one, 1, 64, 64, taps, 4, 2, 0, -1.0, null, ws, big), b"alias")
    bad(den(one, two, 1, 64, 64, taps, 4, 2, 0, -1.0, null, two, big), b"alias")
    bad(den(one, two, 1, 64, 64, taps, 4, 2, 0, -1.0, two, ws, big), b"alias")                      # sigma_used on out
    bad(den(one, two, 1, 64, 64, taps, 5, 1, 0, -1.0, null, ws, big), b"tap count")
    bad(den(one, two, 1, 64, 64, taps, 12, 1, 0, -1.0, null, ws, big), b"tap count")
    bad(den(one, two, 1, 64, 64, taps, 8, 4, 0, -1.0, null, ws, big), b"levels")                    # floor(log2(64 / 7)) = 3
    bad(den(one, two, 1, 64, 64, taps, 8, 0, 0, -1.0, null, ws, big), b"levels")
    bad(den(one, two, 1, 13, 64, taps, 8, 1, 0, -1.0, null, ws, big), b"levels")
    bad(den(one, two, 1, 64, 64, taps, 4, 2, 2, -1.0, null, ws, big), b"method")
    bad(den(one, two, 1, 64, 64, taps, 4, 2, -1, 0.1, null, ws, big), b"method")
    bad(den(one, two, 1, 64, 64, taps, 4, 2, 0, float("nan"), null, ws, big), b"sigma")
    bad(den(one, two, 70000, 64, 64, taps, 4, 2, 0, -1.0, null, ws, big), b"shape")
    bad(den(one, two, 1, 64, -3, taps, 4, 2, 0, -1.0, null, ws, big), b"shape")
    need = lib.emd_filter_wavelet_workspace_bytes(2, 70, 131, 4, 2)
    total = lib.emd_wavelet_pyramid_floats(70, 131, 4, 2, None)
    assert need >= lib.emd_wavelet_workspace_bytes(2, 70, 131, 4, 2) + 2 * total * 4
    bad(den(one, ws, 2, 70, 131, taps, 4, 2, 0, -1.0, null, two, need - 1), b"workspace too small")
    assert den(one, two, 0, 64, 64, taps, 4, 2, 0, -1.0, null, ws, 0) == 0
    nan_taps = (ctypes.c_double * 8)(*([float("nan")] * 8))
    bad(den(one, two, 1, 64, 64, nan_taps, 4, 2, 0, -1.0, null, ws, big), b"finite")
    # the sizes of refused arguments are 0
    for q in (lib.emd_wavelet_workspace_bytes, lib.emd_filter_wavelet_workspace_bytes):
        assert q(0, 64, 64, 4, 2) == 0 and q(1, 64, 64, 3, 1) == 0 and q(1, 64, 64, 4, 5) == 0 and q(1, 0, 64, 4, 1) == 0
        assert q(70000, 64, 64, 4, 1) == 0 and q(1, 5, 200, 4, 1) == 0 and q(1, 64, 64, 4, 4) > 0


def test_python_wrappers_refuse_bad_arguments_before_any_device_work():
    x = np.zeros((1, 64, 64), np.float32)
    for fn in (filters.wavedec2, filters.denoise_wavelet):
        with pytest.raises(ValueError, match="unknown name"):
            fn(x, "sym4")
        with pytest.raises(ValueError, match="tap count"):
            fn(x, [0.5, 0.5, 0.5])
        with pytest.raises(ValueError, match="tap count"):
            fn(x, np.ones(10))
        with pytest.raises(ValueError, match="levels"):
            fn(x, "db2", 5)
        with pytest.raises(ValueError, match="levels"):
            fn(x, "db2", 0)
        with pytest.raises(ValueError, match="allows no level"):
            fn(np.zeros((5, 200), np.float32), "db2")
        with pytest.raises(ValueError, match="allows no level"):
            fn(np.zeros((2, 200, 13, 1), np.float32), DB4)
    with pytest.raises(ValueError, match="method"):
        filters.denoise_wavelet(x, method="hard")
    with pytest.raises(ValueError, match="sigma"):
        filters.denoise_wavelet(x, sigma=-0.1)
    c = R.wavedec2(np.zeros((2, 37, 53)), "db2", 2)
    with pytest.raises(ValueError, match="levels"):
        filters.waverec2(c + [c[-1]] * 3, "db2", (2, 37, 53))
    with pytest.raises(ValueError, match="band of shape"):
        filters.waverec2(c, "db2", (2, 37, 55))
    with pytest.raises(ValueError, match="band of shape"):
        filters.waverec2(c, "db1", (2, 37, 53))
    assert np.allclose(filters.wavelet_taps("db2"), R.rec_lo_of("db2"), atol=0) and np.array_equal(filters.wavelet_taps("haar"), filters.wavelet_taps("db1"))


# ---- baseline_table's seven-column form --------------------------------------------------------------------------------------

def test_baseline_table_reference_columns(monkeypatch):
    calls = {}

    def stand_in(name, offset):
        def fn(a, **kw):
            calls[name] = kw
            return np.asarray(a) + np.float32(offset)
        return fn

    for i, name in enumerate(["gaussian", "bilateral", "median", "wiener", "denoise_wavelet", "tv_chambolle"]):
        monkeypatch.setattr(filters, name, stand_in(name, i + 1))
    monkeypatch.setattr(filters, "_mse_ssim", lambda p, t: (((np.asarray(p) - np.asarray(t)) ** 2).mean(axis=(1, 2, 3)),
                                                             np.asarray(p).mean(axis=(1, 2, 3))))
    monkeypatch.setattr(filters, "_clip01", lambda y: np.clip(y, 0.0, 1.0))
    monkeypatch.setattr(filters, "_upload", lambda a, device=None: (np.asarray(a), True))     # no device here
    lq = np.full((4, 6, 5, 1), 0.25, np.float32)
    truth = np.zeros_like(lq)
    assert filters.REFERENCE_LABELS == ["Unfiltered", "Gaussian", "Bilateral", "Median", "Wiener", "Wavelet", "Chambolle"]
    data, labels = filters.baseline_table(lq, truth, extra={"K": lambda a: a + np.float32(7), "D": lambda a: a + np.float32(8)},
                                          reference_columns=True, denoise_wavelet={"wavelet": "db2", "method": "VisuShrink"},
                                          tv_chambolle={"n_iter": 7})
    assert labels == filters.REFERENCE_LABELS + ["K", "D"] and data.shape == (4, 9, 2)
    want = 0.25 + np.arange(9, dtype=np.float64)
    np.testing.assert_allclose(data[:, :, 1], np.tile(want, (4, 1)), rtol=1e-6)          # each row scores its own method's output
    assert calls["denoise_wavelet"] == {"wavelet": "db2", "method": "VisuShrink"} and calls["tv_chambolle"] == {"n_iter": 7}
    with pytest.raises(ValueError, match="taken"):
        filters.baseline_table(lq, truth, extra={"Wavelet": lambda a: a}, reference_columns=True)
    # the default call is unchanged: six columns, no "Wavelet", and its argument key is refused
    calls.clear()
    data6, labels6 = filters.baseline_table(lq, truth, extra={"Wavelet": lambda a: a + np.float32(9)})
    assert labels6 == filters.LABELS + ["Wavelet"] and data6.shape == (4, 7, 2) and "denoise_wavelet" not in calls
    np.testing.assert_allclose(data6[0, :6, 1], 0.25 + np.array([0, 1, 2, 3, 4, 6.0]), rtol=1e-6)
    assert filters.LABELS == ["Unfiltered", "Gaussian", "Bilateral", "Median", "Wiener", "Chambolle"]
    with pytest.raises(TypeError, match="unknown filter"):
        filters.baseline_table(lq, truth, denoise_wavelet={})
    with pytest.raises(TypeError, match="unknown filter"):
        filters.baseline_table(lq, truth, reference_columns=True, wavelet={})


def test_exported_from_the_package_and_the_shim():
    import emdenoise

    for name in ("wavedec2", "waverec2", "denoise_wavelet", "wavelet_taps"):
        assert callable(getattr(emdenoise.filters, name))
    assert emdenoise.filters.REFERENCE_LABELS[5] == "Wavelet"
