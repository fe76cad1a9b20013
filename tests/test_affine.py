"""CPU tests of the affine registration by mutual information (emdenoise.affine, csrc/affine.hip): the properties of
the float64 restatement (tests/affine_ref.py), the argument checks of the C entry points and of the Python module -- both run before
anything is launched or moved --, and the condition under which the end-to-end recovery test of tests/test_affine_gpu.py means
something: the restatement itself recovers the transform."""
import ctypes as C

import numpy as np
import pytest

from emdenoise import _lib, affine
from tests import affine_ref as R


# ---- the restatement's own properties -----------------------------------------------------------------------------------------------

def test_the_four_spline_weights_sum_to_one():
    tm = np.random.default_rng(0).uniform(2.0, 47.0, 10000)
    jm = np.floor(tm)
    w = np.stack([R.bspline3(jm + d - tm) for d in (-1, 0, 1, 2)])
    assert np.abs(w.sum(0) - 1.0).max() <= 4 * 2.0 ** -53 and (w >= 0).all() and w.max() <= 2 / 3
    q = np.rint(w * 2.0 ** 32).astype(np.int64).sum(0)                      # the fixed-point weights: four roundings of at most 1/2
    assert np.abs(q - 2 ** 32).max() <= 2
    assert R.bspline3(0.0) == 2 / 3 and R.bspline3(2.0) == 0.0 and R.bspline3(-1.0) == R.bspline3(1.0) == 1 / 6


@pytest.mark.parametrize("shape", [(2, 8, 8), (1, 33, 47)], ids=str)
def test_the_identity_warp_is_a_copy(shape):
    x = np.random.default_rng(1).random(shape, dtype=np.float32) + 0.5
    assert np.array_equal(R.warp(x, R.identity()), x)
    assert np.array_equal(R.warp(x, np.stack([R.identity()] * shape[0]), fill=0.25), x)


def test_chain_to_middle_composed_with_its_inverse_is_the_identity():
    pairs = np.stack([R.similarity(1.0 + k, 1.0 + 0.01 * k, (0.5 * k, -k), 64, 64) for k in range(4)])
    Cm = R.chain_to_middle(pairs)                                            # N = 5, middle = 2
    assert np.array_equal(Cm[2], R.identity()) and np.array_equal(Cm[3], pairs[2])
    for j in range(5):
        both = np.array(R._mul3(R._hom(Cm[j]), R._inv3(Cm[j]))[:2])
        assert np.abs(both - R.identity()).max() <= 1e-14
    # the pair transform takes frame j to frame j + 1: C_{j+1} = M_j C_j on either side of the middle
    for j in range(4):
        step = np.array(R._mul3(R._hom(pairs[j]), R._hom(Cm[j]))[:2])
        assert np.abs(step - Cm[j + 1]).max() <= 1e-14
    assert np.array_equal(R.chain_to_middle(pairs, middle=0)[1], pairs[0])
    bad = pairs.copy()
    bad[1] = [[1, 2, 0], [2, 4, 0]]                                          # singular, next to the middle: NaNs from there outwards
    Cb = R.chain_to_middle(bad)
    assert np.isnan(Cb[0]).all() and np.isnan(Cb[1]).all() and np.array_equal(Cb[2:], Cm[2:])


@pytest.mark.parametrize("hw", [(8, 8), (33, 47), (64, 64), (40, 24)], ids=str)
def test_the_limits_of_the_identity_are_the_whole_image(hw):
    H, W = hw
    assert R.common_limits(np.stack([R.identity()] * 3), H, W).tolist() == [0, 0, W, H]
    shifted = np.array([[1, 0, 3 / (max(H, W) / 2)], [0, 1, 0]], np.float64)   # samples 3 px to the right: its content sits 3 px to the left
    assert R.common_limits(np.stack([R.identity(), shifted]), H, W).tolist() == [0, 0, W - 3, H]
    assert R.common_limits(np.array([[[np.nan, 0, 0], [0, 1, 0]]]), H, W).tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("W", [16, 48, 64, 3800])
def test_the_parameters_carry_across_a_pyramid_level(W):
    coarse, fine = R.pyramid_coordinates(W)
    assert np.array_equal(coarse, fine)


def test_to_pixel_matrix_agrees_with_the_pull_map():
    H, W = 33, 47
    T = R.similarity(3.0, 0.97, (2.5, -1.25), H, W)
    M = affine.to_pixel_matrix(T, H, W)
    x, y = np.array([0.0, 46, 10.5]), np.array([0.0, 32, 7.25])
    xs, ys = R.pull(T, H, W, x, y)
    got = M @ np.stack([x, y, np.ones(3)])
    assert np.abs(got[0] - xs).max() <= 1e-12 and np.abs(got[1] - ys).max() <= 1e-12 and got[2].tolist() == [1, 1, 1]
    assert np.array_equal(affine.from_similarity(3.0, 0.97, (2.5, -1.25), H, W), T)


def test_box_muller_moments():
    """10^5 draws; the bars are four standard errors of the sample moments of a standard normal: 1/sqrt(n) for the mean, sqrt(2/n)
    for the variance, sqrt(6/n) for the skewness, sqrt(24/n) for the kurtosis."""
    z = R.normals(16667, 1, seed=3).ravel()[:100000]
    n = z.size
    m, v = z.mean(), z.var()
    skew, kurt = ((z - m) ** 3).mean() / v ** 1.5, ((z - m) ** 4).mean() / v ** 2
    print(f"Box-Muller over {n} draws: mean {m:.4f}, variance {v:.4f}, skewness {skew:.4f}, kurtosis {kurt:.4f}")
    assert abs(m) <= 4 / np.sqrt(n) and abs(v - 1) <= 4 * np.sqrt(2 / n) and abs(skew) <= 4 * np.sqrt(6 / n) and abs(kurt - 3) <= 4 * np.sqrt(24 / n)
    assert np.abs(z).max() <= np.sqrt(-2 * np.log(2.0 ** -33))
    s, c = R.sincospi(np.array([0.0, 0.25, 0.5, 1.0, 1.5, 1.75]))
    assert s[[0, 3]].tolist() == [0, 0] and c[[2, 4]].tolist() == [0, 0] and s[2] == 1 and c[3] == -1 and s[4] == -1
    assert abs(s[1] - np.sqrt(0.5)) <= 2.0 ** -53 and abs(c[5] - np.sqrt(0.5)) <= 2.0 ** -53


def test_the_samples_are_inside_and_repeat():
    s = R.draw_samples(1000, 33, 47, seed=9)
    assert s.dtype == np.uint32 and s.max() < 33 * 47 and len(np.unique(s)) < 1000
    assert np.array_equal(R.draw_samples(5, 33, 47, seed=9), s[:5])


def test_mutual_information_is_indifferent_to_a_contrast_reversal():
    fixed, moving, T = R.recovery_inputs()
    at_truth, at_identity = R.mutual_information(fixed, moving, T), R.mutual_information(fixed, moving, R.identity())
    print(f"MI of the recovery pair: {at_truth:.4f} at the true transform, {at_identity:.4f} at the identity")
    assert at_truth > at_identity + 0.5
    assert R.mutual_information(fixed, np.zeros_like(moving), T) == 0.0
    assert R.mutual_information(fixed, moving, [[1, 0, 9.0], [0, 1, 0]]) == 0.0   # everything outside


# ---- the C entry points' checks: before any launch ----------------------------------------------------------------------------------

def _err():
    return _lib.load().emd_last_error().decode()


def test_c_argument_checks_need_no_gpu():
    lib = _lib.load()
    null = None
    a, b, c, d, e = (C.c_void_p(v) for v in (1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20))   # far apart, 16-byte aligned, never touched
    odd = C.c_void_p((6 << 20) + 4)
    for H, W in ((7, 64), (64, 4097), (0, 0)):
        assert lib.emd_warp_affine_f32(a, 1, H, W, c, 0, 0.0, b, null) == -1 and "bad shape" in _err()
        assert lib.emd_mattes_mi_workspace_bytes(1, H, W, 0, 50) == 0
        assert lib.emd_mattes_mi_f64(a, b, 1, H, W, c, null, 0, 50, d, e, null, a, 1 << 30, null) == -1 and "H and W 8..4096" in _err()
        assert lib.emd_mi_samples_u32(10, H, W, 0, a, null) == -1 and "bad shape" in _err()
        assert lib.emd_affine_limits_i32(a, 2, H, W, b, null) == -1 and "bad shape" in _err()
    assert lib.emd_warp_affine_f32(a, 0, 8, 8, c, 0, 0.0, b, null) == -1 and "1..65535 images" in _err()
    for bins in (7, 65):
        assert lib.emd_mattes_mi_workspace_bytes(1, 64, 64, 0, bins) == 0
        assert lib.emd_mattes_mi_f64(a, b, 1, 64, 64, c, null, 0, bins, d, e, null, a, 1 << 30, null) == -1 and "bins 8..64" in _err()
        assert lib.emd_affine_register_f64(a, b, 1, 64, 64, null, 0, bins, 1e-3, 1.05, 1e-6, 0, null, 0, 1, null, 0, 1, d, c, 1 << 30,
                                           null) == -1 and "bins 8..64" in _err()
    for P in (0, 65):                                                        # P = 0 is an error, not a no-op: there is no state to return
        assert lib.emd_mattes_mi_workspace_bytes(P, 64, 64, 0, 50) == 0
        assert lib.emd_mattes_mi_f64(a, b, P, 64, 64, c, null, 0, 50, d, e, null, a, 1 << 30, null) == -1 and "1..64 pairs" in _err()
        assert lib.emd_affine_register_f64(a, b, P, 64, 64, null, 0, 50, 1e-3, 1.05, 1e-6, 0, null, 0, 1, null, 0, 1, d, c, 1 << 30,
                                           null) == -1 and "1..64 pairs" in _err()
        assert lib.emd_affine_normals_f64(4, P, 0, 0, a, null) == -1
    need = lib.emd_mattes_mi_workspace_bytes(2, 64, 64, 0, 50)
    assert need >= 2 * 4 * 2500 * 8 and need % 256 == 0
    far = C.c_void_p(64 << 20)                                               # the workspace: clear of everything else
    # null pointers
    assert lib.emd_warp_affine_f32(null, 1, 8, 8, c, 0, 0.0, b, null) == -1 and "null pointer" in _err()
    assert lib.emd_warp_affine_f32(a, 1, 8, 8, null, 0, 0.0, b, null) == -1 and "null pointer" in _err()
    assert lib.emd_mattes_mi_f64(a, b, 2, 64, 64, c, null, 0, 50, null, e, null, far, need, null) == -1 and "null pointer" in _err()
    assert lib.emd_mattes_mi_f64(a, b, 2, 64, 64, c, null, 0, 50, d, e, null, null, need, null) == -1 and "null pointer" in _err()
    assert lib.emd_affine_chain_f64(null, 3, 1, b, null) == -1 and "null pointer" in _err()
    assert lib.emd_mi_samples_u32(10, 8, 8, 0, null, null) == -1 and "null pointer" in _err()
    # samples and n go together; so do variates and their rows
    assert lib.emd_mattes_mi_f64(a, b, 2, 64, 64, c, null, 100, 50, d, e, null, far, need, null) == -1 and "bad shape" in _err()
    assert lib.emd_affine_register_f64(a, b, 2, 64, 64, null, 0, 50, 1e-3, 1.05, 1e-6, 0, c, 0, 1, null, 0, 1, d, far, need, null) == -1
    assert "variates_rows" in _err()
    assert lib.emd_affine_register_f64(a, b, 2, 64, 64, null, 0, 50, 1e-3, 1.05, 1e-6, 0, null, 0, 3, null, 0, 1, d, far, need, null) == -1
    assert lib.emd_affine_register_f64(a, b, 2, 64, 64, null, 0, 50, 1e-3, 1.0, 1e-6, 0, null, 0, 1, null, 0, 1, d, far, need, null) == -1
    assert "growth > 1" in _err()
    # misalignment
    assert lib.emd_warp_affine_f32(a, 1, 8, 8, odd, 0, 0.0, b, null) == -3 and "8-byte aligned" in _err()
    assert lib.emd_mattes_mi_f64(a, b, 2, 64, 64, c, null, 0, 50, odd, e, null, far, need, null) == -3 and "aligned" in _err()
    assert lib.emd_mattes_mi_f64(a, b, 2, 64, 64, c, null, 0, 50, d, e, null, C.c_void_p((64 << 20) + 8), need, null) == -3
    assert lib.emd_affine_register_f64(a, b, 2, 64, 64, null, 0, 50, 1e-3, 1.05, 1e-6, 0, null, 0, 1, null, 0, 1, odd, far, need,
                                       null) == -3 and "aligned" in _err()
    # overlapping ranges: out on the images, the state inside the workspace; the two inputs may share bytes
    assert lib.emd_warp_affine_f32(a, 1, 8, 8, c, 0, 0.0, C.c_void_p((1 << 20) + 128), null) == -1 and "overlap" in _err()
    assert lib.emd_affine_register_f64(a, b, 2, 64, 64, null, 0, 50, 1e-3, 1.05, 1e-6, 0, null, 0, 1, null, 0, 1, C.c_void_p((64 << 20) + 256),
                                       far, need, null) == -1 and "overlap" in _err()
    assert lib.emd_mattes_mi_f64(a, b, 2, 64, 64, c, null, 0, 50, d, C.c_void_p((4 << 20) + 8), null, far, need, null) == -1 and "overlap" in _err()
    assert lib.emd_affine_chain_f64(a, 3, 1, C.c_void_p((1 << 20) + 16), null) == -1 and "overlap" in _err()
    # a short workspace
    assert lib.emd_mattes_mi_f64(a, b, 2, 64, 64, c, null, 0, 50, d, e, null, far, need - 1, null) == -1 and "workspace too small" in _err()
    assert lib.emd_affine_register_f64(a, b, 2, 64, 64, null, 0, 50, 1e-3, 1.05, 1e-6, 0, null, 0, 1, null, 0, 1, d, far, need - 1,
                                       null) == -1 and "workspace too small" in _err()
    # the chain's shape
    assert lib.emd_affine_chain_f64(a, 0, 0, b, null) == -1 and lib.emd_affine_chain_f64(a, 3, 3, b, null) == -1 and "middle" in _err()
    assert lib.emd_affine_chain_f64(a, 66, 1, b, null) == -1


# ---- the Python module's checks: before anything moves ------------------------------------------------------------------------------

def test_python_arguments_are_checked_before_anything_moves(monkeypatch):
    import torch

    def no_device(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")

    monkeypatch.setattr(torch.cuda, "current_device", no_device)
    monkeypatch.setattr(_lib, "load", no_device)
    img = np.zeros((2, 16, 16), np.float32)
    eye = np.stack([R.identity()] * 2)
    bad = [lambda: affine.warp(np.zeros((2, 7, 16), np.float32), eye),
           lambda: affine.warp(np.zeros((2, 16, 4097), np.float32), eye),
           lambda: affine.warp(np.zeros((2, 2, 16, 16), np.float32), eye),
           lambda: affine.warp(img.astype(np.complex64), eye),
           lambda: affine.warp(img, np.zeros((3, 2, 3))),
           lambda: affine.warp(img, eye, fill=np.inf),
           lambda: affine.draw_samples(0, 16, 16),
           lambda: affine.draw_samples(10, 16, 5000),
           lambda: affine.draw_samples(10, 16, 16, seed=-1),
           lambda: affine.mutual_information(img, img[:1], eye),
           lambda: affine.mutual_information(img, img, eye[0]),
           lambda: affine.mutual_information(img, img, eye, bins=7),
           lambda: affine.mutual_information(img, img, eye, bins=65),
           lambda: affine.mutual_information(img, img, eye, samples=np.zeros((2, 2), np.int32)),
           lambda: affine.mutual_information(np.zeros((65, 16, 16), np.float32), np.zeros((65, 16, 16), np.float32), np.zeros((65, 2, 3))),
           lambda: affine.normals(0, 1),
           lambda: affine.normals(4, 65),
           lambda: affine.register(img, img, iterations=0),
           lambda: affine.register(img, img, growth=1.0),
           lambda: affine.register(img, img, initial_radius=0.0),
           lambda: affine.register(img, img, epsilon=-1.0),
           lambda: affine.register(img, img, levels=0),
           lambda: affine.register(img, img, levels=3),                      # 16 / 4 = 4 < 8
           lambda: affine.register(np.zeros((1, 36, 36), np.float32), np.zeros((1, 36, 36), np.float32), levels=4),   # 36 % 8 != 0
           lambda: affine.register(img, img, levels=1, samples=0),
           lambda: affine.register(img, img, levels=2, samples=np.zeros(4, np.int32)),
           lambda: affine.register(img, img, levels=1, iterations=10, variates=np.zeros((9, 2, 6))),
           lambda: affine.register(img, img, levels=1, T0=np.zeros((3, 2, 3))),
           lambda: affine.register_series(img[:1]),
           lambda: affine.chain_to_middle(np.zeros((3, 3, 3))),
           lambda: affine.chain_to_middle(eye, middle=3),
           lambda: affine.common_limits(eye, 4, 16),
           lambda: affine.common_limits(np.zeros((2, 5)), 16, 16),
           lambda: affine.warp_stack(img, eye),                              # two images need one pair transform
           lambda: affine.warp_stack(img, eye[:1], middle=2),
           lambda: affine.warp_stack(img, eye[:1], fill=np.nan),
           lambda: affine.to_pixel_matrix(R.identity(), 4, 16)]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {k} was accepted")


# ---- the condition of the end-to-end recovery test ----------------------------------------------------------------------------------

def test_the_restatement_recovers_the_transform_with_the_philox_stream_of_seed_0():
    """600 evaluations, every pixel, one level, the Philox normals of seed 0: the four corners end within 0.5 px of the true transform
    (they start 4.16 px away), and no decision is closer than 1e-9 relative, so that a device whose MI differs in the last bits takes
    the same decisions.  Measured: 0.24 px, 32 accepted, the smallest margin 7.8e-5."""
    fixed, moving, T = R.recovery_inputs()
    start = R.corner_error(R.identity(), T, 64, 64)
    run = R.recovery_run()
    err = R.corner_error(run["T"], T, 64, 64)
    print(f"recovery on the CPU: {start:.3f} px at the identity, {err:.3f} px after {run['iterations']} evaluations, {run['accepted']} accepted, "
          f"smallest margin {min(run['margins']):.3e}, MI {run['f']:.6f}")
    assert start > 3.0 and err <= 0.5 and min(run["margins"]) >= 1e-9 and run["status"] == 0 and run["iterations"] == 600
