"""CPU tests of emdenoise.resample (csrc/resample.hip, csrc/resize_taps.hpp): the tap arithmetic, through the library's
host function ``emd_resize_taps`` (the code the kernel calls), against the numpy restatement of tests/resample_ref.py; that restatement
against independent statements; the refusals.  No GPU: nothing here launches."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from emdenoise import _lib, exitwave, resample
from emdenoise.denoiser import _resize_bilinear_host
from tests import resample_ref as R

MODES = ["nearest", "linear", "cubic", "area"]
LARGE = [(2001, 2000), (4096, 1024), (3000, 1000), (2048, 2047)]
# the other axis of the two area decisions: an equal pair keeps the rule to this axis, an enlarging pair forces the emulated form
OTHERS = [(None, None), (4, 8)]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def assert_same_table(n_in, n_out, mode, other):
    got = resample.taps(n_in, n_out, mode, *other)
    want = R.axis_taps(mode, n_in, n_out, *other)
    where = f"{mode} {n_in} -> {n_out}, other axis {other}"
    assert got.block == want.block, where
    assert np.array_equal(got.count, want.count), where
    assert got.index.shape == want.index.shape and np.array_equal(got.index, want.index), where
    assert np.array_equal(bits(got.weight), bits(want.weight)), where
    return got


def small_pairs():
    return [(n_in, n_out) for n_in in range(1, 97) for n_out in range(1, 97)]


@pytest.mark.parametrize("mode", MODES)
def test_taps_equal_the_restatement_for_every_small_pair(mode):
    for other in (OTHERS if mode == "area" else OTHERS[:1]):
        for n_in, n_out in small_pairs():
            assert_same_table(n_in, n_out, mode, other)


@pytest.mark.parametrize("pair", LARGE, ids=lambda p: f"{p[0]}-{p[1]}")
def test_taps_equal_the_restatement_for_the_large_pairs(pair):
    for mode in MODES:
        for other in (OTHERS if mode == "area" else OTHERS[:1]):
            assert_same_table(*pair, mode, other)


def test_the_sliver_rule_fires_at_2001_to_2000():
    t = resample.taps(2001, 2000, "area")
    assert t.block == 0 and t.count[0] == 1 and t.index[0, 0] == 0
    s = float(t.weight[0].sum())
    print(f"2001 -> 2000 area, sample 0: {t.count[0]} tap, weights sum to {s!r} (1 / 1.0005 = {1 / 1.0005!r})")
    assert abs(s - 1 / 1.0005) < 1e-7
    for n_in in range(1, 200):                                             # never below 200
        for n_out in range(1, n_in + 1):
            w = R.axis_taps("area", n_in, n_out).weight.sum(axis=1)
            assert np.abs(w - 1.0).max() < 5.8e-8, (n_in, n_out)


def test_invariants():
    pairs = small_pairs()[::7] + LARGE
    for n_in, n_out in pairs:
        scale = 1.0 / (n_out / n_in)
        for mode in MODES:
            for other in (OTHERS if mode == "area" else OTHERS[:1]):
                t = resample.taps(n_in, n_out, mode, *other)
                assert t.index.min() >= 0 and t.index.max() <= n_in - 1 and (t.count >= 1).all(), (mode, n_in, n_out)
                if mode == "area":
                    assert (t.weight >= 0.0).all(), (n_in, n_out)
                    if other[0] is None and n_out <= n_in:
                        assert t.count.max() <= math.ceil(scale) + 1, (n_in, n_out)


def test_whole_ratios_take_the_block_form():
    missed = [(n_in, k) for k in (2, 3, 4, 5, 7, 8) for n_in in range(k, 4097, k) if resample.taps(n_in, n_in // k, "area").block != k]
    assert not missed, missed[:10]
    t = resample.taps(12, 4, "area")
    assert np.array_equal(t.index, np.arange(12).reshape(4, 3)) and np.array_equal(t.weight, np.full((4, 3), 1.0 / 3.0))
    assert resample.taps(12, 4, "area", 4, 8).block == 0                  # the other axis enlarges: emulated area, the LINEAR form
    assert resample.taps(12, 4, "area", 7, 3).block == 0                  # the other axis is no whole ratio: runs
    assert np.allclose(resample.taps(12, 4, "area", 7, 3).weight, 1.0 / 3.0, atol=1e-7)


@pytest.mark.parametrize("n", [1, 2, 5, 64, 2048])
def test_equal_sizes_have_weights_exactly_zero_and_one(n):
    for mode in ("nearest", "area"):
        t = resample.taps(n, n, mode)
        assert t.index.shape == (n, 1) and np.array_equal(t.index[:, 0], np.arange(n)) and np.array_equal(t.weight, np.ones((n, 1)))
    for mode, at in (("linear", 0), ("cubic", 1)):
        t = resample.taps(n, n, mode)
        want = np.zeros_like(t.weight)
        want[:, at] = 1.0
        assert np.array_equal(t.weight, want) and np.array_equal(t.index[:, at], np.arange(n)), mode


# ---- the float64 restatement against independent statements --------------------------------------------------------------------

def image(H, W, seed=0):
    return (np.random.default_rng(seed).random((H, W)) * 900.0 - 40.0).astype(np.float32)


@pytest.mark.parametrize("shape,out", [((48, 64), (16, 16)), ((40, 40), (20, 20)), ((2100, 9), (5, 9)), ((64, 64), (64, 64))])
def test_whole_ratio_area_is_the_block_mean(shape, out):
    (H, W), (h, w) = shape, out
    x = image(H, W)
    want = x.astype(np.float64).reshape(h, H // h, w, W // w).mean((1, 3))
    got = R.resize(x, (w, h), "area")
    # 1.0 / (5.0 / 2100.0) is not 420.0 in double, so by cv2's rule 2100 -> 5 is no whole ratio: runs of 420 with the float32 weight
    # (float)(1 / 420.00000000000006), the block mean to float32 precision only
    block = resample.taps(H, h, "area", W, w).block
    assert block == (0 if H == 2100 else H // h) and R.whole_block(H, h) == block
    assert np.abs(got - want).max() <= (1e-12 if block else 6e-8) * np.abs(want).max()


@pytest.mark.parametrize("n_in,n_out", [(64, 16), (16, 64), (40, 20)])
def test_linear_equals_the_numpy_restatement_of_the_denoiser_at_exact_ratios(n_in, n_out):
    x = image(n_in, n_in, 1)
    want = _resize_bilinear_host(x, (n_out, n_out)).astype(np.float64)     # it returns float32: half an ulp is all that may differ
    got = R.resize(x, n_out, "linear")
    assert (np.abs(got - want) <= 2.0 ** -24 * (1 + 1e-9) * np.abs(want)).all()
    # and before that rounding, against its formula kept in float64
    src = (np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5
    lo = np.floor(src).astype(int)
    fr = src - lo
    M = np.zeros((n_out, n_in))
    np.add.at(M, (np.arange(n_out), np.clip(lo, 0, n_in - 1)), 1 - fr)
    np.add.at(M, (np.arange(n_out), np.clip(lo + 1, 0, n_in - 1)), fr)
    full = M @ x.astype(np.float64) @ M.T
    assert np.abs(got - full).max() <= 1e-12 * np.abs(full).max()


def test_linear_at_exactly_two_is_area_at_two():
    x = image(40, 56, 2)
    a, b = R.resize(x, (28, 20), "linear"), R.resize(x, (28, 20), "area")
    assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()


@pytest.mark.parametrize("mode", MODES)
def test_a_constant_image_stays_constant(mode):
    for (H, W), (h, w) in (((37, 53), (16, 20)), ((17, 23), (40, 31)), ((33, 65), (50, 20)), ((5, 1), (2, 4)), ((130, 70), (129, 69))):
        y = R.resize(np.full((H, W), 7.25, np.float32), (w, h), mode)
        assert np.abs(y / 7.25 - 1.0).max() <= 1e-6, (mode, H, W, h, w)
    y = R.resize(np.full((1, 2001), 7.25, np.float32), (2000, 1), mode)    # the sliver rule's case: within 1e-3, not 1e-6
    e = float(np.abs(y / 7.25 - 1.0).max())
    print(f"{mode} 1 x 2001 -> 1 x 2000 of a constant: largest relative distance {e:.3e}")
    assert e <= 1e-3


def test_cubic_reproduces_a_ramp_in_the_interior():
    """The weights of Keys' kernel sum to 1 for every A, and their first moment about the sample's coordinate is
    -(2 A + 1) f (f - 1) (2 f - 1): zero for every f only at A = -0.5.  With cv2's A = -0.75 a ramp of slope m is therefore reproduced
    exactly where f is 0 or 1/2 (64 -> 16, 40 -> 20, 32 -> 32) and comes out m (0.5) f (f - 1) (2 f - 1) off elsewhere (16 -> 64:
    f = 1/8, 3/8, 5/8, 7/8) -- asserted as an identity, in the interior: the samples whose four taps are unclamped."""
    A, m = -0.75, 3.0
    for n_in, n_out, exact in ((64, 16, True), (40, 20, True), (32, 32, True), (16, 64, False), (16, 32, False)):
        t = R.axis_taps("cubic", n_in, n_out)
        coord = (np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5               # exact in float32 at these ratios
        s = np.floor(coord).astype(int)
        f = coord - s
        inner = (s - 1 >= 0) & (s + 2 <= n_in - 1)
        assert inner.any()
        ramp = m * np.arange(n_in) - 5.0
        got = (t.weight * ramp[t.index]).sum(axis=1)
        moment = -(2 * A + 1) * f * (f - 1) * (2 * f - 1)
        assert (np.abs(moment) < 1e-15).all() == exact
        want = m * (coord + moment) - 5.0
        assert np.abs(got - want)[inner].max() <= 1e-12 * np.abs(want).max(), (n_in, n_out)


def test_float32_variant_is_close_and_not_identical():
    x = image(37, 53, 3)
    for mode in MODES[1:]:
        a, b = R.resize(x, (20, 16), mode), R.resize(x, (20, 16), mode, np.float32)
        e = np.linalg.norm(a - b) / np.linalg.norm(a)
        assert b.dtype == np.float32 and 0.0 < e < 1e-6, (mode, e)


# ---- refusals ------------------------------------------------------------------------------------------------------------------

def test_python_refusals_come_before_the_device():
    x = np.zeros((2, 8, 9), np.float32)
    boxes = np.array([[0, 0, 9, 8], [1, 1, 2, 2]], np.int32)
    bad = [
        lambda: resample.resize(x, 4, "lanczos"), lambda: resample.resize(x, 4, 4), lambda: resample.resize(x, 4, -1),
        lambda: resample.resize(x, 4, None), lambda: resample.resize(x, 4, True),
        lambda: resample.resize(x, 0), lambda: resample.resize(x, 8193), lambda: resample.resize(x, (4, 0)), lambda: resample.resize(x, (8193, 4)),
        lambda: resample.resize(x, (4, 4, 4)), lambda: resample.resize(x, 4.0),
        lambda: resample.resize(x.astype(np.float64), 4), lambda: resample.resize(x.astype(np.int32), 4),
        lambda: resample.resize(torch.zeros(2, 8, 9, dtype=torch.float64), 4),
        lambda: resample.resize(np.zeros((2, 8, 9, 1), np.float32), 4), lambda: resample.resize(np.zeros(8, np.float32), 4),
        lambda: resample.crop_resize(x, None, 4),
        lambda: resample.crop_resize(x, boxes[:1], 4), lambda: resample.crop_resize(x, boxes.reshape(8), 4),
        lambda: resample.crop_resize(x, boxes[:, :3], 4), lambda: resample.crop_resize(x, boxes.astype(np.float32), 4),
        lambda: resample.crop_resize(x, np.array([[0, 0, 10, 8], [0, 0, 1, 1]]), 4),       # wider than the image
        lambda: resample.crop_resize(x, np.array([[0, 0, 9, 8], [8, 7, 2, 1]]), 4),        # past the right edge
        lambda: resample.crop_resize(x, np.array([[0, 0, 9, 8], [0, -1, 1, 1]]), 4),       # above the top
        lambda: resample.crop_resize(x, np.array([[0, 0, 9, 8], [0, 0, 0, 1]]), 4),        # empty
        lambda: resample.crop_resize(x, np.array([[0, 0, 9, 8], [0, 1, 1, 8]]), 4),        # past the bottom
        lambda: resample.taps(0, 4, "area"), lambda: resample.taps(4, 8193, "area"), lambda: resample.taps(32769, 4, "linear"),
        lambda: resample.taps(4, 4, "spline"), lambda: resample.taps(4, 4, "area", 0, 4),
        lambda: exitwave.resize_stack(x[0], 4), lambda: exitwave.resize_stack(x, 0),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"refusal {k} did not raise")
    with pytest.raises(ValueError, match="crop_resize: box 1 = \\(8, 7, 2, 1\\)"):
        resample.crop_resize(x, np.array([[0, 0, 9, 8], [8, 7, 2, 1]]), 4)
    with pytest.raises(ValueError, match="resize: dsize must be an integer, 1..8192 \\(got 8193\\)"):
        resample.resize(x, 8193)


def test_c_entry_validation_needs_no_gpu():
    lib = _lib.load()
    null, st = C.c_void_p(0), C.c_void_p(0)
    x, y = C.c_void_p(4096), C.c_void_p(1 << 20)
    call = lambda *a: lib.emd_resize_f32(*a)
    assert call(null, 64, 8, 1, 8, 8, null, y, 4, 4, 1, st) == -1 and b"null" in lib.emd_last_error()
    assert call(x, 64, 8, 1, 8, 8, null, null, 4, 4, 1, st) == -1 and b"null" in lib.emd_last_error()
    assert call(x, 64, 8, 1, 8, 8, null, x, 4, 4, 1, st) == -1 and b"overlap" in lib.emd_last_error()
    assert call(x, 64, 8, 2, 8, 8, null, C.c_void_p(4096 + 4 * 127), 4, 4, 1, st) == -1 and b"overlap" in lib.emd_last_error()   # y at x's last pixel
    assert call(x, 64, 8, 1, 8, 8, y, y, 4, 4, 1, st) == -1 and b"boxes" in lib.emd_last_error()
    for bad in ((x, 64, 8, 1, 0, 8, null, y, 4, 4, 1), (x, 64, 8, 1, 8, 32769, null, y, 4, 4, 1), (x, 64, 8, 1, 8, 8, null, y, 0, 4, 1),
                (x, 64, 8, 1, 8, 8, null, y, 4, 8193, 1), (x, 64, 8, 65536, 8, 8, null, y, 4, 4, 1), (x, 64, 8, -1, 8, 8, null, y, 4, 4, 1),
                (x, 64, 8, 1, 8, 8, null, y, 4, 4, 4), (x, 64, 8, 1, 8, 8, null, y, 4, 4, -1), (x, 64, 7, 1, 8, 8, null, y, 4, 4, 1),
                (x, -1, 8, 1, 8, 8, null, y, 4, 4, 1)):
        assert call(*bad, st) == -1 and lib.emd_last_error().startswith(b"emd_resize_f32"), bad
    assert call(null, 64, 8, 0, 8, 8, null, null, 4, 4, 1, st) == 0                # an empty batch is a no-op
    first, count, w, block = (C.c_int * 4)(), (C.c_int * 4)(), (C.c_double * 16)(), C.c_int(0)
    p = lambda a: C.cast(a, C.c_void_p)
    assert lib.emd_resize_taps(3, 8, 4, 8, 4, p(first), p(count), p(w), C.cast(C.byref(block), C.c_void_p)) == 0 and block.value == 2
    assert lib.emd_resize_taps(3, 8, 4, 8, 4, null, p(count), p(w), C.cast(C.byref(block), C.c_void_p)) == -1
    assert lib.emd_resize_taps(5, 8, 4, 8, 4, p(first), p(count), p(w), C.cast(C.byref(block), C.c_void_p)) == -1
    assert lib.emd_resize_taps(3, 8, 0, 8, 4, p(first), p(count), p(w), C.cast(C.byref(block), C.c_void_p)) == -1
