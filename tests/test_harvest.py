"""CPU tests of the harvester (emdenoise.harvest): the library's one copy of the box-resize table arithmetic
(emd_box_resize_table, a host function) against the restatement of MATLAB's general algorithm in tests/harvest_ref.py, argument
validation, and the field mapping of img_params.  Nothing here touches a GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest

from emdenoise import _lib, harvest
from tests import harvest_ref as R

SMALL_OUT = list(range(1, 65)) + [96, 160]
LARGE_IN = [4096, 2672, 4008, 3838, 3000]


def test_table_equals_the_restatement_and_ties_follow_the_double_arithmetic():
    """Every n_in in 1..400 x n_out in {1..64, 96, 160}, and the detector sizes -> 2048.  Among them are pairs where a candidate lands
    exactly on the window's edge in rational arithmetic and the double expressions put it on the other side: a table from an integer
    formula would differ there, so at least one such pair must be among the tested ones."""
    pairs = list(itertools.product(range(1, 401), SMALL_OUT)) + [(n, 2048) for n in LARGE_IN]
    tie_pairs = 0
    for n_in, n_out in pairs:
        want = R.runs(n_in, n_out)
        got = harvest.box_table(n_in, n_out)
        assert got.dtype == np.int32 and got.shape == (n_out, 2)
        assert np.array_equal(got, want), (n_in, n_out)
        tie_pairs += not np.array_equal(want, R.exact_runs(n_in, n_out))
    print(f"{len(pairs)} pairs, {tie_pairs} where the double arithmetic lands a tie differently from exact arithmetic")
    assert tie_pairs >= 1


def test_exact_runs_is_fraction_arithmetic():
    """The integer form used above is the definition evaluated with fractions.Fraction."""
    for n_in, n_out in ((7, 4), (12, 8), (150, 7), (5, 8), (37, 16), (3, 2), (100, 64)):
        e = R.exact_runs(n_in, n_out)
        for x in range(1, n_out + 1):
            members = [i for i in range(1, n_in + 1) if R.exact_member_fraction(n_in, n_out, x, i)]
            assert members == list(range(e[x - 1, 0] + 1, e[x - 1, 0] + 1 + e[x - 1, 1])), (n_in, n_out, x)


def test_table_known_values():
    assert harvest.box_table(8, 4).tolist() == [[0, 2], [2, 2], [4, 2], [6, 2]]
    assert harvest.box_table(64, 64).tolist() == [[i, 1] for i in range(64)]
    up = harvest.box_table(5, 8)
    assert (up[:, 1] == 1).all() and up[:, 0].min() == 0 and up[:, 0].max() == 4       # nearest neighbour
    t = harvest.box_table(150, 7)
    assert set(t[:, 1]) <= {21, 22} and t[:, 1].sum() == 150 and np.array_equal(t[1:, 0], np.cumsum(t[:-1, 1]))


def test_restatement_resize_is_the_mean_over_the_runs():
    rng = np.random.default_rng(5)
    x = rng.random((70, 131))
    t = R.runs(70, 32)
    want = np.array([[x[a:a + n, b:b + m].mean() for b, m in t] for a, n in t])
    assert np.allclose(R.box_resize(x, 32), want, rtol=1e-13, atol=0)


def test_argument_validation():
    lib = _lib.load()
    tab = (C.c_int * 8)()
    assert lib.emd_box_resize_table(8, 4, None) == -1 and b"null" in lib.emd_last_error()
    for n_in, n_out in ((0, 4), (32769, 4), (8, 0), (8, 8193)):
        assert lib.emd_box_resize_table(n_in, n_out, tab) == -1
    assert lib.emd_image_stats_workspace_bytes(1, 2, 100) == 0 and lib.emd_image_stats_workspace_bytes(1, 3, 32769) == 0
    assert lib.emd_image_stats_workspace_bytes(0, 64, 64) == 0 and lib.emd_image_stats_workspace_bytes(2, 64, 64) > 0
    one, two, three = C.c_void_p(256), C.c_void_p(1 << 20), C.c_void_p(1 << 30)
    null = C.c_void_p(0)
    assert lib.emd_image_stats_f64(one, 1, 2, 64, two, three, 1 << 20, null) == -1 and b"shape" in lib.emd_last_error()
    assert lib.emd_image_stats_f64(one, 1, 64, 64, two, three, 16, null) == -1 and b"workspace" in lib.emd_last_error()
    assert lib.emd_image_stats_f64(null, 1, 64, 64, two, three, 1 << 20, null) == -1 and b"null" in lib.emd_last_error()
    assert lib.emd_image_stats_f64(one, 0, 64, 64, two, three, 0, null) == 0                       # an empty batch: no-op
    assert lib.emd_box_resize_f32(one, 64, 8, 1, 8, three, 9000, two, null) == -1                    # S too large
    assert lib.emd_box_resize_f32(one, 64, 4, 1, 8, three, 4, two, null) == -1                       # row_stride < d
    assert lib.emd_box_resize_f32(null, 64, 8, 1, 8, three, 4, two, null) == -1 and b"null" in lib.emd_last_error()
    assert lib.emd_box_resize_f32(one, 64, 8, 1, 8, one, 4, two, null) == -1 and b"overlap" in lib.emd_last_error()
    assert lib.emd_box_resize_f32(one, 64, 8, 0, 8, three, 4, two, null) == 0
    assert lib.emd_scale01_f32(one, three, 1, 0, two, null) == -1
    assert lib.emd_scale01_f32(one, null, 1, 64, two, null) == -1 and b"null" in lib.emd_last_error()
    assert lib.emd_scale01_f32(one, C.c_void_p(260), 1, 64, two, null) == -1                         # a partial overlap


def test_python_arguments_are_checked_on_the_shape_before_anything_moves():
    """No GPU here: every one of these must raise before a tensor is created on a device."""
    img = np.zeros((2, 64), np.float32)
    for fn in (harvest.image_stats, harvest.scale01, harvest.estimate_noise):
        with pytest.raises(ValueError, match="3 <= H, W"):
            fn(img)
        with pytest.raises(ValueError, match=r"\[B,H,W,1\]"):
            fn(np.zeros((2, 3, 4, 5, 6), np.float32))
    for bad in (0, 8193, 2.5):
        with pytest.raises(ValueError, match="size"):
            harvest.box_resize(np.zeros((8, 8), np.float32), bad)
        with pytest.raises(ValueError, match="size"):
            harvest.img_params(np.zeros((8, 8), np.float32), bad)
    with pytest.raises(ValueError, match="one image"):
        harvest.img_params(np.zeros((2, 8, 8), np.float32), 4)
    with pytest.raises(ValueError, match="one image"):
        harvest.img_params_lq(np.zeros((2, 8, 8), np.float32), 4)
    with pytest.raises(ValueError, match="3 <= H, W"):
        harvest.harvest([np.zeros((2, 8), np.float32)], 4)
    with pytest.raises(ValueError, match="n_in"):
        harvest.box_table(0, 4)
    stack, table = harvest.harvest([], 16)
    assert stack.shape == (0, 16, 16, 1) and stack.dtype == np.float32 and table == []


def test_stat_names_match_the_field_mapping():
    assert harvest.STAT_NAMES == R.STAT_NAMES and len(harvest.STAT_NAMES) == harvest.NSTATS == 17
    for fields in (harvest.FIELDS_RAW, harvest.FIELDS_2048, harvest.FIELDS_0TO1):
        assert set(fields.values()) <= set(harvest.STAT_NAMES)
    # every statistic but the two counts is reported for the resized image; img_params.m has no skewness / kurtosis, min / max of
    # the scaled image (they are those of the resized one, and 0 / 1)
    assert set(harvest.FIELDS_2048.values()) == set(harvest.STAT_NAMES) - {"nonzero", "negative"}
    assert set(harvest.FIELDS_0TO1.values()) == set(harvest.FIELDS_2048.values()) - {"min", "max", "skewness", "kurtosis"}
    assert all(k.endswith("_for_0to1") or k == "rms_0to1" for k in harvest.FIELDS_0TO1)
    assert not (set(harvest.FIELDS_RAW) | {"smallestDim", "imageDims", "num_px", "proportionZero", "proportionNegative"}) & \
        (set(harvest.FIELDS_2048) | set(harvest.FIELDS_0TO1))
    assert not set(harvest.FIELDS_2048) & set(harvest.FIELDS_0TO1)
    assert not [k for k in list(harvest.FIELDS_2048) + list(harvest.FIELDS_0TO1) if "Freq" in k]       # the FFT fields are not built
    text = open(_lib.PKG_DIR + "/../include/emdenoise.h").read()
    assert "#define EMD_NSTATS 17" in text
