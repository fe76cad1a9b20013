"""CPU tests of the frequency fields of the harvester (emdenoise.harvest.rfft2 / radial_profile / freq_stats; csrc/fft.hip;
DESIGN.md 3.19): the restatement of tests/fft_ref.py against itself (the literal loop of img_params.m:59-69 against the vectorised
form), the bin count, argument validation at the C and the Python level, and the field mapping.  Nothing here touches a GPU."""
import ctypes as C

import numpy as np
import pytest

from emdenoise import _lib, harvest
from tests import fft_ref as F

BAD_SIZES = [0, 4, 7, 12, 100, 1000, 2047, 8192]


def test_literal_loop_equals_the_vectorised_restatement():
    rng = np.random.default_rng(7)
    for S in (8, 16, 32):
        mag = F.shifted_magnitude(rng.standard_normal((S, S)))
        pl, fl = F.profile_loop(mag)
        pv, fv = F.profile_vectorised(mag)
        print(f"S = {S}: largest profile distance {np.abs(pl - pv).max():.2e}; frequencies equal: {np.array_equal(fl, fv)}")
        assert np.array_equal(fl, fv) and np.array_equal(pl, pv)          # the same additions in the same order
        empty = np.flatnonzero(~F.radial_freqs(S)[1]).tolist()
        assert empty == {8: [7], 16: [], 32: [24]}[S]
        assert (fl[empty] == 0).all() and (pl[empty] == 0).all()


def test_radial_bins():
    lib = _lib.load()
    for S in F.valid_sizes():
        assert harvest.radial_bins(S) == F.radial_bins(S) == lib.emd_radial_bins(S), S
    assert harvest.radial_bins(2048) == 1450
    for S in BAD_SIZES:
        assert lib.emd_radial_bins(S) == 0, S


def test_ceil_sqrt_is_exact_at_squares_and_their_neighbours():
    r = np.arange(0, 2900, dtype=np.int64)
    assert np.array_equal(F.ceil_sqrt(r * r), r) and np.array_equal(F.ceil_sqrt(r * r + 1), r + 1)
    assert np.array_equal(F.ceil_sqrt(r[1:] * r[1:] - 1), np.where(r[1:] == 1, 0, r[1:]))


def test_c_argument_validation():
    lib = _lib.load()
    one, two, three, four = C.c_void_p(256), C.c_void_p(1 << 20), C.c_void_p(1 << 30), C.c_void_p(1 << 29)
    null = C.c_void_p(0)
    big = 1 << 28
    assert lib.emd_rfft2_workspace_bytes(2, 64) > 0 and lib.emd_freq_stats_workspace_bytes(2, 64) > lib.emd_rfft2_workspace_bytes(2, 64)
    assert lib.emd_rfft2_workspace_bytes(0, 64) == 0 and lib.emd_freq_stats_workspace_bytes(0, 64) == 0
    for S in BAD_SIZES:
        assert lib.emd_rfft2_workspace_bytes(1, S) == 0 and lib.emd_freq_stats_workspace_bytes(1, S) == 0
        assert lib.emd_rfft2_f64(one, 1, S, two, three, big, null) == -1 and b"shape" in lib.emd_last_error()
        assert lib.emd_freq_stats_f64(one, 1, S, null, two, three, big, null) == -1 and b"shape" in lib.emd_last_error()
    assert lib.emd_rfft2_f64(null, 1, 64, two, three, big, null) == -1 and b"null" in lib.emd_last_error()
    assert lib.emd_rfft2_f64(one, 1, 64, null, three, big, null) == -1 and b"null" in lib.emd_last_error()
    assert lib.emd_rfft2_f64(one, 1, 64, two, null, big, null) == -1 and b"null" in lib.emd_last_error()
    assert lib.emd_rfft2_f64(one, 1, 64, two, three, lib.emd_rfft2_workspace_bytes(1, 64) - 1, null) == -1
    assert b"workspace" in lib.emd_last_error()
    assert lib.emd_rfft2_f64(one, 0, 64, two, three, 0, null) == 0                                    # an empty batch: no-op
    assert lib.emd_freq_stats_f64(null, 1, 64, null, two, three, big, null) == -1 and b"null" in lib.emd_last_error()
    assert lib.emd_freq_stats_f64(one, 1, 64, null, null, three, big, null) == -1 and b"null" in lib.emd_last_error()
    assert lib.emd_freq_stats_f64(one, 1, 64, null, two, null, big, null) == -1 and b"null" in lib.emd_last_error()
    assert lib.emd_freq_stats_f64(one, 1, 64, four, two, three, lib.emd_freq_stats_workspace_bytes(1, 64) - 1, null) == -1
    assert b"workspace" in lib.emd_last_error()
    assert lib.emd_freq_stats_f64(one, 0, 64, null, two, three, 0, null) == 0
    assert lib.emd_freq_stats_f64(one, 1, 64, two, two, three, big, null) == -1 and b"overlap" in lib.emd_last_error()
    text = open(_lib.PKG_DIR + "/../include/emdenoise.h").read()
    assert "#define EMD_NFREQ 4" in text and "#define EMD_NSTATS 17" in text and harvest.NFREQ == 4


def test_python_arguments_are_checked_on_the_shape_before_anything_moves():
    """No GPU here: every one of these must raise before a tensor is created on a device."""
    for fn in (harvest.rfft2, harvest.radial_profile, harvest.freq_stats):
        for shape in ((12, 12), (16, 32), (2, 4, 4), (1, 8192, 8192), (2, 100, 100, 1)):
            with pytest.raises(ValueError, match="power of two"):
                fn(np.broadcast_to(np.float32(0), shape))
        with pytest.raises(ValueError, match=r"\[B,H,W,1\]"):
            fn(np.zeros((2, 3, 4, 5, 6), np.float32))
    for bad in BAD_SIZES[1:] + [2.5]:
        with pytest.raises(ValueError, match="size|power of two"):
            harvest.radial_bins(bad)
    for bad in (100, 12, 4, 8192):
        with pytest.raises(ValueError, match="power of two"):
            harvest.img_params(np.zeros((128, 128), np.float32), bad, freq=True)
        with pytest.raises(ValueError, match="power of two"):
            harvest.harvest([np.zeros((128, 128), np.float32)], bad, freq=True)
    with pytest.raises(ValueError, match="one image"):
        harvest.img_params(np.zeros((2, 8, 8), np.float32), 8, freq=True)
    stack, table = harvest.harvest([], 16, freq=True)
    assert stack.shape == (0, 16, 16, 1) and table == []


def test_freq_fields_are_apart_from_the_others():
    assert harvest.FREQ_NAMES == F.FREQ_NAMES == ["mean", "std", "skewness", "kurtosis"]
    assert harvest.FIELDS_FREQ == {"meanFreq2048": "mean", "stddevFreq2048": "std", "skewnessFreq2048": "skewness",
                                   "kurtosisFreq2048": "kurtosis"}
    others = set(harvest.FIELDS_RAW) | set(harvest.FIELDS_2048) | set(harvest.FIELDS_0TO1) | \
        {"smallestDim", "imageDims", "num_px", "proportionZero", "proportionNegative"}
    assert not set(harvest.FIELDS_FREQ) & others
    assert set(harvest.FIELDS_FREQ.values()) == set(harvest.FREQ_NAMES)


def test_restatement_moments_and_degenerate_images():
    z = F.freq_stats(np.zeros((16, 16), np.float32))
    assert np.isnan(z).all()                                              # 0 / 0 in the normalisation
    c = F.freq_stats(np.full((16, 16), 7.25, np.float32))
    print(f"constant image: {c}")
    assert c[0] == 0 and c[1] == 0 and np.isnan(c[2:]).all()             # all the energy in the bin whose frequency is 0
    p = np.array([0.0, 1.0, 3.0, 0.5, 0.25])
    m = F.moments(p)
    d = p - p.mean()
    assert m[0] == p.sum() and np.isclose(m[1], p.std(ddof=1)) and np.isclose(m[2], (d ** 3).mean() / (d ** 2).mean() ** 1.5)
    assert np.isclose(m[3], (d ** 4).mean() / (d ** 2).mean() ** 2)
