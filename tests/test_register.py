"""CPU tests of the registration of a focal series (emdenoise.exitwave, csrc/register.hip): the restatement of
tests/register_ref.py against known shifts and against itself (its two FFT back ends), the conditions the GPU tests' cases rest on,
``largest_crop_side``, the workspace size, and argument validation at the C and the Python level.  Nothing here touches a GPU."""
import ctypes as C

import numpy as np
import pytest

from emdenoise import _lib, exitwave
from tests import register_ref as R
from tests.test_register_gpu import (CANCEL_MAX, MARGIN_MIN, PC_CHAIN, PC_WINDOW, SIGN_OFFSETS, YARD_SHIFT, YARD_SHIFT_HALF, YARD_SURFACE,
                                     YARD_SURFACE_HALF, image, rolled, sign_inputs, yardstick)


@pytest.mark.parametrize("S", [8, 16, 32, 64, 128, 256])
def test_the_restatement_recovers_integer_circular_shifts(S):
    x = image(S)
    h = S // 2 - 1
    for d in ((0, 0), (h, h), (-h, -h), (h, -h), (1, 0), (0, -2), (-3, 2)):
        for fft in (R.NumpyFFT, R.Radix2FFT):
            r = R.phase_correlate(x, rolled(x, *d), fft=fft)
            e = float(np.abs(r["shift"] - np.array(d)).max())
            assert e <= 1e-12 and abs(r["response"] - 1.0) <= 1e-12 and r["margin"] >= 0.99, (S, d, fft.__name__, r["shift"], r["response"])
            assert R.peak_of(r["surface"]) == (S // 2 - d[1], S // 2 - d[0])
    w = R.hanning_window(S)
    assert w.shape == (S, S) and w[0, 0] == 0.0 and np.array_equal(w, w.T) and abs(w[S // 2, S // 2] - 1.0) < 4.0 / S ** 2 + 1e-15


def test_the_two_back_ends_agree_within_the_yardsticks_and_the_cases_meet_their_conditions():
    """Every case the GPU tests run, the 2048 x 2048 chain included: the constants of test_register_gpu are the largest distances of
    the restatement's two back ends (rounded up in the last digit), and every case meets the conditions of its bars."""
    worst, conditions = yardstick()
    print(worst)
    assert worst["surface"] <= YARD_SURFACE <= 1.001 * worst["surface"] and worst["shift"] <= YARD_SHIFT <= 1.001 * worst["shift"]
    assert worst["surface_half"] <= YARD_SURFACE_HALF <= 1.001 * worst["surface_half"]
    assert worst["shift_half"] <= YARD_SHIFT_HALF <= 1.001 * worst["shift_half"]
    for what, margin, cancellation in conditions:
        assert margin >= MARGIN_MIN and cancellation <= CANCEL_MAX, what
    assert YARD_SURFACE_HALF > 1e4 * YARD_SURFACE                          # why the half-pixel case keeps a yardstick of its own


def test_the_sign_cases_precondition_and_the_other_order():
    field, st = sign_inputs()
    d = np.diff(np.array(SIGN_OFFSETS, np.float64), axis=0)
    assert np.abs(R.chain_shifts(st) - d).max() <= 1e-9
    cut_last = np.stack([rolled(field, *o)[16:80, 16:80] for o in SIGN_OFFSETS])   # rolled at 96 x 96, then cut: no circular shifts
    e = float(np.abs(R.chain_shifts(cut_last) - d).max())
    print(f"rolled, then cut: the restatement is {e:.3f} px from the offsets' differences")
    assert e > 1e-3
    centres = R.centres_of(d, 64)
    assert np.allclose(centres - np.array(SIGN_OFFSETS), 32.0 - np.array(SIGN_OFFSETS).mean(0), rtol=0, atol=1e-13)
    crops = R.crop_stack(st, centres, 32)
    assert all(np.array_equal(crops[k], crops[0]) for k in range(4))


def test_restated_crop():
    x = np.arange(36, dtype=np.float32).reshape(1, 6, 6)
    assert np.array_equal(R.crop_stack(x, [(3.0, 3.0)], 2)[0], x[0, 2:4, 2:4])
    assert np.array_equal(R.crop_stack(x, [(3.5, 3.0)], 2)[0], (x[0, 2:4, 2:4] + x[0, 2:4, 3:5]) / 2)
    assert np.array_equal(R.crop_stack(x, [(3.0, 3.25)], 2)[0], 0.75 * x[0, 2:4, 2:4] + 0.25 * x[0, 3:5, 2:4])
    assert np.array_equal(R.crop_stack(x, [(0.0, 0.0)], 2, 9.0)[0], np.array([[9, 9], [9, 0]], np.float32))
    assert np.array_equal(R.crop_stack(x, [(3.0, 3.0)], 6)[0], x[0]) and (R.crop_stack(x, [(100.0, -50.0)], 3, 2.5) == 2.5).all()
    assert np.array_equal(R.crop_stack(x, [(6.0, 6.0)], 2, -1.0)[0], np.array([[35, -1], [-1, -1]], np.float32))


def test_largest_crop_side():
    c = np.array([(32.3, 30.3), (35.3, 33.3), (28.4, 31.0)])
    assert exitwave.largest_crop_side(c, 64, power_of_two=False) == 56 == R.largest_crop_side(c, 64, False)
    assert exitwave.largest_crop_side(c, 64) == 32 == R.largest_crop_side(c, 64)
    assert exitwave.largest_crop_side([(32.0, 32.0)], 64) == 64 and exitwave.largest_crop_side([(32.0, 32.5)], 64) == 32
    assert exitwave.largest_crop_side([(40.0, 32.0), (32.0, 20.25)], 64, power_of_two=False) == 40
    for bad in ([(0.0, 3.0)], [(70.0, 3.0)], [(float("nan"), 3.0)], [1.0, 2.0], np.zeros((0, 2))):
        with pytest.raises(ValueError, match="centre"):
            exitwave.largest_crop_side(bad, 64)


def test_workspace_size():
    lib = _lib.load()
    r = lambda n: (n + 255) & ~255
    for P, S, flags in ((1, 8, 0), (3, 64, 0), (3, 64, 2), (2, 256, 3), (64, 32, 2), (1, 4096, 2)):
        nimg = P + 1 if flags & 2 else 2 * P
        want = r(S * 16) + r(S * 8) + r(nimg * S * S * 16) + r(P * S * S * 16) + r(P * S * S * 8) + r(P * (S // 8) * 8) + r(P * (S // 8) * 4)
        assert lib.emd_phase_correlate_workspace_bytes(P, S, flags) == want, (P, S, flags)
    for P, S, flags in ((0, 64, 0), (65, 64, 0), (-1, 64, 2), (1, 4, 0), (1, 12, 0), (1, 100, 0), (1, 8192, 0), (1, 64, 4), (1, 64, -1)):
        assert lib.emd_phase_correlate_workspace_bytes(P, S, flags) == 0, (P, S, flags)


def test_c_argument_validation():
    lib = _lib.load()
    a, b, c, d, f = (C.c_void_p(v) for v in (1 << 20, 2 << 20, 3 << 20, 4 << 20, 1 << 30))
    null, big = C.c_void_p(0), 1 << 28
    err = lib.emd_last_error
    pc = lib.emd_phase_correlate_f64
    # shapes
    for S in (0, 4, 7, 12, 100, 1000, 8192):
        assert pc(a, b, 1, S, 0, c, null, f, big, null) == -1 and b"shape" in err()
        assert lib.emd_hanning_window_f64(S, a, b, null) == -1 and b"shape" in err()
    for P in (0, -1, 65):
        assert pc(a, b, P, 64, 0, c, null, f, big, null) == -1 and b"shape" in err() and b"pairs" in err()
    assert pc(a, b, 1, 64, 4, c, null, f, big, null) == -1 and b"flags" in err()
    assert pc(a, b, 1, 64, 2, c, null, f, big, null) == -1 and b"EMD_PC_CHAIN" in err()     # chain mode takes no b
    for N, S in ((1, 64), (66, 64), (0, 64), (3, 0), (3, 4097)):
        assert lib.emd_stack_centres_f64(a, N, S, b, null) == -1 and b"shape" in err()
    for N, S, side in ((0, 64, 8), (65536, 64, 8), (2, 0, 1), (2, 4097, 8), (2, 64, 0), (2, 64, 65), (2, 64, -3)):
        assert lib.emd_crop_stack_f32(a, N, S, b, side, 0.0, c, null) == -1 and b"shape" in err()
    # null pointers
    for args in ((null, b, 1, 64, 0, c, d, f), (a, null, 1, 64, 0, c, d, f), (a, b, 1, 64, 0, null, d, f), (a, b, 1, 64, 0, c, d, null),
                 (null, null, 1, 64, 2, c, d, f)):
        assert pc(*args, big, null) == -1 and b"null" in err()
    assert lib.emd_hanning_window_f64(64, null, null, null) == -1 and b"null" in err()
    assert lib.emd_stack_centres_f64(null, 3, 64, b, null) == -1 and b"null" in err()
    assert lib.emd_stack_centres_f64(a, 3, 64, null, null) == -1 and b"null" in err()
    for args in ((null, 2, 64, b, 8, 0.0, c), (a, 2, 64, null, 8, 0.0, c), (a, 2, 64, b, 8, 0.0, null)):
        assert lib.emd_crop_stack_f32(*args, null) == -1 and b"null" in err()
    # a short workspace
    for flags in (0, 2, 3):
        short = lib.emd_phase_correlate_workspace_bytes(2, 64, flags) - 1
        assert pc(a, null if flags & 2 else b, 2, 64, flags, c, null, f, short, null) == -1 and b"workspace" in err()
    # alignment: 16 bytes for the workspace, 8 for doubles, 4 for images
    odd4, odd2 = C.c_void_p((3 << 20) + 4), C.c_void_p((1 << 20) + 2)
    assert pc(a, b, 1, 64, 0, c, null, C.c_void_p((1 << 30) + 8), big, null) == -3 and b"aligned" in err()
    assert pc(a, b, 1, 64, 0, odd4, null, f, big, null) == -3 and b"aligned" in err()
    assert pc(a, b, 1, 64, 0, c, C.c_void_p((4 << 20) + 4), f, big, null) == -3 and b"aligned" in err()
    assert pc(odd2, b, 1, 64, 0, c, null, f, big, null) == -3 and b"aligned" in err()
    assert lib.emd_stack_centres_f64(odd4, 3, 64, b, null) == -3 and lib.emd_stack_centres_f64(a, 3, 64, odd4, null) == -3
    assert lib.emd_crop_stack_f32(odd2, 2, 64, b, 8, 0.0, c, null) == -3 and lib.emd_crop_stack_f32(a, 2, 64, odd4, 8, 0.0, c, null) == -3
    assert lib.emd_hanning_window_f64(64, odd4, null, null) == -3 and b"aligned" in err()
    # overlap: outputs and the workspace against everything; two inputs may share bytes (a == b: test_register_gpu)
    for args in ((a, b, 1, 64, 0, a, d, f), (a, b, 1, 64, 0, b, d, f), (a, b, 1, 64, 0, c, c, f), (a, b, 1, 64, 0, c, b, f),
                 (a, b, 1, 64, 0, c, d, a), (a, b, 1, 64, 0, c, d, c)):
        assert pc(*args, big, null) == -1 and b"overlap" in err()
    assert pc(a, b, 1, 64, 0, c, C.c_void_p((1 << 20) + 64 * 64 * 4 - 8), f, big, null) == -1 and b"overlap" in err()   # the surface on a's last bytes
    assert lib.emd_stack_centres_f64(a, 3, 64, a, null) == -1 and b"overlap" in err()
    assert lib.emd_crop_stack_f32(a, 2, 64, b, 8, 0.0, a, null) == -1 and b"overlap" in err()
    assert lib.emd_crop_stack_f32(a, 2, 64, c, 8, 0.0, c, null) == -1 and b"overlap" in err()
    assert lib.emd_hanning_window_f64(64, a, a, null) == -1 and b"overlap" in err()
    text = open(_lib.PKG_DIR + "/../include/emdenoise.h").read()
    assert "#define EMD_PC_WINDOW 1" in text and "#define EMD_PC_CHAIN 2" in text
    assert (PC_WINDOW, PC_CHAIN, exitwave.MAX_PAIRS) == (1, 2, 64)


def test_python_arguments_are_checked_on_the_shape_before_anything_moves():
    """No GPU here: every one of these must raise before a tensor is created on a device."""
    r = lambda *shape: np.broadcast_to(np.float32(0), shape)
    for shape in ((12, 12), (2, 4, 4), (1, 8192, 8192), (3, 100, 100)):
        with pytest.raises(ValueError, match="power of two"):
            exitwave.phase_correlate(r(*shape), r(*shape))
    with pytest.raises(ValueError, match="square"):
        exitwave.phase_correlate(r(2, 16, 32), r(2, 16, 32))
    with pytest.raises(ValueError, match="same shape"):
        exitwave.phase_correlate(r(2, 16, 16), r(3, 16, 16))
    with pytest.raises(ValueError, match="pairs"):
        exitwave.phase_correlate(r(65, 16, 16), r(65, 16, 16))
    for S in (0, 4, 12, 8192, 16.5):
        with pytest.raises(ValueError, match="power of two|integer"):
            exitwave.hanning_window(S)
    for fn in (exitwave.rel_pos_estimate, lambda v: exitwave.align(v, 8), lambda v: exitwave.reconstruct_series(v, 0.0, 1e-12, 8)):
        with pytest.raises(ValueError, match="images"):
            fn(r(1, 16, 16))
        with pytest.raises(ValueError, match="images"):
            fn(r(67, 16, 16))
        with pytest.raises(ValueError, match="square"):
            fn(r(3, 16, 32))
        with pytest.raises(ValueError, match="square"):
            fn(r(16, 16))
        with pytest.raises(ValueError, match="power of two"):
            fn(r(3, 24, 24))
        with pytest.raises(ValueError, match="real"):
            fn(np.broadcast_to(np.complex128(0), (3, 16, 16)))
    for side in (0, 17, 2.5, -4):
        with pytest.raises(ValueError, match="side"):
            exitwave.align(r(3, 16, 16), side)
        with pytest.raises(ValueError, match="side"):
            exitwave.crop_stack(r(3, 16, 16), np.zeros((3, 2)), side)
    with pytest.raises(ValueError, match="power of two"):
        exitwave.reconstruct_series(r(3, 32, 32), 0.0, 1e-12, 12)
    with pytest.raises(ValueError, match="centres"):
        exitwave.crop_stack(r(3, 16, 16), np.zeros((2, 2)), 4)
    with pytest.raises(ValueError, match="pad_val"):
        exitwave.crop_stack(r(3, 16, 16), np.zeros((3, 2)), 4, pad_val=float("nan"))
    with pytest.raises(ValueError, match="side of the images"):
        exitwave.crop_stack(r(1, 5000, 5000), np.zeros((1, 2)), 4)
    assert "Registration (csrc/register.hip" in exitwave.__doc__
