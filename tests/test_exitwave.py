"""CPU tests of the focal-series reconstruction (emdenoise.exitwave, csrc/exitwave.hip): the series helpers against
the reference's expression, argument validation at the C and the Python level, the restatement of tests/exitwave_ref.py against
itself (its two FFT back ends and its two orders), and the conditions the GPU tests' bars rest on.  Nothing here touches a GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest

from emdenoise import _lib, exitwave
from tests import exitwave_ref as R
from tests.test_exitwave_gpu import CS, CS_RECON_CASES, KAPPA_MAX, RATIO_MIN, SWEEPS, YARD

LAM, PX = R.WAVELENGTH, R.PX
SMALL_CASES = [(1, 8, 0, 1), (2, 8, 0, 2), (3, 16, 0, 5), (5, 32, 0, 5), (2, 8, 1, 2), (3, 16, 3, 2)]


def test_focal_ramp_is_the_references_expression():
    for kind, alt, inc, n, mid in itertools.product(("linear", "quadratic", "cubic"), (True, False), (True, False), (1, 5, 8), (None, 2)):
        got = exitwave.focal_ramp(n, kind, middle=mid, alternating=alt, increasing=inc)
        assert got.dtype == np.float64 and np.array_equal(got, R.focal_ramp(n, kind, mid, alt, inc)), (kind, alt, inc, n, mid)
    assert exitwave.focal_ramp(5, "cubic").tolist() == [8.0, 1.0, 0.0, 1.0, 8.0]          # sign(x) x^3, as the reference writes it
    assert exitwave.focal_ramp(5, "quadratic").tolist() == [-4.0, -1.0, 0.0, 1.0, 4.0]
    assert exitwave.focal_ramp(4, "quadratic", alternating=False, increasing=False).tolist() == [-0.0, -1.0, -4.0, -9.0]
    with pytest.raises(ValueError, match="series_type"):
        exitwave.focal_ramp(5, "quartic")
    with pytest.raises(ValueError, match="positive integer"):
        exitwave.focal_ramp(0)


def test_c_argument_validation():
    lib = _lib.load()
    a, b, c, d, e, f = (C.c_void_p(v) for v in (1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20, 1 << 30))
    null = C.c_void_p(0)
    big = 1 << 28
    err = lib.emd_last_error
    # sizes
    assert lib.emd_cfft2_workspace_bytes(2, 64) == 64 * 16 + 2 * 64 * 64 * 16
    assert lib.emd_propagate_workspace_bytes(2, 32, 1) > lib.emd_propagate_workspace_bytes(2, 32, 0) > 0
    fused = lib.emd_exitwave_workspace_bytes(3, 32, 0)
    _lib.knob(exitwave.COMPOSED_KNOB, 1)                                    # the development knob: the composed path at pad 0
    try:
        composed = lib.emd_exitwave_workspace_bytes(3, 32, 0)
        assert lib.emd_exitwave_reconstruct_f64(a, 3, 32, 0, b, LAM, PX, 0.0, 1, 0, c, d, e, f, composed - 1, null) == -1
        assert b"workspace" in err()
    finally:
        _lib.knob(exitwave.COMPOSED_KNOB, 0)
    assert composed > fused > 0 and lib.emd_exitwave_workspace_bytes(3, 32, 0) == fused
    assert lib.emd_exitwave_workspace_bytes(3, 16, 1) > 0
    assert lib.emd_cfft2_workspace_bytes(0, 64) == 0 and lib.emd_propagate_workspace_bytes(0, 64, 0) == 0
    for S in (0, 4, 7, 12, 100, 1000, 2047, 8192):
        assert lib.emd_cfft2_workspace_bytes(1, S) == 0 and lib.emd_propagate_workspace_bytes(1, S, 0) == 0
        assert lib.emd_exitwave_workspace_bytes(1, S, 0) == 0
        assert lib.emd_cfft2_f64(a, 1, S, 0, b, f, big, null) == -1 and b"shape" in err()
        assert lib.emd_transfer_function_f64(S, 1, a, LAM, PX, 0.0, b, null) == -1 and b"shape" in err()
        assert lib.emd_propagate_f64(a, 0, 1, S, 0, b, LAM, PX, 0.0, c, f, big, null) == -1 and b"shape" in err()
        assert lib.emd_exitwave_reconstruct_f64(a, 1, S, 0, b, LAM, PX, 0.0, 1, 0, c, null, null, f, big, null) == -1 and b"shape" in err()
    for s, pad in ((8, 2), (12, 1), (4096, 1), (2, 1), (16, -1)):             # a padded side that is no power of two in 8..4096
        assert lib.emd_propagate_workspace_bytes(1, s, pad) == 0 and lib.emd_exitwave_workspace_bytes(1, s, pad, 0) == 0
        assert lib.emd_propagate_f64(a, 0, 1, s, pad, b, LAM, PX, 0.0, c, f, big, null) == -1 and b"shape" in err()
        assert lib.emd_exitwave_reconstruct_f64(a, 1, s, pad, b, LAM, PX, 0.0, 1, 0, c, null, null, f, big, null) == -1 and b"shape" in err()
    assert lib.emd_propagate_workspace_bytes(1, 4, 1) > 0 and lib.emd_propagate_workspace_bytes(1, 2, 3) > 0
    for N in (0, -1, 65):
        assert lib.emd_exitwave_workspace_bytes(N, 32, 0) == 0
        assert lib.emd_exitwave_reconstruct_f64(a, N, 32, 0, b, LAM, PX, 0.0, 1, 0, c, null, null, f, big, null) == -1 and b"shape" in err()
    assert lib.emd_exitwave_reconstruct_f64(a, 2, 32, 0, b, LAM, PX, 0.0, 0, 0, c, null, null, f, big, null) == -1 and b"iterations" in err()
    assert lib.emd_exitwave_reconstruct_f64(a, 2, 32, 0, b, LAM, 0.0, 0.0, 1, 0, c, null, null, f, big, null) == -1 and b"px" in err()
    # null pointers
    assert lib.emd_cfft2_f64(null, 1, 64, 0, b, f, big, null) == -1 and b"null" in err()
    assert lib.emd_cfft2_f64(a, 1, 64, 0, null, f, big, null) == -1 and b"null" in err()
    assert lib.emd_cfft2_f64(a, 1, 64, 0, b, null, big, null) == -1 and b"null" in err()
    assert lib.emd_transfer_function_f64(64, 1, null, LAM, PX, 0.0, b, null) == -1 and b"null" in err()
    assert lib.emd_transfer_function_f64(64, 1, a, LAM, PX, 0.0, null, null) == -1 and b"null" in err()
    for args in ((null, 0, 1, 64, 0, b), (a, 0, 1, 64, 0, null)):
        assert lib.emd_propagate_f64(*args, LAM, PX, 0.0, c, f, big, null) == -1 and b"null" in err()
    assert lib.emd_propagate_f64(a, 0, 1, 64, 0, b, LAM, PX, 0.0, null, f, big, null) == -1 and b"null" in err()
    assert lib.emd_propagate_f64(a, 0, 1, 64, 0, b, LAM, PX, 0.0, c, null, big, null) == -1 and b"null" in err()
    for args in ((null, 2, 32, 0, b, LAM, PX, 0.0, 1, 0, c, d, e, f), (a, 2, 32, 0, null, LAM, PX, 0.0, 1, 0, c, d, e, f),
                 (a, 2, 32, 0, b, LAM, PX, 0.0, 1, 0, null, d, e, f), (a, 2, 32, 0, b, LAM, PX, 0.0, 1, 0, c, d, e, null)):
        assert lib.emd_exitwave_reconstruct_f64(*args, big, null) == -1 and b"null" in err()
    # a short workspace
    assert lib.emd_cfft2_f64(a, 1, 64, 0, b, f, lib.emd_cfft2_workspace_bytes(1, 64) - 1, null) == -1 and b"workspace" in err()
    assert lib.emd_propagate_f64(a, 0, 1, 64, 0, b, LAM, PX, 0.0, c, f, lib.emd_propagate_workspace_bytes(1, 64, 0) - 1, null) == -1
    assert b"workspace" in err()
    for pad in (0, 1):
        short = lib.emd_exitwave_workspace_bytes(2, 32, pad) - 1
        assert lib.emd_exitwave_reconstruct_f64(a, 2, 32, pad, b, LAM, PX, 0.0, 1, 0, c, d, e, f, short, null) == -1
        assert b"workspace" in err()
    # alignment and overlap
    assert lib.emd_cfft2_f64(C.c_void_p((1 << 20) + 8), 1, 64, 0, b, f, big, null) == -3 and b"aligned" in err()
    odd = C.c_void_p((2 << 20) + 4)                                         # arrays of doubles: 8-byte alignment is checked too
    assert lib.emd_transfer_function_f64(64, 1, odd, LAM, PX, 0.0, c, null) == -3 and b"aligned" in err()
    assert lib.emd_propagate_f64(a, 0, 1, 64, 0, odd, LAM, PX, 0.0, c, f, big, null) == -3 and b"aligned" in err()
    assert lib.emd_exitwave_reconstruct_f64(a, 2, 32, 0, odd, LAM, PX, 0.0, 1, 0, c, d, e, f, big, null) == -3 and b"aligned" in err()
    assert lib.emd_exitwave_reconstruct_f64(a, 2, 32, 0, b, LAM, PX, 0.0, 1, 0, c, d, odd, f, big, null) == -3 and b"aligned" in err()
    assert lib.emd_cfft2_f64(a, 1, 64, 0, a, f, big, null) == -1 and b"overlap" in err()
    assert lib.emd_cfft2_f64(a, 1, 64, 0, b, a, big, null) == -1 and b"overlap" in err()
    assert lib.emd_transfer_function_f64(64, 1, a, LAM, PX, 0.0, a, null) == -1 and b"overlap" in err()
    assert lib.emd_propagate_f64(a, 0, 1, 64, 0, b, LAM, PX, 0.0, a, f, big, null) == -1 and b"overlap" in err()
    assert lib.emd_propagate_f64(a, 0, 1, 64, 0, c, LAM, PX, 0.0, c, f, big, null) == -1 and b"overlap" in err()
    assert lib.emd_propagate_f64(a, 0, 1, 64, 0, b, LAM, PX, 0.0, c, c, big, null) == -1 and b"overlap" in err()
    for args in ((a, 2, 32, 0, b, LAM, PX, 0.0, 1, 0, a, d, e, f), (a, 2, 32, 0, b, LAM, PX, 0.0, 1, 0, c, c, e, f),
                 (a, 2, 32, 0, b, LAM, PX, 0.0, 1, 0, c, d, d, f), (a, 2, 32, 0, b, LAM, PX, 0.0, 1, 0, c, d, b, f),
                 (a, 2, 32, 0, b, LAM, PX, 0.0, 1, 0, c, d, e, d)):
        assert lib.emd_exitwave_reconstruct_f64(*args, big, null) == -1 and b"overlap" in err()
    # empty batches are no-ops
    assert lib.emd_cfft2_f64(a, 0, 64, 0, b, f, 0, null) == 0 and lib.emd_propagate_f64(a, 0, 0, 64, 0, b, LAM, PX, 0.0, c, f, 0, null) == 0
    assert lib.emd_transfer_function_f64(64, 0, a, LAM, PX, 0.0, b, null) == 0
    text = open(_lib.PKG_DIR + "/../include/emdenoise.h").read()
    dev = open(_lib.PKG_DIR + "/../include/emdenoise_dev.h").read()
    assert "#define EMD_EXITWAVE_FROM_INTENSITY 1" in text and "COMPOSED" not in text and exitwave.COMPOSED_KNOB in dev
    assert exitwave.FROM_INTENSITY == 1 and lib.emd_debug_knob(b"exitwave_composed", 0) == 0


def test_python_arguments_are_checked_on_the_shape_before_anything_moves():
    """No GPU here: every one of these must raise before a tensor is created on a device."""
    z = lambda *shape: np.broadcast_to(np.complex128(0), shape)
    r = lambda *shape: np.broadcast_to(np.float32(0), shape)
    for fn in (exitwave.fft2, exitwave.ifft2, lambda v: exitwave.propagate(v, 0.0, LAM)):
        for shape in ((12, 12), (2, 4, 4), (1, 8192, 8192), (3, 100, 100)):
            with pytest.raises(ValueError, match="power of two"):
                fn(z(*shape))
        with pytest.raises(ValueError, match="square"):
            fn(z(2, 16, 32))
        with pytest.raises(ValueError, match="dimensions"):
            fn(z(2, 2, 16, 16))
    for s, pad in ((8, 2), (12, 1), (4096, 1), (16, -1), (16, 0.5)):
        with pytest.raises(ValueError, match="power of two|pad_periods"):
            exitwave.propagate(z(1, s, s), 0.0, LAM, pad_periods=pad)
        with pytest.raises(ValueError, match="power of two|pad_periods"):
            exitwave.reconstruct(r(2, s, s), [0.0, 1.0], LAM, pad_periods=pad)
    for S in (0, 4, 12, 8192, 16.5):
        with pytest.raises(ValueError, match="power of two|integer"):
            exitwave.transfer_function(S, LAM, 1e-8)
    with pytest.raises(ValueError, match="defocuses"):
        exitwave.transfer_function(16, LAM, [])
    with pytest.raises(ValueError, match="images"):
        exitwave.reconstruct(r(0, 16, 16), [], LAM)
    with pytest.raises(ValueError, match="images"):
        exitwave.reconstruct(r(65, 16, 16), np.zeros(65), LAM)
    with pytest.raises(ValueError, match="square"):
        exitwave.reconstruct(r(2, 16, 32), [0.0, 1.0], LAM)
    with pytest.raises(ValueError, match="square"):
        exitwave.reconstruct(r(16, 16), [0.0], LAM)
    with pytest.raises(ValueError, match="real"):
        exitwave.reconstruct(z(2, 16, 16), [0.0, 1.0], LAM)
    with pytest.raises(ValueError, match="iterations"):
        exitwave.reconstruct(r(2, 16, 16), [0.0, 1.0], LAM, iterations=0)
    for kw in ({"wavelength": 0.0}, {"wavelength": LAM, "px": 0.0}, {"wavelength": float("nan")}):
        with pytest.raises(ValueError, match="positive"):
            exitwave.reconstruct(r(2, 16, 16), [0.0, 1.0], **kw)
    with pytest.raises(ValueError, match="ramp"):
        exitwave.defocus_sweep(r(3, 16, 16), LAM, [1e-8], [0.0, 1.0])
    with pytest.raises(ValueError, match="increment"):
        exitwave.defocus_sweep(r(2, 16, 16), LAM, [], [0.0, 1.0])
    for kw in ({"per_image": True}, {"return_stack": True}, {"pixels": 2}):
        with pytest.raises(TypeError, match="unexpected keyword"):
            exitwave.defocus_sweep(r(2, 16, 16), LAM, [1e-8], [0.0, 1.0], **kw)
    with pytest.raises(TypeError, match="unexpected keyword"):
        exitwave.reconstruction_loss(r(2, 16, 16), [0.0, 1.0], LAM, return_stack=True)


def test_restatement_transfer_function():
    for S in (8, 16):
        H = R.transfer_function(S, LAM, 4e-8, PX)
        q = np.fft.fftfreq(S, PX)
        want = np.exp(1j * np.pi * LAM * 4e-8 * (q[:, None] ** 2 + q[None, :] ** 2))
        print(f"S = {S}: restated H against exp(i pi lam df q^2) on numpy.fft.fftfreq: {np.abs(H - want).max():.2e}")
        assert np.abs(H - want).max() <= 1e-14 and H[0, 0] == 1.0
        assert np.array_equal(R.transfer_function(S, LAM, -4e-8, PX), np.conj(H))
        assert np.allclose(np.abs(R.transfer_function(S, LAM, 4e-8, PX, 1e-3)), 1.0, rtol=0, atol=1e-15)
    padded = R.propagate(np.ones((8, 8)), 0.0, LAM, PX, 0.0, 1)
    assert padded.shape == (8, 8) and np.allclose(padded, 1.0, rtol=0, atol=1e-14)


def test_the_restatements_back_ends_and_orders_agree_within_the_yardstick():
    assert YARD > 0
    for case in SMALL_CASES:
        N, s, pad, iters = case
        images, df = R.series(N, s)
        a = R.reconstruct(images, df, LAM, PX, 0.0, iters, pad)
        b = R.reconstruct(images, df, LAM, PX, 0.0, iters, pad, fft=R.Radix2FFT)
        eE, eS = R.rel_l2(b["E"], a["E"]), R.rel_l2(b["stack"], a["stack"])
        print(f"{case}: numpy.fft against radix-2: E {eE:.3e}, stack {eS:.3e}; yardstick {YARD:.3e}; min |b| / mean |b| {a['ratio']:.3f}")
        assert max(eE, eS) <= YARD and a["ratio"] >= RATIO_MIN
        if pad == 0:
            f = R.reconstruct(images, df, LAM, PX, 0.0, iters, 0, order="freq")
            eE, eS = R.rel_l2(f["E"], a["E"]), R.rel_l2(f["stack"], a["stack"])
            print(f"{case}: frequency-domain order against real-space order: E {eE:.3e}, stack {eS:.3e}; bar, the yardstick, {YARD:.3e}")
            assert max(eE, eS) <= YARD


def test_with_spherical_aberration_the_back_propagation_is_not_the_conjugate():
    """The condition of the GPU tests at Cs != 0: H(-df) is far from conj H(df), and the restatement stays well conditioned."""
    for S in (16, 32):
        Hm, Hc = R.transfer_function(S, LAM, -4e-8, PX, CS), np.conj(R.transfer_function(S, LAM, 4e-8, PX, CS))
        print(f"S = {S}, Cs = {CS}: H(-df) against conj H(df), rel L2 {R.rel_l2(Hm, Hc):.3f}")
        assert R.rel_l2(Hm, Hc) > 0.5
        assert np.array_equal(np.conj(R.transfer_function(S, LAM, 4e-8, PX, CS)), R.transfer_function(S, LAM, -4e-8, PX, -CS))
    for N, s, pad, iters in CS_RECON_CASES:
        images, df = R.series(N, s)
        r = R.reconstruct(images, df, LAM, PX, CS, iters, pad)
        print(f"{(N, s, pad, iters)}, Cs = {CS}: min |b| / mean |b| {r['ratio']:.3f}")
        assert r["ratio"] >= RATIO_MIN


def test_the_conditions_of_the_loss_bars():
    images, df = R.series(3, 32)
    for pad in (0, 1):
        r = R.reconstruct(images, 1.5 * df, LAM, PX, 0.0, 5, pad)
        print(f"pad {pad}: kappa {r['kappa']}, losses {r['losses']}, min |b| / mean |b| {r['ratio']:.3f}")
        assert r["kappa"].max() <= KAPPA_MAX and r["ratio"] >= RATIO_MIN and (r["losses"] > 1e-8).all()
    for name, x, incs, fi in SWEEPS:                                        # the sweeps of the GPU test: smallest at the true increment
        want = []
        for inc in incs:
            r = R.reconstruct(x(images), inc * (df / 1e-8), LAM, PX, 0.0, 5, from_intensity=fi)
            assert r["kappa"].max() <= KAPPA_MAX and r["ratio"] >= RATIO_MIN
            want.append(r["losses"].max())
        print(f"sweep of {name} images: {want}")
        assert int(np.argmin(want)) == 2 and incs[2] == 1e-8
