"""CPU tests of the 2-D FFT of any side (emdenoise.spectral, csrc/fft_any.hip): the line length against its
restatement, argument validation at the C and the Python level, the restatement of tests/spectral_ref.py against the long-double DFT
and against numpy.fft, and the yardsticks that the GPU tests' bars are copies of.  Nothing here touches a GPU."""
import ctypes as C

import numpy as np
import pytest

from emdenoise import _lib, spectral
from tests import spectral_ref as R
from tests import test_spectral_gpu as G

LAM, PX = G.LAM, G.PX


def test_line_length():
    lib = _lib.load()
    for n in range(0, 4101):
        want = R.line_length(n)
        assert lib.emd_fft_any_line(n) == want == spectral.line_length(n), n
    for n, want in ((1, 0), (2, 8), (3, 8), (5, 16), (12, 32), (1025, 4096), (2047, 4096), (2048, 2048), (2049, 0), (4096, 4096), (4097, 0),
                    (8, 8), (4, 8), (-8, 0)):
        assert lib.emd_fft_any_line(n) == want, n
    for n in range(2, 2049):
        M = R.line_length(n)
        assert M & (M - 1) == 0 and 8 <= M <= 4096 and (M == n or M >= 2 * n - 1) and (M == n or M == 8 or M // 2 < 2 * n - 1), n
    with pytest.raises(ValueError, match="integer"):
        spectral.line_length(8.0)


def test_c_argument_validation():
    lib = _lib.load()
    a, b, c, f = (C.c_void_p(v) for v in (1 << 20, 2 << 20, 3 << 20, 1 << 30))
    null = C.c_void_p(0)
    big = 1 << 28
    err = lib.emd_last_error
    cfft = lambda x, B, H, W, out, ws, n, real=0, inv=0: lib.emd_cfft2_any_f64(x, real, B, H, W, inv, out, ws, n, null)
    rfft = lambda x, B, H, W, out, ws, n: lib.emd_rfft2_any_f64(x, B, H, W, out, ws, n, null)
    prop = lambda x, B, H, W, d, out, ws, n, px=PX: lib.emd_propagate_any_f64(x, 0, B, H, W, d, LAM, px, 0.0, out, ws, n, null)
    # sizes: the tables of each distinct side, then the transposed intermediate (and, for propagate, a second one)
    r256 = lambda n: (n + 255) & ~255
    tab = lambda n: r256(R.line_length(n) * 16) + (0 if R.is_plain(n) else r256(n * 16) + r256(R.line_length(n) * 16))
    assert lib.emd_cfft2_any_workspace_bytes(2, 64, 64) == tab(64) + r256(2 * 64 * 64 * 16)
    assert lib.emd_cfft2_any_workspace_bytes(2, 12, 12) == tab(12) + r256(2 * 12 * 12 * 16)              # a square: one set
    assert lib.emd_cfft2_any_workspace_bytes(3, 17, 64) == tab(64) + tab(17) + r256(3 * 17 * 64 * 16)
    assert lib.emd_rfft2_any_workspace_bytes(3, 17, 20) == tab(20) + tab(17) + r256(3 * 17 * 11 * 16)
    assert lib.emd_propagate_any_workspace_bytes(3, 17, 20) == tab(20) + tab(17) + 2 * r256(3 * 17 * 20 * 16)
    for fn in (lib.emd_cfft2_any_workspace_bytes, lib.emd_rfft2_any_workspace_bytes, lib.emd_propagate_any_workspace_bytes):
        assert fn(0, 64, 64) == 0 and fn(-1, 64, 64) == 0 and fn(65536, 8, 8) == 0 and fn(65535, 2, 2) > 0
    # bad sides, on either axis
    for n in (0, 1, -3, 2049, 2050, 3000, 4095, 4097, 8192):
        for H, W in ((n, 16), (16, n), (n, n)):
            assert lib.emd_cfft2_any_workspace_bytes(1, H, W) == 0 and lib.emd_rfft2_any_workspace_bytes(1, H, W) == 0
            assert lib.emd_propagate_any_workspace_bytes(1, H, W) == 0
            assert cfft(a, 1, H, W, b, f, big) == -1 and b"shape" in err() and str(n).encode() in err()
            assert rfft(a, 1, H, W, b, f, big) == -1 and b"shape" in err()
            assert prop(a, 1, H, W, c, b, f, big) == -1 and b"shape" in err()
    assert b"each side 2..2048, or a power of two up to 4096" in err()
    for B in (-1, 65536):
        assert cfft(a, B, 16, 16, b, f, big) == -1 and b"shape" in err()
    assert prop(a, 1, 16, 16, c, b, f, big, px=0.0) == -1 and b"px" in err()
    assert prop(a, 1, 16, 16, c, b, f, big, px=float("nan")) == -1 and b"px" in err()
    # null pointers
    for args in ((null, 1, 12, 20, b, f), (a, 1, 12, 20, null, f), (a, 1, 12, 20, b, null)):
        assert cfft(*args, big) == -1 and b"null" in err()
        assert rfft(*args, big) == -1 and b"null" in err()
    for args in ((null, 1, 12, 20, c, b, f), (a, 1, 12, 20, null, b, f), (a, 1, 12, 20, c, null, f), (a, 1, 12, 20, c, b, null)):
        assert prop(*args, big) == -1 and b"null" in err()
    # a workspace one byte short
    for H, W in ((12, 20), (64, 64), (2047, 8)):
        assert cfft(a, 1, H, W, b, f, lib.emd_cfft2_any_workspace_bytes(1, H, W) - 1) == -1 and b"workspace" in err()
        assert rfft(a, 1, H, W, b, f, lib.emd_rfft2_any_workspace_bytes(1, H, W) - 1) == -1 and b"workspace" in err()
        assert prop(a, 1, H, W, c, b, f, lib.emd_propagate_any_workspace_bytes(1, H, W) - 1) == -1 and b"workspace" in err()
    # alignment: 16 bytes for complex arrays and the workspace, 4 for float32 images, 8 for the defocuses
    odd16, odd4 = C.c_void_p((1 << 20) + 8), C.c_void_p((1 << 20) + 2)
    assert cfft(odd16, 1, 12, 20, b, f, big) == -3 and b"aligned" in err()
    assert cfft(odd4, 1, 12, 20, b, f, big, real=1) == -3 and b"aligned" in err()
    assert cfft(a, 1, 12, 20, C.c_void_p((2 << 20) + 8), f, big) == -3 and b"aligned" in err()
    assert rfft(odd4, 1, 12, 20, b, f, big) == -3 and b"aligned" in err()
    assert prop(a, 1, 12, 20, C.c_void_p((3 << 20) + 4), b, f, big) == -3 and b"aligned" in err()
    # overlap: an output or the workspace with anything
    assert cfft(a, 1, 12, 20, a, f, big) == -1 and b"overlap" in err()
    assert cfft(a, 1, 12, 20, b, a, big) == -1 and b"overlap" in err()
    assert cfft(a, 1, 12, 20, b, b, big) == -1 and b"overlap" in err()
    assert cfft(a, 1, 12, 20, C.c_void_p((1 << 20) + 12 * 20 * 16 - 16), f, big) == -1 and b"overlap" in err()    # the last element
    assert rfft(a, 1, 12, 20, a, f, big) == -1 and b"overlap" in err()
    assert rfft(a, 1, 12, 20, b, b, big) == -1 and b"overlap" in err()
    assert prop(a, 1, 12, 20, c, a, f, big) == -1 and b"overlap" in err()
    assert prop(a, 1, 12, 20, c, c, f, big) == -1 and b"overlap" in err()
    assert prop(a, 1, 12, 20, c, b, c, big) == -1 and b"overlap" in err()
    assert prop(a, 1, 12, 20, c, b, b, big) == -1 and b"overlap" in err()
    # (every call above is refused before anything is launched: the pointers are made up)
    # empty batches are no-ops
    assert cfft(a, 0, 12, 20, b, f, 0) == 0 and rfft(a, 0, 12, 20, b, f, 0) == 0 and prop(a, 0, 12, 20, c, b, f, 0) == 0
    assert cfft(null, 0, 12, 20, null, null, 0) == 0


def test_python_arguments_are_checked_before_anything_moves():
    """No GPU here: every one of these must raise before a tensor is created on a device."""
    z = lambda *shape: np.broadcast_to(np.complex128(0), shape)
    r = lambda *shape: np.broadcast_to(np.float32(0), shape)
    fns = (spectral.fft2, spectral.ifft2, spectral.rfft2, lambda v: spectral.propagate(v, 0.0, LAM))
    for fn in fns:
        arg = r if fn is spectral.rfft2 else z
        for shape in ((1, 12), (12, 1), (2, 2049, 16), (16, 3000), (8192, 8192), (1, 4097, 4097), (0, 16)):
            with pytest.raises(ValueError, match=r"each side 2\.\.2048, or a power of two up to 4096"):
                fn(arg(*shape))
        for shape in ((16,), (2, 2, 16, 16), ()):
            with pytest.raises(ValueError, match="dimensions"):
                fn(arg(*shape))
        with pytest.raises(ValueError, match="images"):
            fn(arg(0, 16, 16))
        with pytest.raises(ValueError, match="numeric"):
            fn(np.broadcast_to(np.bool_(0), (16, 16)))
    with pytest.raises(ValueError, match="real"):
        spectral.rfft2(z(12, 20))
    for kw in ({"wavelength": 0.0}, {"wavelength": LAM, "px": 0.0}, {"wavelength": float("nan")}, {"wavelength": LAM, "px": -1.0}):
        with pytest.raises(ValueError, match="positive"):
            spectral.propagate(z(12, 20), 0.0, **kw)
    with pytest.raises(ValueError, match="cs"):
        spectral.propagate(z(12, 20), 0.0, LAM, cs=float("inf"))
    assert spectral.RULE == "each side 2..2048, or a power of two up to 4096"


def test_restatement_pieces():
    for n in (2, 3, 5, 12, 100, 255, 1228, 2047):
        w = R.chirp(n)
        k = np.arange(n, dtype=np.int64)
        ang = -(R.PI_LD) * ((k * k) % (2 * n)).astype(R.LD) / R.LD(n)
        assert np.abs(w - (np.cos(ang) + 1j * np.sin(ang)).astype(np.complex128)).max() <= 2.0 ** -50, n   # the angle is at most pi / 2 with two roundings, then the function's
        assert w[0] == 1.0
        M = R.line_length(n)
        b = np.fft.ifft(R.filter_spectrum(n))
        assert np.abs(b[:n] - np.conj(w)).max() < 1e-14 and np.abs(b[M - n + 1:] - np.conj(w[1:][::-1])).max() < 1e-14
        assert np.abs(b[n:M - n + 1]).max(initial=0.0) < 1e-14
    # the 1-D line, every kind of length, against numpy and against its own inverse
    rng = np.random.default_rng(5)
    for n in (2, 3, 4, 5, 7, 8, 12, 17, 64, 100, 255, 257, 1000, 1228, 2047, 2048, 4096):
        x = rng.standard_normal((3, n)) + 1j * rng.standard_normal((3, n))
        assert R.rel_l2(R.line_dft(x), np.fft.fft(x)) < 2e-15, n
        assert R.rel_l2(R.line_idft(R.line_dft(x)), x) < 3e-15, n
    # fftfreq's indices and the transfer function: even and odd sides, |Hf| = 1, exactly 1 at q = 0, the square case of exitwave_ref
    from tests import exitwave_ref as ER

    for n in (2, 3, 8, 17, 20):
        assert np.array_equal(R.fftfreq_index(n), np.rint(np.fft.fftfreq(n) * n)), n
    Hf = R.transfer_function(17, 20, LAM, 4e-8, PX, G.CS)
    assert Hf[0, 0] == 1.0 and np.allclose(np.abs(Hf), 1.0, rtol=0, atol=1e-15)
    assert np.array_equal(R.transfer_function(16, 16, LAM, 4e-8, PX, G.CS), ER.transfer_function(16, LAM, 4e-8, PX, G.CS))
    assert np.abs(R.transfer_function(17, 20, LAM, 4e-8, PX, G.CS, R.LD) - Hf).max() < 1e-13


def test_yardsticks_are_the_constants_of_the_gpu_tests(capsys):
    """The restatement against numpy.fft.fft2 at every case of the GPU test (the field yardstick), both against the long-double DFT at
    sides <= 257, the restatement's element errors on the impulse, and the propagation's phase yardstick: recomputed here, printed,
    and held against the constants copied into tests/test_spectral_gpu.py (`python -m tests.test_spectral_gpu` prints them too)."""
    y = G.yardsticks()
    with capsys.disabled():
        print()
        for line in y["log"]:
            print("  " + line)
    held = lambda const, value: value <= const <= 1.02 * value      # the copy is the value rounded up in its fourth digit
    assert held(G.YARD, y["field"]), (G.YARD, y["field"])
    assert held(G.PROP_YARD, y["prop"]), (G.PROP_YARD, y["prop"])
    assert set(G.IMPULSE_ERR) == set(y["impulse"]) == set(G.IMPULSE_CASES)
    for c in G.IMPULSE_CASES:
        assert held(G.IMPULSE_ERR[c], y["impulse"][c]), (c, G.IMPULSE_ERR[c], y["impulse"][c])
    for (H, W), (yard, rest_ld, numpy_ld) in y["small"].items():
        assert rest_ld <= yard and numpy_ld <= yard, ((H, W), yard, rest_ld, numpy_ld)
    # what the bars are far from: a wrapped chirp index, a wrong conjugate and a dropped Cs term are O(1)
    z = R.noise(1, 12, 20)[0]
    bad = np.fft.fft2(np.conj(z))
    assert R.rel_l2(bad, np.fft.fft2(z)) > 0.5
    p0, p1 = R.propagate(z, 1.2e-7, LAM, PX, 0.0), R.propagate(z, 1.2e-7, LAM, PX, G.CS)
    assert R.rel_l2(p1, p0) > 1e-2
    assert 4.0 * G.YARD < 1e-13 and 4.0 * G.PROP_YARD < 1e-12
