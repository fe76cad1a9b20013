"""GPU tests of the 2-D FFT of any side (emdenoise.spectral, csrc/fft_any.hip).

Inputs are seeded white noise, complex128.  No bar comes from the device:
  * fields (fft2, ifft2, rfft2) by relative L2 against numpy.fft: 4 x YARD, YARD the largest distance, over SHAPES, of the float64
    restatement of tests/spectral_ref.py from numpy.fft.fft2 (two independent double-precision algorithms); round trips 2 x that;
  * the impulse element by element against the long-double phase ramp: 4 x the restatement's largest element error on that input;
  * propagate against the restatement: 4 x PROP_YARD, the largest distance, over the propagation cases, of the restatement as written
    from the same restatement with the phase formed in long double; the energy 2 x that.
The constants are copies: tests/test_spectral.py recomputes them on the CPU and holds these against the values (``python -m
tests.test_spectral_gpu`` prints them).  Measured on an MI355X (DESIGN.md 3.29 has the table): fields <= 8.4e-16 (bar 4.77e-15), round
trips <= 8.5e-16, impulse 7.5e-16 / 5.3e-16 / 1.8e-15 (bars 1.74e-15 / 2.72e-15 / 1.06e-14), propagate <= 1.41e-15 (bar 2.78e-14), on a
power-of-two square bit for bit exitwave.propagate, energy within 2.3e-16."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from emdenoise import _lib, exitwave, spectral
from tests import exitwave_ref as ER
from tests import guarded as GD
from tests import spectral_ref as R

pytestmark = pytest.mark.gpu

FACTOR = 4.0
LAM, PX = ER.WAVELENGTH, ER.PX
CS = 1e-3                     # the CS of tests/test_exitwave_gpu.py
# (H, W): M = 8 and the power-of-two lengths below 8; Bluestein against a plain line, in each order; M = 512 against 1024 across the
# 2 n - 1 boundary; the psi-art crop; M = 4096, the whole 64 KiB, on one axis; the largest shape, once
SHAPES = [(2, 3), (3, 5), (4, 8), (12, 20), (17, 64), (64, 17), (100, 96), (255, 257), (1228, 1000), (2047, 8), (8, 2047), (2047, 2047)]
IMPULSE_CASES = [(3, 5), (17, 64), (255, 257)]
PROP_SHAPES = [(12, 20), (100, 96), (1228, 1000)]
YARD = 1.192e-15              # the restatement's largest distance from numpy.fft.fft2 over SHAPES (at 2047 x 2047)
PROP_YARD = 6.960e-15         # the phase in double against the phase in long double, the largest over PROP_SHAPES x (0, CS)
IMPULSE_ERR = {(3, 5): 4.349e-16, (17, 64): 6.790e-16, (255, 257): 2.654e-15}   # the restatement's largest element error


def batch_of(H, W):
    return 2 if H * W <= 1 << 17 else 1


def field_bar():
    return FACTOR * YARD


def prop_bar():
    return FACTOR * PROP_YARD


def ids(c):
    return "x".join(str(v) for v in c)


def dev():
    return torch.device("cuda", 0)


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def bits(t):
    return torch.view_as_real(t) if t.is_complex() else t


def field(H, W):
    """[B,H,W] complex128 white noise of the case.  Cached: do not write into the result."""
    return R.noise(batch_of(H, W), H, W)


def prop_defocuses(B):
    return np.array([1.2e-7, -5e-8, 3e-8])[:B]


@functools.lru_cache(maxsize=None)
def prop_spectra(H, W):
    """The forward half of the restatement's propagation of every wave of the case, shared by its Cs = 0 and Cs = CS halves."""
    return [R.spectrum_along_rows_then_columns(w) for w in field(H, W)]


@functools.lru_cache(maxsize=None)
def prop_ref(H, W, cs, dtype=np.float64):
    return np.stack([R.propagate_from(s, d, LAM, PX, cs, dtype) for s, d in zip(prop_spectra(H, W), prop_defocuses(batch_of(H, W)))])


def impulse(H, W):
    x = np.zeros((H, W), np.complex128)
    x[H - 1, 1] = 1.0
    return x


def yardsticks():
    """Everything the bars are made of, on the CPU: dict(field, prop, impulse {case: err}, small {case: (yard, restatement against the
    long-double DFT, numpy against it)}, log [lines])."""
    log, small, imp = [], {}, {}
    worst = 0.0
    for H, W in SHAPES:
        z = field(H, W)
        f, want = R.fft2(z), np.fft.fft2(z)
        e = R.rel_l2(f, want)
        worst = max(worst, e)
        extra = ""
        if max(H, W) <= 257:
            x = z.real.astype(np.float32)
            extra = f"; ifft2 {R.rel_l2(R.ifft2(z), np.fft.ifft2(z)):.3e}; rfft2 {R.rel_l2(R.rfft2(x), np.fft.rfft2(x.astype(np.float64))):.3e}"
            ld = np.stack([R.dft2_longdouble(v) for v in z])
            small[(H, W)] = (e, R.rel_l2(f, ld), R.rel_l2(want, ld))
            extra += f"; against the long-double DFT: restatement {small[(H, W)][1]:.3e}, numpy {small[(H, W)][2]:.3e}"
        log.append(f"yardstick fft2 {H} x {W}: {e:.3e}" + extra)
    for H, W in IMPULSE_CASES:
        exact = R.impulse_spectrum(H, W, H - 1, 1)
        imp[(H, W)] = float(np.abs(R.fft2(impulse(H, W)).astype(R.CLD) - exact).max())
        log.append(f"impulse {H} x {W}: the restatement's largest element error {imp[(H, W)]:.4e} "
                   f"(numpy's {float(np.abs(np.fft.fft2(impulse(H, W)).astype(R.CLD) - exact).max()):.3e})")
    pworst = 0.0
    for H, W in PROP_SHAPES:
        for cs in (0.0, CS):
            e = R.rel_l2(prop_ref(H, W, cs), prop_ref(H, W, cs, R.LD))
            pworst = max(pworst, e)
            log.append(f"propagate {H} x {W}, Cs = {cs}: the phase in double against the phase in long double {e:.3e}")
    log.append(f"field yardstick {worst:.4e} (bar {FACTOR * worst:.3e}); propagation yardstick {pworst:.4e} (bar {FACTOR * pworst:.3e})")
    return {"field": worst, "prop": pworst, "impulse": imp, "small": small, "log": log}


def check_field(got, want, what, factor=1.0):
    e = R.rel_l2(got, want)
    print(f"{what}: rel L2 {e:.3e}; bar {factor * field_bar():.3e} (yardstick {YARD:.3e})")
    assert e <= factor * field_bar(), what


# ---- 1. bit equality on the old ground ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [8, 64, 512])
def test_power_of_two_squares_are_exitwaves_bits(S):
    z = up(R.noise(2, S, S))
    assert torch.equal(bits(spectral.fft2(z)), bits(exitwave.fft2(z)))
    assert torch.equal(bits(spectral.ifft2(z)), bits(exitwave.ifft2(z)))


@pytest.mark.parametrize("case", [(12, 20), (64, 17)], ids=ids)
def test_an_images_bits_do_not_depend_on_the_batch(case):
    H, W = case
    z = up(R.noise(3, H, W))
    x = z.real.float().contiguous()
    for fn in (spectral.fft2, spectral.ifft2):
        whole = fn(z)
        for b in range(3):
            assert torch.equal(bits(fn(z[b:b + 1].contiguous())[0]), bits(whole[b])), (fn.__name__, b)
    whole = spectral.rfft2(x)
    assert all(torch.equal(bits(spectral.rfft2(x[b])), bits(whole[b])) for b in range(3))


def test_bitwise_reproducible():
    for H, W in ((12, 20), (64, 17), (255, 257)):
        z = up(field(H, W))
        for fn in (spectral.fft2, spectral.ifft2, lambda v: spectral.propagate(v, 3e-8, LAM, px=PX, cs=CS)):
            a, b = fn(z), fn(z)
            assert torch.equal(bits(a), bits(b)) and not torch.isnan(bits(a)).any(), (H, W)


# ---- 2. accuracy -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", SHAPES, ids=ids)
def test_fft2_ifft2_rfft2_against_numpy(case):
    """Measured on an MI355X, the largest over the twelve shapes: fft2 8.24e-16, ifft2 8.38e-16, rfft2 8.17e-16 (all at 1228 x 1000),
    round trip 8.51e-16 (at 2047 x 2047), beside the bars of 4.77e-15 and 9.54e-15."""
    H, W = case
    z = field(H, W)
    B = z.shape[0]
    zd = up(z)
    f, i = spectral.fft2(zd), spectral.ifft2(zd)
    assert f.is_cuda and f.dtype == torch.complex128 and tuple(f.shape) == (B, H, W) and tuple(i.shape) == (B, H, W)
    check_field(f.cpu().numpy(), np.fft.fft2(z), f"fft2 [{B},{H},{W}]")
    check_field(i.cpu().numpy(), np.fft.ifft2(z), f"ifft2 [{B},{H},{W}]")
    check_field(spectral.ifft2(f).cpu().numpy(), z, f"ifft2(fft2(z)) [{B},{H},{W}]", 2.0)
    x = z.real.astype(np.float32)
    r = spectral.rfft2(up(x))
    assert r.dtype == torch.complex128 and tuple(r.shape) == (B, H, W // 2 + 1)
    check_field(r.cpu().numpy(), np.fft.rfft2(x.astype(np.float64)), f"rfft2 [{B},{H},{W}]")


# ---- 3. element-wise, against exact values -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", IMPULSE_CASES, ids=ids)
def test_impulse_gives_the_phase_ramp_at_every_element(case):
    H, W = case
    exact = R.impulse_spectrum(H, W, H - 1, 1)
    got = spectral.fft2(up(impulse(H, W))).cpu().numpy()
    e = float(np.abs(got.astype(R.CLD) - exact).max())
    bar = FACTOR * IMPULSE_ERR[case]
    print(f"impulse at ({H - 1}, 1) of {H} x {W}: largest element error {e:.3e}; bar {bar:.3e}")
    assert e <= bar


# ---- 4. propagate ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cs", [0.0, CS])
@pytest.mark.parametrize("case", PROP_SHAPES, ids=ids)
def test_propagate(case, cs):
    H, W = case
    z = field(H, W)
    B = z.shape[0]
    got = spectral.propagate(up(z), up(prop_defocuses(B)), LAM, px=PX, cs=cs)
    assert got.is_cuda and got.dtype == torch.complex128 and tuple(got.shape) == (B, H, W)
    e = R.rel_l2(got.cpu().numpy(), prop_ref(H, W, cs))
    energy = abs(float((got.abs() ** 2).sum()) / float((np.abs(z) ** 2).sum()) - 1.0)
    print(f"propagate [{B},{H},{W}], Cs = {cs}: rel L2 {e:.3e}, bar {prop_bar():.3e} (yardstick {PROP_YARD:.3e}); "
          f"energy off by {energy:.3e}, bar {2.0 * prop_bar():.3e}")
    assert e <= prop_bar()
    assert energy <= 2.0 * prop_bar()


@pytest.mark.parametrize("S", [64, 512])
def test_propagate_agrees_with_exitwave_on_a_power_of_two_square(S):
    z = up(R.noise(2, S, S))
    d = up(prop_defocuses(2))
    for cs in (0.0, CS):
        a, b = spectral.propagate(z, d, LAM, px=PX, cs=cs), exitwave.propagate(z, d, LAM, px=PX, cs=cs, pad_periods=0)
        e = R.rel_l2(a.cpu().numpy(), b.cpu().numpy())
        print(f"propagate {S} x {S}, Cs = {cs}, against exitwave.propagate: rel L2 {e:.3e}; bar {prop_bar():.3e}")
        assert e <= prop_bar()


def test_propagate_uses_each_images_own_defocus():
    for H, W in ((12, 20), (100, 96)):
        z = up(R.noise(3, H, W))
        d = up(prop_defocuses(3))
        whole = spectral.propagate(z, d, LAM, px=PX, cs=CS)
        for b in range(3):
            alone = spectral.propagate(z[b], d[b:b + 1], LAM, px=PX, cs=CS)
            assert torch.equal(bits(alone), bits(whole[b])), (H, W, b)
        assert not torch.equal(bits(whole[0]), bits(spectral.propagate(z[0], d[1:2], LAM, px=PX, cs=CS)))
        x = z.real.float().contiguous()                    # a float32 image is its real part
        assert torch.equal(bits(spectral.propagate(x, d, LAM, px=PX)), bits(spectral.propagate(x.to(torch.complex128), d, LAM, px=PX)))


# ---- 5. memory -------------------------------------------------------------------------------------------------------------------

def guarded_complex(B, H, W, name):
    view, g = GD.guarded(B * H * W * 2, torch.float64, dev(), name=name)
    return view, g


@pytest.mark.parametrize("case", [(17, 64), (255, 257)], ids=ids)
def test_outputs_and_workspace_stay_inside_their_advertised_sizes(case):
    """A NaN-filled workspace of exactly the advertised size, guard bands around it and around every output: the outputs are written
    completely, hold no NaN (whatever a call reads of its workspace, it has written itself), and the guards are intact."""
    H, W = case
    B, K = 2, W // 2 + 1
    lib, st = _lib.load(), _lib.stream_ptr()
    z = up(R.noise(B, H, W))
    x = z.real.float().contiguous()
    d = up(prop_defocuses(B))
    p = lambda t: C.c_void_p(t.data_ptr())

    def run(what, nbytes, numel, call, want):
        assert nbytes > 0 and nbytes % 8 == 0, what
        ws, gws = GD.guarded(nbytes // 8, torch.float64, dev(), name=f"{what}: workspace of {nbytes} bytes")
        out, gout = GD.guarded(numel * 2, torch.float64, dev(), name=f"{what}: output")
        _lib.check(call(p(out), p(ws), nbytes), what)
        torch.cuda.synchronize()
        gws()
        gout()
        GD.assert_written(out, what)
        assert not torch.isnan(out).any(), what
        assert torch.equal(out.view(-1), bits(want).reshape(-1)), what

    for inverse in (0, 1):
        run(f"cfft2_any {H} x {W} inverse {inverse}", lib.emd_cfft2_any_workspace_bytes(B, H, W), B * H * W,
            lambda o, w, n: lib.emd_cfft2_any_f64(p(z), 0, B, H, W, inverse, o, w, n, st), spectral.ifft2(z) if inverse else spectral.fft2(z))
    run(f"rfft2_any {H} x {W}", lib.emd_rfft2_any_workspace_bytes(B, H, W), B * H * K,
        lambda o, w, n: lib.emd_rfft2_any_f64(p(x), B, H, W, o, w, n, st), spectral.rfft2(x))
    run(f"propagate_any {H} x {W}", lib.emd_propagate_any_workspace_bytes(B, H, W), B * H * W,
        lambda o, w, n: lib.emd_propagate_any_f64(p(z), 0, B, H, W, p(d), LAM, PX, CS, o, w, n, st), spectral.propagate(z, d, LAM, px=PX, cs=CS))


# ---- 6. capture, conventions -----------------------------------------------------------------------------------------------------

def test_captured_in_one_graph_and_replayed_on_new_contents_and_new_defocuses():
    H, W = 100, 96
    z0, z1 = up(R.noise(2, H, W, seed=1)), up(R.noise(2, H, W, seed=2))
    d0, d1 = up(prop_defocuses(2)), up(prop_defocuses(2)[::-1].copy() * 1.25)

    def run(z, d):
        return bits(spectral.fft2(z)), bits(spectral.propagate(z, d, LAM, px=PX, cs=CS))

    want0, want1 = run(z0, d0), run(z1, d1)                                # eager
    sz, sd = z0.clone(), d0.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = run(sz, sd)
        with pytest.raises(RuntimeError, match="capturing"):
            spectral.propagate(sz, [3e-8, 3e-8], LAM, px=PX)               # host defocuses cannot be uploaded inside a capture
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs, want0))
    sz.copy_(z1)
    sd.copy_(d1)
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs, want1))
    assert not torch.equal(want0[1], want1[1])


def test_numpy_and_tensor_conventions():
    z = R.noise(2, 12, 20)
    zd = up(z)
    for fn in (spectral.fft2, spectral.ifft2, lambda v: spectral.propagate(v, 3e-8, LAM, px=PX)):
        a, b, one = fn(z), fn(zd), fn(z[0])
        assert isinstance(a, np.ndarray) and a.dtype == np.complex128 and a.shape == (2, 12, 20) and one.shape == (12, 20)
        assert torch.is_tensor(b) and b.is_cuda and np.array_equal(a, b.cpu().numpy()) and np.array_equal(one, a[0])
        assert tuple(fn(zd[0]).shape) == (12, 20)
    x = z.real
    r = spectral.rfft2(x)                                                  # float64 in: cast to float32
    assert isinstance(r, np.ndarray) and r.shape == (2, 12, 11) and spectral.rfft2(x[0]).shape == (12, 11)
    assert np.array_equal(r, spectral.rfft2(up(x.astype(np.float32))).cpu().numpy())
    assert np.array_equal(spectral.fft2(x.astype(np.float32)), spectral.fft2(x.astype(np.float32).astype(np.complex128)))
    per_image = spectral.propagate(z, [3e-8, -5e-8], LAM, px=PX)
    assert np.array_equal(per_image[0], spectral.propagate(z[0], 3e-8, LAM, px=PX))
    with pytest.raises(ValueError, match="defocus"):
        spectral.propagate(z, [3e-8, -5e-8, 1e-8], LAM, px=PX)


if __name__ == "__main__":
    for line in yardsticks()["log"]:
        print(line)
