"""GPU tests of the 2-D FFT and the radial frequency profile (csrc/fft.hip, emdenoise.harvest.rfft2 / radial_profile / freq_stats;
DESIGN.md 3.19) against numpy.fft in float64 and the restatement of tests/fft_ref.py.

Inputs: ``raw = float32(900) * synthetic_lq(B, S, S, seed=300 + 2 S)[..., 0] - 40``, as the harvest tests use.

Which size runs which schedule of the 1-D transform (radix-4 passes, then a radix-2 pass where log2 S is odd; a thread holds
S / 1024 radix-4 butterflies):
     8: 1 x radix-4 + radix-2, two active threads       16: 2 x radix-4             32: 2 x radix-4 + radix-2
    64: 3 x radix-4                                    128: 3 x radix-4 + radix-2  256: 4 x radix-4, a quarter of the threads idle
  1024: 5 x radix-4, one butterfly per thread; the loads and the split loop over the line
  2048: 5 x radix-4 + radix-2, two butterflies per thread (the profile only)
  4096: 6 x radix-4, four butterflies per thread, the 64 KiB line (the spectrum only)
The row pass has one workgroup per image at 8 and S / 8 from there on; the split's last thread handles kx = S / 2 alone from 512 up.

The bars are not derived from the device's output.

* Spectrum: relative L2 against ``numpy.fft.rfft2`` of the float64 cast.  The bar is FACTOR = 4 times YARD_FFT, the LARGEST relative
  L2 distance, over the sizes <= 256, of the plain float64 radix-2 restatement (fft_ref.fft2_radix2) from the direct DFT evaluated in
  numpy.longdouble -- computed on the CPU by ``python -m tests.test_fft_gpu`` (no GPU) and written below.
* Profile and moments: relative ``(S^2 2^-53 + FACTOR YARD_FFT) x COND_MAX x 10``: sequential double summation of at most S^2
  magnitudes, each carrying the spectrum's error, times the condition number sum |t| / |sum t| of every sum (asserted <= COND_MAX on
  the CPU before the GPU is touched), times 10 for the mean's error entering the central moments.
* radialFreqs: exact.  An impulse at the origin has |F| = 1 everywhere, bit for bit (every butterfly adds zeros to one), so the
  profile is the bins' pixel counts, its sum is S^2 and ``p = count / S^2 * radialFreqs`` is one rounding of an exact factor: p equals
  the restatement's p bitwise iff the device found the reference's last-visited pixel of every non-empty bin.

Every figure is printed before it is asserted."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from emdenoise import _lib, harvest
from tests import fft_ref as F
from tests.synth_inputs import synthetic_lq

pytestmark = pytest.mark.gpu

FACTOR = 4.0
YARD_FFT = 4.624e-16       # the float64 radix-2 restatement's largest relative L2 distance from the long-double DFT (python -m tests.test_fft_gpu)
COND_MAX = 50.0
SPEC_SIZES = [(2, 8), (2, 16), (2, 32), (2, 64), (2, 128), (2, 256), (2, 1024), (1, 4096)]
PROF_SIZES = [(2, 8), (2, 16), (2, 32), (2, 64), (2, 128), (2, 256), (2, 1024), (1, 2048)]
YARD_SIZES = [8, 16, 32, 64, 128, 256]
SENTINEL = -12345.5


def spec_bar():
    return FACTOR * YARD_FFT


def prof_bar(S):
    return (S * S * 2.0 ** -53 + spec_bar()) * COND_MAX * 10.0


@functools.lru_cache(maxsize=None)
def raw(B, S):
    return np.float32(900) * synthetic_lq(B, S, S, seed=300 + 2 * S)[..., 0] - np.float32(40)


@functools.lru_cache(maxsize=None)
def nyquist(S):
    """All the energy on the -S/2 row and the -S/2 column: x[r, c] = (-1)^r + (-1)^c."""
    s = (-1.0) ** np.arange(S)
    return (s[:, None] + s[None, :]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def spectrum64(B, S):
    return np.fft.rfft2(raw(B, S).astype(np.float64))


@functools.lru_cache(maxsize=None)
def profile64(B, S):
    return np.stack([F.radial_profile(im) for im in raw(B, S)])


def rel_l2(a, b):
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def yardstick():
    """The float64 radix-2 restatement's largest relative L2 distance from the long-double direct DFT, sizes <= 256 (CPU only)."""
    worst = 0.0
    for S in YARD_SIZES:
        for im in raw(2, S):
            re, im_ = F.dft2_longdouble(im)
            got = F.fft2_radix2(im)
            num = np.sqrt(float(((got.real - re) ** 2).sum() + ((got.imag - im_) ** 2).sum()))
            den = np.sqrt(float((re ** 2).sum() + (im_ ** 2).sum()))
            print(f"yardstick S = {S}: radix-2 float64 vs long-double DFT rel L2 {num / den:.3e}")
            worst = max(worst, num / den)
    return worst


def dev():
    return torch.device("cuda", 0)


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev())


def check_conditions(im, what):
    cond = F.condition_numbers(im)
    print(f"condition numbers {what}: {cond}")
    assert max(cond.values()) <= COND_MAX


def assert_close(got, want, bar, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    e = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    e = np.where(want == 0, np.abs(got), e)
    print(f"{what}: largest relative distance {e.max():.3e}; bar {bar:.3e}")
    assert (e <= bar).all(), what


# ---- the spectrum ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", SPEC_SIZES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_rfft2(case):
    B, S = case
    assert YARD_FFT > 0
    want = spectrum64(B, S)
    got = harvest.rfft2(up(raw(B, S)))
    assert got.is_cuda and got.dtype == torch.complex128 and tuple(got.shape) == (B, S, S // 2 + 1)
    got = got.cpu().numpy()
    e = rel_l2(got, want)
    print(f"rfft2 [{B},{S},{S}]: rel L2 {e:.3e}; bar {spec_bar():.3e} (radix-2 restatement's largest {YARD_FFT:.3e})")
    assert e <= spec_bar()
    for kx in (0, S // 2):                                                  # the Hermitian edge columns
        ek = rel_l2(got[:, :, kx], want[:, :, kx])
        herm = np.abs(got[:, 1:, kx] - np.conj(got[:, :0:-1, kx])).max() / np.abs(want[:, :, kx]).max()
        print(f"  column kx = {kx}: rel L2 {ek:.3e}; F(ky) - conj F(-ky) relative to the column's largest {herm:.3e}")
        assert ek <= spec_bar() and herm <= spec_bar()
        assert (np.abs(got[:, [0, S // 2], kx].imag) <= spec_bar() * np.abs(want[:, :, kx]).max()).all()   # the four real entries


@pytest.mark.parametrize("S", [8, 32, 64, 1024])
def test_impulse_gives_the_phase_ramp(S):
    x = np.zeros((S, S), np.float32)
    x[1, 2] = 1.0
    got = harvest.rfft2(up(x)).cpu().numpy()
    ky, kx = np.arange(S)[:, None], np.arange(S // 2 + 1)[None, :]
    want = np.exp(-2j * np.pi * ((ky * 1 + kx * 2) % S) / S)
    e = np.abs(got - want).max()
    print(f"impulse at (1, 2), S = {S}: largest distance from exp(-2 pi i (ky + 2 kx) / S) {e:.3e}; bound {S * 2.0 ** -52:.3e}")
    assert got.shape == (S, S // 2 + 1) and e <= S * 2.0 ** -52           # unit-modulus products of log2 S twiddles, far below
    assert np.abs(got - np.conj(want)).max() > 0.5 and np.abs(got - np.exp(-2j * np.pi * ((ky * 2 + kx) % S) / S)).max() > 0.5


# ---- the profile and its moments ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", PROF_SIZES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_freq_stats_and_profile(case):
    B, S = case
    x = raw(B, S)
    for i, im in enumerate(x):                                             # a condition of the bound, before the GPU is touched
        check_conditions(im, f"[{i}] of {case}")
    want_p = profile64(B, S)
    want = np.stack([F.moments(p) for p in want_p])
    xd = up(x)
    got, got_p = harvest.freq_stats(xd), harvest.radial_profile(xd)
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (B, 4)
    assert got_p.is_cuda and got_p.dtype == torch.float64 and tuple(got_p.shape) == (B, F.radial_bins(S))
    got, got_p = got.cpu().numpy(), got_p.cpu().numpy()
    print(f"freq_stats {case}: {got} (numpy {want})")
    for k, name in enumerate(harvest.FREQ_NAMES):
        assert_close(got[:, k], want[:, k], prof_bar(S), f"{name} {case}")
    assert_close(got_p, want_p, prof_bar(S), f"radial_profile per bin {case}")
    empty = ~F.radial_freqs(S)[1]
    assert empty.sum() == {8: 1, 32: 1}.get(S, 0) and (got_p[:, empty] == 0).all()


@pytest.mark.parametrize("S", [8, 32, 256])
def test_nyquist_row_and_column_are_counted_once(S):
    x = nyquist(S)
    check_conditions(x, f"nyquist {S}")
    want_p = F.radial_profile(x)
    want = F.moments(want_p)
    assert np.count_nonzero(want_p > 1e-9) == 1                            # one bin: t = S / 2 holds (-S/2, 0) and (0, -S/2)
    got, got_p = harvest.freq_stats(up(x)).cpu().numpy()[0], harvest.radial_profile(up(x)).cpu().numpy()[0]
    print(f"nyquist S = {S}: {got} (numpy {want}); p[S/2] = {got_p[S // 2]} (numpy {want_p[S // 2]})")
    assert_close(got, want, prof_bar(S), f"nyquist moments {S}")
    assert_close(got_p[S // 2], want_p[S // 2], prof_bar(S), f"nyquist bin {S}")
    assert np.abs(np.delete(got_p, S // 2)).max() <= prof_bar(S)


@pytest.mark.parametrize("S", [8, 16, 32, 64, 256, 1024])
def test_radial_freqs_follow_the_last_visited_pixel_exactly(S):
    x = np.zeros((S, S), np.float32)
    x[0, 0] = 1.0
    spec = harvest.rfft2(up(x)).cpu().numpy()
    assert np.array_equal(spec, np.ones_like(spec))                        # |F| = 1 bit for bit
    bins, _, R = F.geometry(S)
    freqs, nonempty = F.radial_freqs(S)
    count = np.bincount(bins.ravel(), minlength=R).astype(np.float64)
    want = count / float(S * S) * freqs
    got = harvest.radial_profile(up(x)).cpu().numpy()[0]
    recovered = got[nonempty] / (count[nonempty] / float(S * S))
    print(f"S = {S}: {int(nonempty.sum())} non-empty bins of {R}; p equal bitwise: {np.array_equal(got, want)}; radialFreqs recovered "
          f"to {np.abs(recovered - freqs[nonempty]).max():.2e}")
    assert np.array_equal(got, want)
    loop_freqs = F.profile_loop(np.ones((S, S)))[1] if S <= 32 else freqs
    assert np.array_equal(loop_freqs, freqs)


# ---- img_params -----------------------------------------------------------------------------------------------------------------

def test_img_params_with_the_frequency_fields():
    img = np.float32(900) * synthetic_lq(1, 70, 131, seed=501)[0, :, :, 0] - np.float32(40)
    x = up(img)
    plain, image0 = harvest.img_params(x, 32)
    stats, image = harvest.img_params(x, 32, freq=True)
    fs = harvest.freq_stats(harvest.box_resize(x, 32)).cpu().numpy()[0]
    for k, v in harvest.FIELDS_FREQ.items():
        print(f"{k} = {stats[k]!r} (freq_stats {fs[harvest.FREQ_NAMES.index(v)]!r})")
        assert stats[k] == fs[harvest.FREQ_NAMES.index(v)] and isinstance(stats[k], float)
    assert {k: v for k, v in stats.items() if k not in harvest.FIELDS_FREQ} == plain and len(stats) == len(plain) + 4
    assert not [k for k in plain if "Freq" in k] and torch.equal(image, image0)
    want = F.freq_stats(harvest.box_resize(x, 32).cpu().numpy())
    assert_close([stats[k] for k in harvest.FIELDS_FREQ], want, prof_bar(32), "img_params frequency fields")
    stack, table = harvest.harvest([img, img[:40, :50]], 16, freq=True)
    assert stack.shape == (2, 16, 16, 1) and all(set(harvest.FIELDS_FREQ) <= set(t) for t in table)
    assert table[1]["meanFreq2048"] == harvest.freq_stats(harvest.box_resize(img[:40, :50], 16))[0, 0]
    assert not set(harvest.FIELDS_FREQ) & set(harvest.harvest([img], 16)[1][0])


# ---- degenerate images ----------------------------------------------------------------------------------------------------------

def test_zero_and_constant_images_give_the_documented_nans():
    x = np.stack([raw(2, 32)[0], np.zeros((32, 32), np.float32), np.full((32, 32), 7.25, np.float32), raw(2, 32)[1]])
    got = harvest.freq_stats(up(x)).cpu().numpy()
    p = harvest.radial_profile(up(x)).cpu().numpy()
    print(f"zero image: {got[1]}; constant image: {got[2]}")
    assert np.isnan(got[1]).all() and np.isnan(p[1]).all()                 # 0 / 0 in the normalisation
    assert got[2, 0] == 0 and got[2, 1] == 0 and np.isnan(got[2, 2:]).all() and (p[2] == 0).all()
    assert np.array_equal(got[[0, 3]], harvest.freq_stats(up(raw(2, 32))).cpu().numpy())    # the others are undisturbed
    assert np.isfinite(got[[0, 3]]).all()


# ---- conventions, bits and safety -----------------------------------------------------------------------------------------------

def test_numpy_and_tensor_conventions():
    x4 = raw(2, 16)[..., None]
    R = F.radial_bins(16)
    for a in (x4, x4[..., 0], x4[0, :, :, 0]):
        keep = a.copy()
        lead = () if a.ndim == 2 else (2,)
        tail = (1,) if a.ndim == 4 else ()
        s, st = harvest.rfft2(a), harvest.rfft2(up(a))
        assert isinstance(s, np.ndarray) and s.dtype == np.complex128 and s.shape == lead + (16, 9) + tail and np.array_equal(a, keep)
        assert isinstance(st, torch.Tensor) and st.is_cuda and tuple(st.shape) == s.shape and np.array_equal(s, st.cpu().numpy())
        p, pt = harvest.radial_profile(a), harvest.radial_profile(up(a))
        assert isinstance(p, np.ndarray) and p.dtype == np.float64 and p.shape == (len(lead) and 2 or 1, R)
        assert np.array_equal(p, pt.cpu().numpy())
        f, ft = harvest.freq_stats(a), harvest.freq_stats(up(a))
        assert isinstance(f, np.ndarray) and f.dtype == np.float64 and f.shape == (p.shape[0], 4) and np.array_equal(f, ft.cpu().numpy())
    stats, image = harvest.img_params(x4[0, :, :, 0], 8, freq=True)
    assert isinstance(image, np.ndarray) and image.shape == (8, 8) and isinstance(stats["meanFreq2048"], float)


def test_bitwise_reproducible_and_independent_of_the_batch():
    x = up(np.concatenate([raw(2, 64), nyquist(64)[None]]))
    run = lambda t: (harvest.rfft2(t), harvest.radial_profile(t), harvest.freq_stats(t))
    a, b = run(x), run(x)
    assert all(torch.equal(torch.view_as_real(p) if p.is_complex() else p, torch.view_as_real(q) if q.is_complex() else q)
               for p, q in zip(a, b))
    for i in range(3):
        one = run(x[i:i + 1].clone())                                      # alone = inside a batch of other images
        for p, q in zip(one, a):
            assert np.array_equal(p[0].cpu().numpy(), q[i].cpu().numpy()), i
    assert not torch.isnan(a[2]).any()


class Guarded:
    """`nbytes` bytes, 256-byte aligned, inside a sentinel-filled buffer with 4 KiB of guard on either side."""
    GUARD = 1024   # floats

    def __init__(self, nbytes):
        self.n = (nbytes + 3) // 4
        self.buf = torch.full((self.n + 2 * self.GUARD + 64,), SENTINEL, dtype=torch.float32, device=dev())
        self.off = self.GUARD + (-(self.buf.data_ptr() // 4 + self.GUARD)) % 64
        self.view = self.buf[self.off:self.off + self.n]
        assert self.view.data_ptr() % 256 == 0

    def ptr(self):
        return C.c_void_p(self.view.data_ptr())

    def intact(self):
        return bool((self.buf[:self.off] == SENTINEL).all()) and bool((self.buf[self.off + self.n:] == SENTINEL).all())


def test_outputs_and_workspace_stay_inside_their_advertised_sizes():
    lib = _lib.load()
    st = _lib.stream_ptr()
    for B, S in ((2, 8), (3, 32), (2, 128)):
        x = up(raw(2, S)[[0, 1, 0][:B]])
        R = lib.emd_radial_bins(S)
        nbytes = lib.emd_rfft2_workspace_bytes(B, S)
        spec, ws = Guarded(B * S * (S // 2 + 1) * 16), Guarded(nbytes)
        _lib.check(lib.emd_rfft2_f64(x.data_ptr(), B, S, spec.ptr(), ws.ptr(), nbytes, st), "rfft2")
        torch.cuda.synchronize()
        assert spec.intact(), "wrote outside [B][S][S/2+1][2]"
        assert ws.intact(), f"wrote outside its {nbytes}-byte workspace"
        got = torch.view_as_complex(spec.view.view(torch.float64).reshape(B, S, S // 2 + 1, 2))
        assert torch.equal(torch.view_as_real(got), torch.view_as_real(harvest.rfft2(x)))
        nbytes = lib.emd_freq_stats_workspace_bytes(B, S)
        prof, fs, ws = Guarded(B * R * 8), Guarded(B * 4 * 8), Guarded(nbytes)
        _lib.check(lib.emd_freq_stats_f64(x.data_ptr(), B, S, prof.ptr(), fs.ptr(), ws.ptr(), nbytes, st), "freq_stats")
        torch.cuda.synchronize()
        assert prof.intact() and fs.intact(), "wrote outside [B][R] or [B][4]"
        assert ws.intact(), f"wrote outside its {nbytes}-byte workspace"
        assert torch.equal(fs.view.view(torch.float64).reshape(B, 4), harvest.freq_stats(x))
        assert torch.equal(prof.view.view(torch.float64).reshape(B, R), harvest.radial_profile(x))
        fs2, ws2 = Guarded(B * 4 * 8), Guarded(nbytes)                     # without the profile
        _lib.check(lib.emd_freq_stats_f64(x.data_ptr(), B, S, None, fs2.ptr(), ws2.ptr(), nbytes, st), "freq_stats")
        torch.cuda.synchronize()
        assert fs2.intact() and ws2.intact() and torch.equal(fs2.view, fs.view)


def test_captured_in_one_graph_and_replayed_on_new_contents():
    x0, x1 = up(raw(2, 64)), up(raw(2, 64)[::-1].copy() * 0.5 + 0.25)
    run = lambda t: (torch.view_as_real(harvest.rfft2(t)), harvest.freq_stats(t))
    want0, want1 = run(x0), run(x1)                                        # eager
    static = x0.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = run(static)
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs, want0))
    static.copy_(x1)
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs, want1))


if __name__ == "__main__":
    y = yardstick()
    print(f"spectrum: radix-2 float64 restatement's largest {y:.3e}; bar {FACTOR * y:.3e}")
    for B, S in PROF_SIZES:
        for im in raw(B, S):
            print(S, F.condition_numbers(im))
    for S in (8, 32, 256):
        print("nyquist", S, F.condition_numbers(nyquist(S)))
