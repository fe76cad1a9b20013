"""GPU tests of the wavelet transform and wavelet shrinkage (csrc/wavelet.hip, emdenoise.filters wavedec2 / waverec2 /
denoise_wavelet) against the float64 restatement of tests/wavelet_ref.py.

Inputs are ``synthetic_lq`` plus continuous Gaussian noise (sigma 0.02), rounded to float32: on the quantised synthetic images alone,
which coefficients are exactly zero differs between float32 and float64 arithmetic, and the noise estimate drops exact zeros.  A
CPU-side condition checks that for every end-to-end case: the exactly-zero dd_1 coefficients of the float32 and the float64
restatement are the same set.

The bars are not derived from the device's output.  For each quantity the bar is FACTOR = 4 times the LARGEST relative L2 distance
of the float32 restatement from the float64 one over the cases of this file, computed once on the CPU by
``python -m tests.test_wavelet_gpu`` (it prints them; no GPU) and written below as constants:

    quantity                               float32 restatement, largest    bar (4 x)
    wavedec2, any band                     1.440e-6  (YARD_BANDS)          5.76e-6
    waverec2(wavedec2(x)) against x        3.301e-7  (YARD_ROUNDTRIP)      1.32e-6
    denoise_wavelet, given sigma 0.02      3.386e-7  (YARD_GIVEN)          1.35e-6
    denoise_wavelet, estimated sigma       3.214e-7  (YARD_ESTIMATED)      1.29e-6

The noise estimate is checked teacher-forced on the device's own coefficients against numpy's median: relative 2.4e-7, two
float32 ulps (one for the mean of the two middle values, one for the division), derived and not measured.  Every figure is
printed before it is asserted; DESIGN.md 3.17 has the device's measured distances beside the bars.

Measured on an MI355X, the largest over the cases: bands 1.44e-6, round trip 3.32e-7, given sigma 3.37e-7,
estimated sigma 3.14e-7, sigma 4.64e-8 relative."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import emdenoise
from emdenoise import _lib, filters
from tests import wavelet_ref as R
from tests.synth_inputs import synthetic_lq

pytestmark = pytest.mark.gpu

FACTOR = 4.0
# the float32 restatement's largest relative L2 distance from the float64 one (python -m tests.test_wavelet_gpu)
YARD_BANDS = 1.440e-6
YARD_ROUNDTRIP = 3.301e-7
YARD_GIVEN = 3.386e-7
YARD_ESTIMATED = 3.214e-7
SIGMA_RTOL = 2.4e-7

# odd sizes, 131 columns: several tiles at level 1 and more than one at level 2; a power of two; the thinnest one level of db2
# allows; the default rule gives 4 levels for Haar at 128
SHAPES = [(3, 37, 53), (2, 70, 131), (2, 64, 64), (2, 8, 200), (2, 200, 8), (1, 128, 128)]
DB4 = tuple(R.daubechies(4))
GIVEN_SIGMA = 0.02


def wavelets_for(shape):
    return ["db1", "db2"] + ([DB4] if min(shape[1:]) >= 14 else [])


def levels_for(shape, wavelet):
    top = R.max_levels(shape[1], shape[2], len(R.rec_lo_of(wavelet)))
    return [l for l in (1, 2, 3) if l <= top] + [None]


def cases():
    return [(s, w, l) for s in SHAPES for w in wavelets_for(s) for l in levels_for(s, w)]


def cid(c):
    s, w, l = c
    return f"{'x'.join(map(str, s))}-{w if isinstance(w, str) else 'db4'}-{l}"


@functools.lru_cache(maxsize=None)
def images(shape):
    B, H, W = shape
    rng = np.random.default_rng(700 + H * 1000 + W)
    return (synthetic_lq(B, H, W, seed=300 + H + W)[..., 0].astype(np.float64) + 0.02 * rng.standard_normal(shape)).astype(np.float32)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def bands_of(coeffs):
    return [("cA", coeffs[0])] + [(f"{k}{len(coeffs) - 1 - i}", d[k]) for i, d in enumerate(coeffs[1:]) for k in ("ad", "da", "dd")]


@functools.lru_cache(maxsize=None)
def dec64(case):
    s, w, l = case
    return R.wavedec2(images(s), w, l, np.float64)


@functools.lru_cache(maxsize=None)
def den64(case, method, sigma):
    s, w, l = case
    return R.denoise_wavelet(images(s), w, l, method, sigma, np.float64)


def same_zero_set(case):
    """The condition of the end-to-end comparison: float32 and float64 arithmetic agree on which dd_1 coefficients are exactly 0."""
    s, w, l = case
    return np.array_equal(R.wavedec2(images(s), w, l, np.float32)[-1]["dd"] == 0, dec64(case)[-1]["dd"] == 0)


def yardsticks():
    """The float32 restatement's largest distances from the float64 one over the cases of this file (CPU only)."""
    y = {"bands": 0.0, "roundtrip": 0.0, "given": 0.0, "estimated": 0.0}
    for case in cases():
        s, w, l = case
        x = images(s)
        c32 = R.wavedec2(x, w, l, np.float32)
        y["bands"] = max([y["bands"]] + [rel_l2(a, b) for (_, a), (_, b) in zip(bands_of(c32), bands_of(dec64(case)))])
        y["roundtrip"] = max(y["roundtrip"], rel_l2(R.waverec2(c32, w, x.shape, np.float32), x))
        for m in R.METHODS:
            y["given"] = max(y["given"], rel_l2(R.denoise_wavelet(x, w, l, m, GIVEN_SIGMA, np.float32), den64(case, m, GIVEN_SIGMA)))
            assert same_zero_set(case), case
            y["estimated"] = max(y["estimated"], rel_l2(R.denoise_wavelet(x, w, l, m, None, np.float32), den64(case, m, None)))
    return y


def dev():
    return torch.device("cuda", 0)


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev())


def wv(w):
    return w if isinstance(w, str) else np.array(w)


def check(what, case, got, want, yard):
    e = rel_l2(got, want)
    print(f"{what} {cid(case)}: rel L2 {e:.3e}; bar {FACTOR * yard:.3e} (float32 restatement's largest {yard:.3e})")
    assert e <= FACTOR * yard, (what, cid(case), e, FACTOR * yard)


# ---- the transform -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", cases(), ids=cid)
def test_wavedec2_and_waverec2(case):
    s, w, l = case
    x = up(images(s))
    c = filters.wavedec2(x, wv(w), l)
    ref = dec64(case)
    assert len(c) == len(ref)
    for (name, a), (_, b) in zip(bands_of(c), bands_of(ref)):
        assert a.is_cuda and tuple(a.shape) == b.shape, name
        check(f"wavedec2 {name}", case, a.cpu().numpy(), b, YARD_BANDS)
    back = filters.waverec2(c, wv(w), x.shape)
    assert back.is_cuda and back.shape == x.shape
    check("waverec2(wavedec2)", case, back.cpu().numpy(), images(s), YARD_ROUNDTRIP)


def test_numpy_and_tensor_conventions():
    x4 = images((2, 70, 131))[..., None]
    for a in (x4, x4[..., 0], x4[0, :, :, 0]):
        keep = a.copy()
        c = filters.wavedec2(a, "db2", 2)
        ct = filters.wavedec2(up(a), "db2", 2)
        assert isinstance(c[0], np.ndarray) and c[0].dtype == np.float32 and np.array_equal(a, keep)
        for (_, p), (_, q) in zip(bands_of(c), bands_of(ct)):
            assert isinstance(q, torch.Tensor) and p.shape == tuple(q.shape) and p.ndim == a.ndim and np.array_equal(p, q.cpu().numpy())
        y, yt = filters.waverec2(c, "db2", a.shape), filters.waverec2(ct, "db2", a.shape)
        assert isinstance(y, np.ndarray) and y.shape == a.shape and np.array_equal(y, yt.cpu().numpy())
        d, dt = filters.denoise_wavelet(a), filters.denoise_wavelet(up(a))
        assert isinstance(d, np.ndarray) and d.shape == a.shape and d.dtype == np.float32 and np.array_equal(d, dt.cpu().numpy())
    y, s = filters.denoise_wavelet(x4, return_sigma=True)
    assert isinstance(s, np.ndarray) and s.shape == (2,) and s.dtype == np.float32


# ---- the noise estimate, teacher-forced on the device's own coefficients --------------------------------------------------------

def numpy_sigma(dd1, drop_zeros=True):
    a = np.abs(dd1.ravel())
    if drop_zeros:
        a = a[a != 0]
    return np.float64(np.median(a)) / 0.67448975 if a.size else 0.0


def test_sigma_is_the_exact_median_of_the_nonzero_coefficients():
    parities = set()
    for case in cases():
        s, w, l = case
        x = up(images(s))
        _, sig = filters.denoise_wavelet(x, wv(w), l, return_sigma=True)
        dd1 = filters.wavedec2(x, wv(w), l)[-1]["dd"].cpu().numpy()
        for b in range(s[0]):
            want = numpy_sigma(dd1[b])
            parities.add(int(np.count_nonzero(dd1[b])) % 2)
            e = abs(float(sig[b]) - want) / want
            print(f"sigma {cid(case)} image {b}: {float(sig[b]):.9e} (numpy {want:.9e}); relative {e:.2e}; bound {SIGMA_RTOL:.1e}")
            assert e <= SIGMA_RTOL
    assert parities == {0, 1}                                              # odd and even counts


def test_sigma_drops_exact_zeros():
    x = images((2, 70, 131)).copy()
    x[:, :, :66] = 0.0                                                     # the left half is exactly 0.0
    x[1] = 0.0                                                             # and an image that is all zero
    for w in ("db1", "db2"):
        y, sig = filters.denoise_wavelet(up(x), w, 2, return_sigma=True)
        dd1 = filters.wavedec2(up(x), w, 2)[-1]["dd"].cpu().numpy()
        assert np.count_nonzero(dd1[0] == 0) > dd1[0].size // 3
        want, with_zeros = numpy_sigma(dd1[0]), numpy_sigma(dd1[0], drop_zeros=False)
        e = abs(float(sig[0]) - want) / want
        print(f"sigma, left half zero, {w}: {float(sig[0]):.9e} (numpy {want:.9e}, with the zeros {with_zeros:.9e}); relative {e:.2e}")
        assert e <= SIGMA_RTOL
        assert abs(float(sig[0]) - with_zeros) > 0.5 * float(sig[0])       # the with-zeros median is another number altogether
        assert float(sig[1]) == 0.0 and torch.equal(y[1].cpu(), torch.zeros(70, 131))    # sigma 0, output equal to input
        for method in R.METHODS:                                           # a given sigma = 0 returns x through the transform
            y0 = filters.denoise_wavelet(up(x), w, 2, method, sigma=0.0)
            assert rel_l2(y0.cpu().numpy(), x) <= FACTOR * YARD_ROUNDTRIP


def parted_image():
    """[2, 130, 140]: one non-zero pixel in each 2 x 2 block, so that Haar's dd_1 (65 x 70 = 4550 coefficients: two chunks of the
    selection, the second ragged) is half that pixel; as many magnitudes in [1, 3) as in [5, 7), ten blocks all zero.  The second
    image is the first with one more block zeroed."""
    rng = np.random.default_rng(41)
    nb = 65 * 70
    mag = np.concatenate([rng.uniform(1.0, 3.0, (nb - 10) // 2), rng.uniform(5.0, 7.0, (nb - 10) // 2), np.zeros(10)])
    mag = rng.permutation(mag) * rng.choice([-1.0, 1.0], nb)
    r, c = np.divmod(np.arange(nb), 70)
    x = np.zeros((2, 130, 140), np.float32)
    x[0, 2 * r + rng.integers(0, 2, nb), 2 * c + rng.integers(0, 2, nb)] = mag
    x[1] = x[0]
    k = int(np.flatnonzero(mag)[0])
    x[1, 2 * r[k]:2 * r[k] + 2, 2 * c[k]:2 * c[k] + 2] = 0.0
    return x


def middle_values_part_at_the_top_byte(dd1):
    """The precondition of the test below, on a [2, 65, 70] dd_1: an even count of non-zeros in the first image, whose two middle
    magnitudes lie on either side of 2.0 (bit patterns 0x3f...... and 0x40......), and an odd count in the second."""
    a = [np.sort(np.abs(d[d != 0])) for d in dd1]
    lo, hi = a[0][a[0].size // 2 - 1:a[0].size // 2 + 1]
    return (dd1.shape == (2, 65, 70) and a[0].size % 2 == 0 and a[0].size < dd1[0].size and a[1].size == a[0].size - 1
            and lo < 2.0 <= hi and int(lo.view(np.uint32)) >> 24 != int(hi.view(np.uint32)) >> 24)


def test_sigma_when_the_middle_ranks_part_at_the_first_pass():
    x = up(parted_image())
    _, sig = filters.denoise_wavelet(x, "db1", 1, return_sigma=True)
    dd1 = filters.wavedec2(x, "db1", 1)[-1]["dd"].cpu().numpy()
    assert middle_values_part_at_the_top_byte(dd1)
    for b in range(2):
        want = numpy_sigma(dd1[b])
        e = abs(float(sig[b]) - want) / want
        print(f"sigma, middle ranks in two bins of pass 0, image {b}: {float(sig[b]):.9e} (numpy {want:.9e}); relative {e:.2e}; "
              f"bound {SIGMA_RTOL:.1e}")
        assert e <= SIGMA_RTOL


# ---- the denoiser against float64 -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", cases(), ids=cid)
def test_denoise_wavelet_given_sigma(case):
    s, w, l = case
    x = up(images(s))
    for m in R.METHODS:
        y, sig = filters.denoise_wavelet(x, wv(w), l, m, GIVEN_SIGMA, return_sigma=True)
        assert torch.equal(sig.cpu(), torch.full((s[0],), GIVEN_SIGMA, dtype=torch.float32))
        check(f"denoise_wavelet {m} sigma {GIVEN_SIGMA}", case, y.cpu().numpy(), den64(case, m, GIVEN_SIGMA), YARD_GIVEN)


@pytest.mark.parametrize("case", cases(), ids=cid)
def test_denoise_wavelet_estimated_sigma(case):
    s, w, l = case
    assert same_zero_set(case)                                             # a condition of the comparison, not a tolerance
    x = up(images(s))
    for m in R.METHODS:
        check(f"denoise_wavelet {m} estimated", case, filters.denoise_wavelet(x, wv(w), l, m).cpu().numpy(), den64(case, m, None),
              YARD_ESTIMATED)


# ---- bits and safety ------------------------------------------------------------------------------------------------------------

def test_bitwise_reproducible_and_independent_of_the_batch():
    x = up(images((2, 70, 131)))
    for w, l in (("db1", None), ("db2", 3), (np.array(DB4), 2)):
        a, sa = filters.denoise_wavelet(x, w, l, return_sigma=True)
        b, sb = filters.denoise_wavelet(x, w, l, return_sigma=True)
        assert torch.equal(a, b) and torch.equal(sa, sb)
        one, s1 = filters.denoise_wavelet(x[1:2].clone(), w, l, return_sigma=True)   # alone = inside a batch of other images
        assert torch.equal(one[0], a[1]) and torch.equal(s1[0], sa[1])
        ca, cb = filters.wavedec2(x, w, l), filters.wavedec2(x[1:2].clone(), w, l)
        assert all(torch.equal(p[1], q[0]) for (_, p), (_, q) in zip(bands_of(ca), bands_of(cb)))


SENTINEL = -12345.5


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


def test_outputs_and_workspaces_stay_inside_their_advertised_sizes():
    lib = _lib.load()
    B, H, W = 2, 70, 131
    x = up(images((B, H, W)))
    st = _lib.stream_ptr()
    for taps, levels in ((R.rec_lo_of("db1"), 3), (R.rec_lo_of("db2"), 2), (np.array(DB4), 3)):
        L, tp = len(taps), taps.ctypes.data_as(C.c_void_p)
        total = lib.emd_wavelet_pyramid_floats(H, W, L, levels, None)
        tb, fb = lib.emd_wavelet_workspace_bytes(B, H, W, L, levels), lib.emd_filter_wavelet_workspace_bytes(B, H, W, L, levels)
        pyr, ws = Guarded(B * total * 4), Guarded(tb)
        _lib.check(lib.emd_wavelet_forward_f32(x.data_ptr(), pyr.ptr(), B, H, W, tp, L, levels, ws.ptr(), tb, st), "forward")
        torch.cuda.synchronize()
        assert pyr.intact() and ws.intact() and bool((pyr.view != SENTINEL).all())
        out, ws = Guarded(B * H * W * 4), Guarded(tb)
        _lib.check(lib.emd_wavelet_inverse_f32(pyr.ptr(), out.ptr(), B, H, W, tp, L, levels, ws.ptr(), tb, st), "inverse")
        torch.cuda.synchronize()
        assert out.intact() and ws.intact() and pyr.intact() and bool((out.view != SENTINEL).all())
        for sigma in (-1.0, 0.02):
            out, used, ws = Guarded(B * H * W * 4), Guarded(B * 4), Guarded(fb)
            _lib.check(lib.emd_filter_wavelet_f32(x.data_ptr(), out.ptr(), B, H, W, tp, L, levels, 0, C.c_float(sigma), used.ptr(), ws.ptr(),
                                                  fb, st), "filter")
            torch.cuda.synchronize()
            assert out.intact(), "wrote outside out"
            assert used.intact() and bool((used.view != SENTINEL).all()), "sigma_used"
            assert ws.intact(), f"wrote outside its {fb}-byte workspace"
            assert bool((out.view != SENTINEL).all()), "left output pixels unwritten"


def test_captured_in_one_graph_and_replayed_on_new_contents():
    x0, x1 = up(images((2, 70, 131))), up(images((2, 70, 131))[::-1].copy() * 0.5 + 0.25)
    run = lambda t: filters.denoise_wavelet(t, "db2", 2, return_sigma=True)
    want0, want1 = run(x0), run(x1)                                        # eager (and warm)
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


# ---- the seven-column table ---------------------------------------------------------------------------------------------------

def test_baseline_table_reference_columns():
    from emdenoise.input_pipeline import DeviceRecordParser

    hq = up(synthetic_lq(4, 64, 64, seed=77) * 200.0 + 5.0)
    lq, truth = DeviceRecordParser(dev(), seed=3)(hq)                      # Poisson LQ / truth pairs [4,64,64,1]
    data, labels = emdenoise.baseline_table(lq, truth, reference_columns=True, denoise_wavelet={"wavelet": "db2"})
    assert labels == filters.REFERENCE_LABELS and data.is_cuda and data.shape == (4, 7, 2)
    y = filters.denoise_wavelet(lq, wavelet="db2")
    _, mse = emdenoise.psnr(y, truth, per_image=True, return_mse=True)
    assert torch.equal(data[:, 5, 0], mse) and torch.equal(data[:, 5, 1], emdenoise.ssim(y, truth, per_image=True))
    six, labels6 = emdenoise.baseline_table(lq, truth)
    assert labels6 == filters.LABELS and six.shape == (4, 6, 2)
    assert torch.equal(data[:, [0, 1, 2, 3, 4, 6]], six)
    assert not torch.equal(data[:, 5], data[:, 0])


if __name__ == "__main__":
    for k, v in yardsticks().items():
        print(f"{k}: float32 restatement's largest {v:.3e}; bar {FACTOR * v:.3e}")
