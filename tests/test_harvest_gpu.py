"""GPU tests of the harvester (csrc/harvest.hip, emdenoise.harvest) against the float64 restatement of
tests/harvest_ref.py.

Inputs: ``x01 = synthetic_lq(B, H, W, seed=300 + H + W)[..., 0]`` and ``raw = float32(900) * x01 - 40`` with ``raw[:, ::7, ::5] = 0``:
negatives, exact zeros and heavy duplicates (the synthetic images are quantised counts), so the median meets ties.

The bars are not derived from the device's output.

* Resize: relative L2 against the float64 restatement (MATLAB's general algorithm as W X W^T).  The bar is FACTOR = 4 times the
  LARGEST relative L2 distance of the float32 restatement from the float64 one over the resize cases of this file, computed once on
  the CPU by ``python -m tests.test_harvest_gpu`` (it prints it; no GPU) and written below as YARD_RESIZE.  64 -> 64 is bitwise.
* Statistics, teacher-forced on the device's own input arrays: min, max, nonzero, negative and median are exactly numpy's on the
  float64 cast.  The other twelve: relative 1e-9, derived: sequential double summation of N <= 16 900 terms has worst case
  N 2^-53 = 1.9e-12, times the condition number sum |t| / |sum t| of each sum, which the test computes on the CPU and asserts to be
  <= 50 for its inputs before it touches the GPU (measured <= 7); the remaining x10 covers the mean's error entering the central
  moments.
* scale01: absolute 2.4e-7, two float32 ulps at 1 (one subtraction, one division), against float32 numpy.

Every figure is printed before it is asserted."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from emdenoise import _lib, harvest
from tests import harvest_ref as R
from tests.synth_inputs import synthetic_lq

pytestmark = pytest.mark.gpu

FACTOR = 4.0
YARD_RESIZE = 5.554e-8     # the float32 restatement's largest relative L2 distance from the float64 one (python -m tests.test_harvest_gpu)
STATS_RTOL = 1e-9
COND_MAX = 50.0
SCALE_ATOL = 2.4e-7
EXACT = ["min", "max", "nonzero", "negative", "median"]

SHAPES = [(3, 37, 53), (2, 70, 131), (1, 128, 128), (2, 3, 200)]
# (H, W, S): 8 -> 4 and 12 -> 8 whole ratios; 7 -> 4 and 37 -> 16 runs of differing counts; 100 -> 64; 64 -> 64 the identity; 5 -> 8 an
# upscale; a 70 x 131 image cropped to 70; 300 x 260 -> 96 several tiles and LDS segments; 150 -> 7 runs of 21-22
RESIZE_CASES = [(8, 8, 4), (12, 12, 8), (7, 7, 4), (37, 37, 16), (100, 100, 64), (64, 64, 64), (5, 5, 8), (70, 131, 32), (300, 260, 96),
                (150, 150, 7)]


@functools.lru_cache(maxsize=None)
def x01(shape):
    B, H, W = shape
    return synthetic_lq(B, H, W, seed=300 + H + W)[..., 0]


@functools.lru_cache(maxsize=None)
def raw(shape):
    r = np.float32(900) * x01(shape) - np.float32(40)
    r[:, ::7, ::5] = 0
    return r


@functools.lru_cache(maxsize=None)
def resized64(case):
    H, W, S = case
    return R.box_resize(raw((2, H, W)), S)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def yardstick():
    """The float32 restatement's largest distance from the float64 one over RESIZE_CASES (CPU only)."""
    return max(rel_l2(R.box_resize(raw((2, c[0], c[1])), c[2], np.float32), resized64(c)) for c in RESIZE_CASES)


def dev():
    return torch.device("cuda", 0)


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev())


# ---- resize ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", RESIZE_CASES, ids=lambda c: f"{c[0]}x{c[1]}-{c[2]}")
def test_box_resize(case):
    H, W, S = case
    x = raw((2, H, W))
    y = harvest.box_resize(up(x), S)
    assert y.is_cuda and tuple(y.shape) == (2, S, S) and y.dtype == torch.float32
    e = rel_l2(y.cpu().numpy(), resized64(case))
    print(f"box_resize {H}x{W} -> {S}: rel L2 {e:.3e}; bar {FACTOR * YARD_RESIZE:.3e} (float32 restatement's largest {YARD_RESIZE:.3e})")
    assert e <= FACTOR * YARD_RESIZE
    if min(H, W) == S:
        assert np.array_equal(y.cpu().numpy(), x[:, :S, :S])               # the identity, bit for bit


# ---- statistics -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_image_stats(shape):
    x = raw(shape)
    want = np.stack([R.image_stats(im) for im in x])
    for im in x:                                                           # a condition of the bound, checked before the GPU is touched
        cond = R.condition_numbers(im)
        print(f"condition numbers {shape}: {cond}")
        assert max(cond.values()) <= COND_MAX
    got = harvest.image_stats(up(x))
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (shape[0], 17)
    got = got.cpu().numpy()
    for k, name in enumerate(harvest.STAT_NAMES):
        if name in EXACT:
            print(f"{name} {shape}: {got[:, k]} (numpy {want[:, k]})")
            assert np.array_equal(got[:, k], want[:, k]), name
        else:
            e = np.abs(got[:, k] - want[:, k]) / np.abs(want[:, k])
            print(f"{name} {shape}: {got[:, k]} (numpy {want[:, k]}); relative {e.max():.2e}; bound {STATS_RTOL:.0e}")
            assert (e <= STATS_RTOL).all(), name
    n = shape[1] * shape[2]
    assert (want[:, 3] > 0).all() and (want[:, 2] < n).all()              # negatives and exact zeros are present


def test_median_ties_signed_zero_and_parity():
    parities = {s[1] * s[2] % 2 for s in SHAPES}
    assert parities == {0, 1}                                              # odd and even pixel counts
    x = raw((2, 70, 131)).copy()
    x[0, :40] = -0.0                                                       # the two middle values are zeros of either sign
    x[0, 40:, ::2] = 0.0
    x[1] = -np.abs(x[1]) - 1.0                                             # all negative
    got = harvest.image_stats(up(x)).cpu().numpy()
    col = harvest.STAT_NAMES.index("median")
    want = [np.median(im.astype(np.float64)) for im in x]
    print(f"median with signed zeros / all negative: {got[:, col]} (numpy {want})")
    assert got[0, col] == 0.0 and np.array_equal(got[:, col], want)
    assert np.array_equal(got[:, 2], [np.count_nonzero(im) for im in x]) and np.array_equal(got[:, 3], [np.count_nonzero(im < 0) for im in x])
    # an even count (66 x 70 = 4620: two chunks, the second ragged) whose lower middle value is negative and whose upper one is not:
    # the two keys' top bytes lie on either side of 0x80, so the middle ranks part at the first pass
    rng = np.random.default_rng(5)
    z = rng.permutation(np.concatenate([-rng.uniform(0.5, 900.0, 2310), rng.uniform(0.5, 900.0, 2310)])).astype(np.float32)
    lo, hi = np.sort(z)[2309:2311]
    assert lo < 0.0 <= hi and int(lo.view(np.uint32)) >> 31 == 1 and int(hi.view(np.uint32)) >> 31 == 0
    got = harvest.image_stats(up(z.reshape(1, 66, 70))).cpu().numpy()
    want = np.median(z.astype(np.float64))
    print(f"median with the middle values on either side of zero: {got[0, col]} (numpy {want})")
    assert got[0, col] == want


def test_estimate_noise_is_the_full_convolution_sum():
    x = raw((2, 70, 131))
    got = harvest.estimate_noise(up(x)).cpu().numpy()
    want = np.array([R.noise_sum(im) * np.sqrt(0.5 * np.pi) / (6.0 * 129 * 68) for im in x])
    print(f"noise {got} (numpy {want})")
    assert (np.abs(got - want) <= STATS_RTOL * want).all()
    assert got.shape == (2,)


# ---- scale01 --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_scale01(shape):
    x = raw(shape)
    y = harvest.scale01(up(x)).cpu().numpy()
    want = np.stack([R.scale01(im) for im in x])
    e = float(np.abs(y - want).max())
    print(f"scale01 {shape}: largest absolute distance {e:.2e}; bound {SCALE_ATOL:.1e}")
    assert e <= SCALE_ATOL and y.min() == 0.0 and y.max() == 1.0


def test_scale01_constant_image_is_one_half():
    x = np.stack([np.full((37, 53), 7.25, np.float32), raw((3, 37, 53))[0]])
    y = harvest.scale01(up(x)).cpu().numpy()
    assert np.array_equal(y[0], np.full((37, 53), 0.5, np.float32))
    assert np.abs(y[1] - R.scale01(x[1])).max() <= SCALE_ATOL


# ---- img_params -----------------------------------------------------------------------------------------------------------------

def test_img_params():
    img = raw((2, 70, 131))[1]
    S = 32
    x = up(img)
    stats, image = harvest.img_params(x, S)
    assert image.is_cuda and tuple(image.shape) == (S, S) and image.dtype == torch.float32
    small = harvest.box_resize(x, S)
    s_small = harvest.image_stats(small).cpu().numpy()[0]
    scaled = harvest.scale01(small)
    s_scaled = harvest.image_stats(scaled).cpu().numpy()[0]
    assert torch.equal(image, scaled)
    col = {n: i for i, n in enumerate(harvest.STAT_NAMES)}
    for k, v in harvest.FIELDS_2048.items():
        assert stats[k] == s_small[col[v]], k
    for k, v in harvest.FIELDS_0TO1.items():
        assert stats[k] == s_scaled[col[v]], k
    v64 = img.astype(np.float64)
    want = {"smallestDim": 70, "imageDims": (70, 131), "num_px": 70 * 131, "min": v64.min(), "max": v64.max(),
            "numberNonZero": np.count_nonzero(v64), "proportionZero": np.count_nonzero(v64) / (70 * 131),
            "numNegative": np.count_nonzero(v64 < 0), "proportionNegative": np.count_nonzero(v64 < 0) / (70 * 131)}
    for k, v in want.items():
        assert stats[k] == v, (k, stats[k], v)
    assert len(stats) == len(want) + len(harvest.FIELDS_2048) + len(harvest.FIELDS_0TO1)
    ref = R.box_resize(v64, S)
    ref = (ref - ref.min()) / (ref.max() - ref.min())
    e = rel_l2(image.cpu().numpy(), ref)
    print(f"img_params image: rel L2 {e:.3e}; bar {FACTOR * YARD_RESIZE + SCALE_ATOL:.3e}")
    assert e <= FACTOR * YARD_RESIZE + SCALE_ATOL
    assert torch.equal(harvest.img_params_lq(x, S), image)
    stack, table = harvest.harvest([img, raw((3, 37, 53))[0]], 16)
    assert isinstance(stack, np.ndarray) and stack.shape == (2, 16, 16, 1) and stack.dtype == np.float32 and len(table) == 2
    assert np.array_equal(stack[1, :, :, 0], harvest.img_params(raw((3, 37, 53))[0], 16)[1]) and table[1]["imageDims"] == (37, 53)


# ---- conventions, bits and safety -----------------------------------------------------------------------------------------------

def test_numpy_and_tensor_conventions():
    x4 = raw((2, 70, 131))[..., None]
    for a in (x4, x4[..., 0], x4[0, :, :, 0]):
        keep = a.copy()
        y, yt = harvest.box_resize(a, 32), harvest.box_resize(up(a), 32)
        want = (32, 32) if a.ndim == 2 else (2, 32, 32, 1) if a.ndim == 4 else (2, 32, 32)
        assert isinstance(y, np.ndarray) and y.dtype == np.float32 and y.shape == want and np.array_equal(a, keep)
        assert isinstance(yt, torch.Tensor) and tuple(yt.shape) == want and np.array_equal(y, yt.cpu().numpy())
        s, st = harvest.image_stats(a), harvest.image_stats(up(a))
        assert isinstance(s, np.ndarray) and s.dtype == np.float64 and s.shape == (1 if a.ndim == 2 else 2, 17)
        assert np.array_equal(s, st.cpu().numpy())
        z, zt = harvest.scale01(a), harvest.scale01(up(a))
        assert isinstance(z, np.ndarray) and z.shape == a.shape and z.dtype == np.float32 and np.array_equal(z, zt.cpu().numpy())
        n = harvest.estimate_noise(a)
        assert isinstance(n, np.ndarray) and n.shape == (s.shape[0],) and np.array_equal(n, s[:, 11])
    stats, image = harvest.img_params(x4[0, :, :, 0], 16)
    assert isinstance(image, np.ndarray) and image.shape == (16, 16) and isinstance(stats["mean2048"], float)


def test_bitwise_reproducible_and_independent_of_the_batch():
    x = up(raw((3, 37, 53)))
    run = lambda t: (harvest.box_resize(t, 16), harvest.image_stats(t), harvest.scale01(t))
    a, b = run(x), run(x)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    for i in range(3):
        one = run(x[i:i + 1].clone())                                      # alone = inside a batch of other images
        assert all(torch.equal(p[0], q[i]) for p, q in zip(one, a)), i
    assert not torch.isnan(a[1]).any()


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


def test_outputs_and_workspace_stay_inside_their_advertised_sizes():
    lib = _lib.load()
    st = _lib.stream_ptr()
    for (B, H, W), S in (((2, 70, 131), 32), ((3, 37, 53), 16), ((2, 3, 200), 8)):
        x = up(raw((B, H, W)))
        d = min(H, W)
        tab = torch.from_numpy(harvest.box_table(d, S)).to(dev())
        y = Guarded(B * S * S * 4)
        _lib.check(lib.emd_box_resize_f32(x.data_ptr(), H * W, W, B, d, y.ptr(), S, tab.data_ptr(), st), "resize")
        torch.cuda.synchronize()
        assert y.intact() and bool((y.view != SENTINEL).all())
        nbytes = lib.emd_image_stats_workspace_bytes(B, H, W)
        stats, ws = Guarded(B * 17 * 8), Guarded(nbytes)
        _lib.check(lib.emd_image_stats_f64(x.data_ptr(), B, H, W, stats.ptr(), ws.ptr(), nbytes, st), "stats")
        torch.cuda.synchronize()
        assert stats.intact(), "wrote outside [B][17]"
        assert ws.intact(), f"wrote outside its {nbytes}-byte workspace"
        got = stats.view.view(torch.float64).reshape(B, 17)
        assert torch.equal(got, harvest.image_stats(x))
        z = Guarded(B * H * W * 4)
        _lib.check(lib.emd_scale01_f32(x.data_ptr(), z.ptr(), B, H * W, stats.ptr(), st), "scale01")
        torch.cuda.synchronize()
        assert z.intact() and bool((z.view != SENTINEL).all())


def test_captured_in_one_graph_and_replayed_on_new_contents():
    x0, x1 = up(raw((2, 70, 131))), up(raw((2, 70, 131))[::-1].copy() * 0.5 + 0.25)
    run = lambda t: (harvest.box_resize(t, 32), harvest.image_stats(t), harvest.scale01(t))
    want0, want1 = run(x0), run(x1)                                        # eager (and warm: the table is on the device)
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
    print(f"resize: float32 restatement's largest {y:.3e}; bar {FACTOR * y:.3e}")
    for s in SHAPES:
        for im in raw(s):
            print(s, R.condition_numbers(im))
