"""GPU tests of the classical baseline filters (csrc/filters.hip, emdenoise.filters) against the float64
restatements of tests/filters_ref.py (scipy for Gaussian, median and Wiener; the formulas for bilateral and Chambolle).

The median is compared bit for bit.  For the others the tolerance is not a literal: the yardstick is the float32 restatement's own
relative L2 distance from the float64 one on the same inputs, and the bar of a filter is FACTOR = 4 times the LARGEST such distance
over every shape and setting used here (the HIP path sums in another order and uses the hardware exponential); the margin is the
one tests/test_metrics_gpu.py uses.  The noise power Wiener estimates is a scalar the kernels sum in double: it gets the same
factor over the float32 restatement's error with a floor of 1e-6 of its value (16 float32 roundings).  Every figure is printed
before it is asserted.

Measured on an MI355X (relative L2 against float64, the largest over the cases) beside the bars (4 x the float32 restatement's
largest distance from float64):
    Gaussian   7.3e-8   bar 3.0e-7
    bilateral  1.7e-7   bar 6.9e-7
    Wiener     3.9e-7   bar 1.4e-6
    Chambolle  5.1e-8   bar 2.0e-7
(DESIGN.md 3.16 has the table.)
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import emdenoise
from emdenoise import _lib, filters
from tests import filters_ref as R
from tests import ssim_ref
from tests.synth_inputs import synthetic_lq, synthetic_pair

pytestmark = pytest.mark.gpu

FACTOR = 4.0

# smaller than one tile with odd extents; across tile edges in both axes with a ragged last tile; exact tiles; and, per filter,
# the smallest extents its largest radius allows under the mirror border (added by shapes_for)
SHAPES = [(3, 37, 53), (2, 70, 131), (1, 128, 128)]
RADIUS = {"gaussian": 7, "median": 2, "bilateral": 4, "wiener": 4, "tv": 1}
GAUSS = [(3, 1.5), (11, 1.5), (15, 3.0)]                                     # (ksize, sigma)
BILATERAL = [(d, sc) for d in (3, 5, 9) for sc in (0.05, 0.5)]               # (d, sigma_color)
WIENER = [(k, n) for k in (3, 5, 9) for n in (None, 0.004)]                  # (ksize, noise)
TV = [(w, n) for w in (0.05, 0.3) for n in (1, 2, 30)]                       # (weight, n_iter)


def dev():
    return torch.device("cuda", 0)


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev())


def shapes_for(name):
    r = RADIUS[name]
    return SHAPES + [(1, r + 1, 200), (1, 200, r + 1)]


def sid(s):
    return "x".join(map(str, s))


@functools.lru_cache(maxsize=None)
def images(shape):
    """Seeded micrograph-like images in [0,1] of that shape plus one more image with a sharp noisy step, float32 [B+1,H,W]."""
    B, H, W = shape
    x = synthetic_lq(B, H, W, seed=900 + H + W)[..., 0]
    rng = np.random.default_rng(H * 1000 + W)
    step = np.full((H, W), 0.1, np.float32)
    step[:, W // 2:] = 0.9
    step += (0.02 * rng.standard_normal((H, W))).astype(np.float32)
    return np.concatenate([x, step[None]]).astype(np.float32)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


REF = {"gaussian": lambda x, c, dt: R.gaussian(x, sigma=c[1], ksize=c[0], dtype=dt),
       "bilateral": lambda x, c, dt: R.bilateral(x, d=c[0], sigma_color=c[1], sigma_space=1.5, dtype=dt),
       "wiener": lambda x, c, dt: R.wiener(x, ksize=c[0], noise=c[1], dtype=dt),
       "tv": lambda x, c, dt: R.tv_chambolle(x, weight=c[0], n_iter=c[1], dtype=dt)}
CASES = {"gaussian": GAUSS, "bilateral": BILATERAL, "wiener": WIENER, "tv": TV}
RUN = {"gaussian": lambda x, c: filters.gaussian(x, sigma=c[1], ksize=c[0]),
       "bilateral": lambda x, c: filters.bilateral(x, d=c[0], sigma_color=c[1], sigma_space=1.5),
       "wiener": lambda x, c: filters.wiener(x, ksize=c[0], noise=c[1]),
       "tv": lambda x, c: filters.tv_chambolle(x, weight=c[0], n_iter=c[1])}


@functools.lru_cache(maxsize=None)
def ref64(name, shape, case):
    return REF[name](images(shape), case, np.float64)


@functools.lru_cache(maxsize=None)
def two_noise_levels():
    """One clean image with little and with much noise added, float32 [2,70,131]: the local variance is the noise added here."""
    rng = np.random.default_rng(8)
    base = synthetic_pair(1, 70, 131, seed=31)[1][0, :, :, 0]
    return np.stack([base + 0.01 * rng.standard_normal(base.shape), base + 0.2 * rng.standard_normal(base.shape)]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def bar(name):
    """FACTOR x the largest float32-restatement error of that filter over every shape and setting of this file (for Wiener also the
    batch of two_noise_levels with the estimated noise)."""
    worst = 0.0
    if name == "wiener":
        x = two_noise_levels()
        worst = max(rel_l2(R.wiener(x, k, None, np.float32), R.wiener(x, k, None, np.float64)) for k in (3, 5, 9))
    for shape in shapes_for(name):
        for case in CASES[name]:
            worst = max(worst, rel_l2(REF[name](images(shape), case, np.float32), ref64(name, shape, case)))
    return FACTOR * worst


def check_against_oracle(name, shape, case):
    got = RUN[name](up(images(shape)), case)
    assert got.is_cuda and tuple(got.shape) == tuple(images(shape).shape)
    e = rel_l2(got.cpu().numpy(), ref64(name, shape, case))
    print(f"{name} {shape} {case}: rel L2 {e:.3e}; bar {bar(name):.3e} (float32 restatement's largest {bar(name) / FACTOR:.3e})")
    assert e <= bar(name), (name, shape, case, e, bar(name))


# ---- median: bit for bit -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ksize", [3, 5])
@pytest.mark.parametrize("shape", shapes_for("median"), ids=sid)
def test_median_is_bitwise_the_oracle(shape, ksize):
    x = images(shape)
    assert torch.equal(filters.median(up(x), ksize).cpu(), torch.from_numpy(R.median(x, ksize)))
    q = np.floor(x * 8.0).clip(0, 7).astype(np.float32) / 8.0            # 8 levels: windows full of exact ties
    assert len(np.unique(q)) <= 8
    assert torch.equal(filters.median(up(q), ksize).cpu(), torch.from_numpy(R.median(q, ksize)))
    c = np.full(shape, 0.625, np.float32)                                # a constant image
    assert torch.equal(filters.median(up(c), ksize).cpu(), torch.from_numpy(c))


# ---- the float filters against float64 ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", shapes_for("gaussian"), ids=sid)
def test_gaussian(shape):
    for case in GAUSS:
        check_against_oracle("gaussian", shape, case)


@pytest.mark.parametrize("shape", shapes_for("bilateral"), ids=sid)
def test_bilateral(shape):
    for case in BILATERAL:
        check_against_oracle("bilateral", shape, case)


@pytest.mark.parametrize("shape", shapes_for("wiener"), ids=sid)
def test_wiener(shape):
    for case in WIENER:
        check_against_oracle("wiener", shape, case)


@pytest.mark.parametrize("shape", shapes_for("tv"), ids=sid)
def test_tv_chambolle(shape):
    for case in TV:
        check_against_oracle("tv", shape, case)
    x = up(images(shape))
    assert torch.equal(filters.tv_chambolle(x, 0.1, 1), x)               # one iteration returns x, bit for bit


def test_wiener_estimates_the_noise_of_every_image_on_its_own():
    x = two_noise_levels()
    for k in (3, 5, 9):
        got, n = filters.wiener(up(x), ksize=k, return_noise=True)
        r64, n64 = R.wiener(x, k, None, np.float64, return_noise=True)
        r32, n32 = R.wiener(x, k, None, np.float32, return_noise=True)
        n = n.cpu().numpy().astype(np.float64)
        assert n.shape == (2,) and n[1] > 10 * n[0]
        for b in range(2):
            bound = max(FACTOR * abs(float(n32[b]) - n64[b]), 1e-6 * n64[b])
            print(f"wiener k={k} image {b}: noise {n[b]:.6e} (float64 {n64[b]:.6e}); error {abs(n[b] - n64[b]):.3e}; bound {bound:.3e}")
            assert abs(n[b] - n64[b]) <= bound
        e, y = rel_l2(got.cpu().numpy(), r64), rel_l2(r32, r64)
        print(f"wiener k={k} two noise levels: rel L2 {e:.3e}; float32 restatement {y:.3e}; bar {bar('wiener'):.3e}")
        assert e <= bar("wiener")
        # a given noise power comes back as given
        _, n_given = filters.wiener(up(x), ksize=k, noise=0.003, return_noise=True)
        assert torch.equal(n_given.cpu(), torch.full((2,), 0.003, dtype=torch.float32))


def test_wiener_on_a_constant_image():
    """v = 0 and n = 0 is scipy's 0 / 0: here the mean -- the constant wherever the window lies inside the image -- and finite
    everywhere, for a given n = 0 and for the estimated n."""
    c = np.full((1, 40, 70), 0.3, np.float32)
    for k in (3, 9):
        r = k // 2
        for noise in (0.0, None):
            y = filters.wiener(up(c), ksize=k, noise=noise).cpu().numpy()
            assert np.isfinite(y).all()
            assert np.array_equal(y[:, r:-r, r:-r], c[:, r:-r, r:-r])


# ---- borders ---------------------------------------------------------------------------------------------------------------

def test_borders_agree_with_a_padded_image():
    """The output on [1,70,131] is the output on the same image embedded in a larger (mirror- or zero-) padded image, cropped
    back: other tile positions, the same pixels, so the same bits -- for the mirror filters and for Wiener (zero padding, a given
    noise power: an estimated one is a mean over the other image)."""
    x = images((2, 70, 131))[:1]
    P, Q = 9, 13                                                              # pad by more than the largest radius, off the tile grid
    crop = lambda t: t[:, P:P + 70, Q:Q + 131]
    mir = np.pad(x, ((0, 0), (P, P), (Q, Q)), mode="reflect")
    for name, fn in (("gaussian 3", lambda a: filters.gaussian(a, 1.5, 3)), ("gaussian 15", lambda a: filters.gaussian(a, 3.0, 15)),
                     ("median 3", lambda a: filters.median(a, 3)), ("median 5", lambda a: filters.median(a, 5)),
                     ("bilateral 9", lambda a: filters.bilateral(a, 9, 0.1, 1.5)), ("bilateral 3", lambda a: filters.bilateral(a, 3, 0.5, 1.5))):
        assert torch.equal(fn(up(x)), crop(fn(up(mir)))), name
    zer = np.pad(x, ((0, 0), (P, P), (Q, Q)))
    for k in (3, 5, 9):
        assert torch.equal(filters.wiener(up(x), k, noise=0.004), crop(filters.wiener(up(zer), k, noise=0.004))), f"wiener {k}"


# ---- guard regions: exactly the advertised sizes -----------------------------------------------------------------------------

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
    x = up(images((B - 1, H, W)))
    assert x.shape == (B, H, W)
    st = _lib.stream_ptr()
    taps = filters.gaussian_taps(15, 3.0)
    wb, tb = lib.emd_filter_wiener_workspace_bytes(B, H, W), lib.emd_filter_tv_workspace_bytes(B, H, W)
    calls = {
        "gaussian": (0, lambda o, w: lib.emd_filter_gaussian_f32(x.data_ptr(), o, B, H, W, taps.ctypes.data_as(C.c_void_p), 15, st)),
        "median": (0, lambda o, w: lib.emd_filter_median_f32(x.data_ptr(), o, B, H, W, 5, st)),
        "bilateral": (0, lambda o, w: lib.emd_filter_bilateral_f32(x.data_ptr(), o, B, H, W, 9, C.c_float(0.1), C.c_float(1.5), st)),
        "wiener": (wb, lambda o, w: lib.emd_filter_wiener_f32(x.data_ptr(), o, B, H, W, 9, C.c_float(-1.0), None, w, wb, st)),
        "tv": (tb, lambda o, w: lib.emd_filter_tv_f32(x.data_ptr(), o, B, H, W, C.c_float(0.1), 5, w, tb, st)),
    }
    for name, (ws_bytes, call) in calls.items():
        out, ws = Guarded(B * H * W * 4), Guarded(max(ws_bytes, 4))
        _lib.check(call(out.ptr(), ws.ptr()), name)
        torch.cuda.synchronize()
        assert out.intact(), f"{name}: wrote outside out"
        assert ws.intact(), f"{name}: wrote outside its {ws_bytes}-byte workspace"
        assert bool((out.view != SENTINEL).all()), f"{name}: left output pixels unwritten"


# ---- reproducibility, capture, conventions -----------------------------------------------------------------------------------

def test_bitwise_reproducible():
    x = up(images((2, 70, 131)))
    a, na = filters.wiener(x, 5, return_noise=True)
    b, nb = filters.wiener(x, 5, return_noise=True)
    assert torch.equal(a, b) and torch.equal(na, nb)
    assert torch.equal(filters.tv_chambolle(x, 0.1, 30), filters.tv_chambolle(x, 0.1, 30))


def test_captured_in_one_graph_and_replayed_on_new_contents():
    x0, x1 = up(images((2, 70, 131))), up(images((2, 70, 131))[::-1].copy() * 0.5 + 0.25)
    run = lambda t: (filters.gaussian(t, 1.5, 11), filters.wiener(t, 5), filters.tv_chambolle(t, 0.1, 4))
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


def test_numpy_and_tensor_conventions():
    x4 = synthetic_lq(2, 24, 40, seed=1)                                   # [B,H,W,1]
    for fn in (filters.gaussian, filters.median, filters.bilateral, filters.wiener, filters.tv_chambolle):
        for a in (x4, x4[..., 0], x4[0, :, :, 0]):
            keep = a.copy()
            y = fn(a)
            assert isinstance(y, np.ndarray) and y.shape == a.shape and y.dtype == np.float32, fn.__name__
            assert np.array_equal(a, keep)
            t = up(a)
            tkeep = t.clone()
            yt = fn(t)
            assert isinstance(yt, torch.Tensor) and yt.device == t.device and yt.shape == t.shape, fn.__name__
            assert torch.equal(t, tkeep)
            assert np.array_equal(yt.cpu().numpy(), y)                     # the same bits either way
    y, n = filters.wiener(x4, return_noise=True)
    assert isinstance(n, np.ndarray) and n.shape == (2,)


# ---- the comparison table ----------------------------------------------------------------------------------------------------

def test_baseline_table():
    from emdenoise.input_pipeline import DeviceRecordParser

    hq = up(synthetic_lq(4, 64, 64, seed=77) * 200.0 + 5.0)
    lq, truth = DeviceRecordParser(dev(), seed=3)(hq)                      # Poisson LQ / truth pairs [4,64,64,1]
    assert lq.shape == (4, 64, 64, 1) and truth.shape == lq.shape
    k = emdenoise.Micrograph_Autoencoder(depth=2, width=3)                 # initial parameters
    data, labels = emdenoise.baseline_table(lq, truth, extra={"K": k.denoise_batch})
    assert labels == ["Unfiltered", "Gaussian", "Bilateral", "Median", "Wiener", "Chambolle", "K"]
    assert data.is_cuda and data.dtype == torch.float32 and data.shape == (4, 7, 2)
    d = data.cpu().numpy().astype(np.float64)
    lqn, tn = lq.cpu().numpy(), truth.cpu().numpy()
    # row 0: the input itself, by numpy and the float64 restatement of tf_ssim; the bars are the metrics' own
    # (tests/test_metrics_gpu.py: FACTOR x the float32 restatement's error, floor 1e-6)
    mse64 = ((lqn.astype(np.float64) - tn) ** 2).mean(axis=(1, 2, 3))
    mse32 = ((lqn - tn) ** 2).mean(axis=(1, 2, 3), dtype=np.float32)
    s64 = ssim_ref.ssim(lqn, tn, torch.float64)["means"][:, 0]
    s32 = ssim_ref.ssim(lqn, tn, torch.float32)["means"][:, 0]
    for name, got, r64, r32 in (("mse", d[:, 0, 0], mse64, mse32), ("ssim", d[:, 0, 1], s64, s32)):
        e, y = np.max(np.abs(got - r64)), np.max(np.abs(np.asarray(r32, np.float64) - r64))
        print(f"baseline_table row 0 {name}: abs error {e:.3e}; float32 restatement {y:.3e}; bound {max(FACTOR * y, 1e-6):.3e}")
        assert e <= max(FACTOR * y, 1e-6)
    # every row: the scores of that method's own output, the same device reductions -> the same bits
    outs = [lq, filters.gaussian(lq), filters.bilateral(lq), filters.median(lq), filters.wiener(lq), filters.tv_chambolle(lq),
            k.denoise_batch(lq)]
    for m, y in enumerate(outs):
        _, mse = emdenoise.psnr(y, truth, per_image=True, return_mse=True)
        assert torch.equal(data[:, m, 0], mse) and torch.equal(data[:, m, 1], emdenoise.ssim(y, truth, per_image=True)), labels[m]
    assert len({tuple(np.round(d[:, m, 0], 9)) for m in range(7)}) == 7    # seven different methods
    # clip=True scores the clipped outputs; numpy in -> numpy out with the same numbers
    clipped, _ = emdenoise.baseline_table(lq, truth, clip=True)
    y = filters.wiener(lq).clamp(0.0, 1.0)
    assert torch.equal(clipped[:, 4, 1], emdenoise.ssim(y, truth, per_image=True))
    dn, ln = emdenoise.baseline_table(lqn, tn)
    assert isinstance(dn, np.ndarray) and dn.shape == (4, 6, 2) and ln == labels[:6]
    assert np.array_equal(dn, data[:, :6].cpu().numpy())
