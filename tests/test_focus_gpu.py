"""GPU tests of emdenoise.focus (csrc/focus.hip) against the restatement of tests/focus_ref.py.

Shapes: the tile is 64 columns x 32 rows, so 2 x 2, 3 x 3 and 5 x 7 are all halo, 17 x 33 and 40 x 70 have ragged tiles both ways,
64 x 129 has one column and 130 x 70 two rows past a tile edge, and 3 x 16400 has 257 tiles: the second-stage sum over the tiles' partials (256 threads)
makes more than one trip (a long strip, because a larger image of continuous values cannot keep every one of its pixels 1e-6 away
from the mean, which the moments' test asserts).  Inputs: Poisson counts (integers: the float32 Laplacian is exact) and Gaussian floats.

The bars are not derived from the device's output.  ``laplacian``, ``n``, histogram counts, ``index`` and ``zbest`` are exact.  The
other moment columns: relative distance from the restatement with exact (``math.fsum``) sums <= 4 x the relative distance between
that and the same restatement with numpy's pairwise sums, with a floor of H W 2^-53.  The entropy: bins / 4 x 2^-53 relative to
``scipy.stats.entropy`` of the device's own counts.  The spline's curve: 4 x the distance between InterpolatedUnivariateSpline and
CubicSpline(not-a-knot), with a floor of N 2^-52 of the curve's largest magnitude.  Every figure is printed before it is asserted."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.interpolate
import scipy.stats
import torch

from emdenoise import _lib, focus
from tests import focus_ref as R
from tests.guarded import assert_written, guarded

pytestmark = pytest.mark.gpu

SMALL = [(2, 2), (3, 3), (5, 7), (17, 33), (40, 70), (64, 129), (130, 70)]
MANY_TILES = (3, 16400)           # 257 tiles
# seeds moved on where an input put a Laplacian value within 1e-6 max|L| of the mean (the condition the moments' test asserts)
BUMP = {("poisson", 5, 2, 2): 5, ("gauss", 5, 130, 70): 4, ("gauss", 2, 3, 16400): 3}
SHAPES = SMALL + [MANY_TILES]
KINDS = ["poisson", "gauss"]
U = 2.0 ** -53


def dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def images(kind, B, H, W):
    rng = np.random.default_rng(1000 * H + W + (7 if kind == "gauss" else 0) + 100003 * BUMP.get((kind, B, H, W), 0))
    if kind == "poisson":
        x = rng.poisson(20.0, (B, H, W)).astype(np.float32)
    else:
        x = (3.0 * rng.standard_normal((B, H, W)) + 1.0).astype(np.float32)
    x.setflags(write=False)                                                 # shared: nobody writes it
    return x


@functools.lru_cache(maxsize=None)
def ref_moments(kind, B, H, W, ksize, rectify, exact):
    return R.laplacian_moments(images(kind, B, H, W), ksize, rectify, exact)


def rel(a, b):
    """|a - b| / |b| per element; 0 where both are equal (two zeros, two NaNs)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    with np.errstate(all="ignore"):
        return np.where(same, 0.0, np.abs(a - b) / np.abs(b))


def batch_of(shape):
    return 2 if shape == MANY_TILES else 5


# ---- laplacian -------------------------------------------------------------------------------------------------------------------
def laplacian_c(x, ksize):
    B, H, W = x.shape
    xin, gx = guarded(x.size, torch.float32, dev(), fill=np.array(x), name="x")
    out, gy = guarded(x.size, torch.float32, dev(), name="y")
    _lib.check(_lib.load().emd_laplacian_f32(C.c_void_p(xin.data_ptr()), B, H, W, ksize, C.c_void_p(out.data_ptr()),
                                             _lib.stream_ptr()), "emd_laplacian_f32")
    torch.cuda.synchronize()
    gx()
    gy()
    assert_written(out)
    assert np.array_equal(xin.cpu().numpy().view(np.int32), np.ascontiguousarray(x).ravel().view(np.int32)), "the input was written"
    return out.view(B, H, W).cpu().numpy()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_laplacian_bitwise(shape, kind):
    for B in (1, batch_of(shape)):
        x = images(kind, B, *shape)
        for ksize in (1, 3):
            got, want = laplacian_c(x, ksize), R.laplacian(x, ksize)
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), (B, ksize, int((got != want).sum()))


def test_laplacian_by_hand_and_wrapper_shapes():
    for x, k1, k3 in ((R.HAND_2X2, R.HAND_2X2_K1, R.HAND_2X2_K3), (R.HAND_3X3, R.HAND_3X3_K1, R.HAND_3X3_K3)):
        assert np.array_equal(focus.laplacian(x, 1), k1) and np.array_equal(focus.laplacian(x, 3), k3)
    x = images("gauss", 5, 17, 33)
    y = focus.laplacian(torch.from_numpy(np.array(x)).to(dev()))
    assert y.is_cuda and tuple(y.shape) == x.shape and np.array_equal(y.cpu().numpy(), R.laplacian(x, 1))
    assert focus.laplacian(x[0], 3).shape == x[0].shape


# ---- moments ---------------------------------------------------------------------------------------------------------------------
def moments_c(x, ksize, rectify):
    B, H, W = x.shape
    lib = _lib.load()
    need = lib.emd_laplacian_moments_workspace_bytes(B, H, W)
    xin, gx = guarded(x.size, torch.float32, dev(), fill=np.array(x), name="x")
    out, go = guarded(B * focus.NMOMENTS, torch.float64, dev(), name="out")
    ws, gw = guarded(need // 8, torch.float64, dev(), name="workspace")
    _lib.check(lib.emd_laplacian_moments_f64(C.c_void_p(xin.data_ptr()), B, H, W, ksize, int(rectify), C.c_void_p(out.data_ptr()),
                                             C.c_void_p(ws.data_ptr()), need, _lib.stream_ptr()), "emd_laplacian_moments_f64")
    torch.cuda.synchronize()
    gx()
    go()
    gw()
    assert_written(out)
    return out.view(B, focus.NMOMENTS).cpu().numpy()


@pytest.mark.parametrize("rectify", [True, False], ids=["rectified", "all"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_moments_against_the_exact_restatement(shape, kind, rectify):
    H, W = shape
    B = batch_of(shape)
    x = images(kind, B, H, W)
    for ksize in (1, 3):
        want, margin = ref_moments(kind, B, H, W, ksize, rectify, True)
        pairwise, _ = ref_moments(kind, B, H, W, ksize, rectify, False)
        print(f"{H}x{W} {kind} ksize {ksize} rectify {rectify}: membership margin {margin:.3e} of max|L|")
        assert margin > 1e-6, "a Laplacian value lies within 1e-6 max|L| of the mean: change the seed"
        assert np.array_equal(want[:, 1], pairwise[:, 1])
        got = moments_c(x, ksize, rectify)
        yard, dist = rel(pairwise, want), rel(got, want)
        bar = np.maximum(4.0 * yard, H * W * U)
        for col, name in enumerate(focus.MOMENT_NAMES):
            print(f"  {name:15s} device {dist[:, col].max():.3e}  pairwise {yard[:, col].max():.3e}  bar {bar[:, col].min():.3e}")
        assert np.array_equal(got[:, 1], want[:, 1]), "n"
        assert np.all(dist <= bar), (dist / bar).max()
        # row b of a batch is the same image run alone
        alone = moments_c(x[B - 1:B], ksize, rectify)
        assert np.array_equal(alone.view(np.int64), got[B - 1:B].view(np.int64))


@pytest.mark.parametrize("rectify", [True, False])
def test_moments_of_a_constant_image(rectify):
    x = np.full((2, 40, 70), 3.25, np.float32)
    for ksize in (1, 3):
        got = focus.laplacian_moments(x, ksize, rectify)
        assert got.shape == (2, 6) and np.all(got[:, 0] == 0) and np.all(got[:, 1] == 40 * 70) and np.all(got[:, 2] == 0)
        assert np.all(got[:, 3] == 0) and np.all(got[:, 4] == 0) and np.all(np.isnan(got[:, 5]))


def test_fresnel_quantifier_is_column_5_and_scipys_kurtosis():
    x = images("gauss", 5, 40, 70)
    xd = torch.from_numpy(np.array(x)).to(dev())
    for rectify in (True, False):
        m = focus.laplacian_moments(xd, 3, rectify)
        k = focus.fresnel_quantifier(xd, rectify)
        assert k.is_cuda and k.dtype == torch.float64 and torch.equal(k, m[:, 5])
        assert np.array_equal(focus.fresnel_quantifier(x, rectify), k.cpu().numpy())
        for b in range(5):
            flat = R.laplacian(x[b], 3).ravel().astype(np.float64)
            want = scipy.stats.kurtosis(flat[flat >= flat.mean()] if rectify else flat)
            assert abs(float(k[b]) - want) <= 1e-11 * abs(want)


# ---- histogram and entropy -------------------------------------------------------------------------------------------------------
def histogram_c(x, bins, normalize):
    B, H, W = x.shape
    lib = _lib.load()
    need = lib.emd_histogram01_workspace_bytes(B, H, W, int(normalize))
    xin, gx = guarded(x.size, torch.float32, dev(), fill=np.array(x), name="x")
    counts = torch.full((B * bins + 2,), -77, dtype=torch.int64, device=dev())   # one sentinel word on either side
    ws, gw = guarded(max(need // 8, 1), torch.float64, dev(), name="workspace")
    _lib.check(lib.emd_histogram01_i64(C.c_void_p(xin.data_ptr()), B, H, W, bins, int(normalize), C.c_void_p(counts.data_ptr() + 8),
                                       C.c_void_p(ws.data_ptr()), need, _lib.stream_ptr()), "emd_histogram01_i64")
    torch.cuda.synchronize()
    gx()
    gw()
    c = counts.cpu().numpy()
    assert c[0] == -77 and c[-1] == -77, "counts: a word outside the output was written"
    return c[1:-1].reshape(B, bins)


def with_edges(shape, bins, seed):
    """Uniform values over [-0.2, 1.2] with the edge values at the start of every image."""
    B, H, W = shape
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.2, 1.2, (B, H * W)).astype(np.float32)
    one = np.float32(1)
    e = [0.0, 1.0, one - np.float32(2.0 ** -24), np.nextafter(one, np.float32(2)), -0.0, -1e-30, -0.25, 1.5, np.nan, np.inf, -np.inf]
    e += [k / bins for k in range(0, bins + 1, max(1, bins // 32))]
    e = np.array(e, np.float32)[: H * W]
    x[:, : e.size] = e
    return x.reshape(B, H, W)


@pytest.mark.parametrize("bins", [2, 256, 4096])
@pytest.mark.parametrize("shape", [(1, 5, 7), (5, 40, 70), (2, 200, 331)], ids=lambda s: "x".join(map(str, s)))
def test_histogram_equals_numpy(shape, bins):                # 200 x 331 = 66200 pixels: three workgroups per image, the last ragged
    x = with_edges(shape, bins, seed=bins + shape[1])
    got = histogram_c(x, bins, False)
    for b in range(shape[0]):
        v = x[b].ravel()
        want = np.histogram(v[np.isfinite(v)], bins, range=(0, 1))[0]
        assert np.array_equal(got[b], want), (b, np.nonzero(got[b] != want)[0][:8])
        assert np.array_equal(got[b], R.histogram01(v, bins))
    assert np.array_equal(focus.histogram01(x, bins), got)


@pytest.mark.parametrize("bins", [2, 256, 4096])
@pytest.mark.parametrize("case", [("gauss", 5, 40, 70), ("poisson", 1, 17, 33), ("gauss", 2, 515, 1030)], ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}x{c[3]}")
def test_histogram_normalized_equals_the_float64_restatement(case, bins):
    x = images(*case)
    got = histogram_c(x, bins, True)
    for b in range(x.shape[0]):
        t = R.normalized(x[b])
        frac = np.abs(t * bins - np.rint(t * bins))
        print(f"{case} bins {bins} image {b}: least distance of t bins from an integer {frac.min():.3e}")
        assert frac.min() > 1e-9, "a value sits on a bin edge to within rounding: change the seed"
        assert np.array_equal(got[b], R.histogram01(t, bins))
        assert got[b].sum() == np.count_nonzero((t >= 0) & (t <= 1))
    assert np.array_equal(focus.histogram01(x, bins, normalize=True), got)


def test_histogram_normalized_second_stage_makes_two_trips():
    """2050 x 4100 pixels are 257 chunks of 32768: the sum over the chunks' partials (256 threads) wraps round."""
    rng = np.random.default_rng(77)
    x = (2.0 * rng.standard_normal((1, 2050, 4100)) - 5.0).astype(np.float32)
    t = R.normalized(x[0])
    frac = np.abs(t * 256 - np.rint(t * 256))
    print(f"least distance of t bins from an integer {frac.min():.3e}")
    assert frac.min() > 1e-9
    xd = torch.from_numpy(x).to(dev())
    assert np.array_equal(focus.histogram01(xd, 256, normalize=True).cpu().numpy()[0], R.histogram01(t, 256))
    v = x[0].ravel()
    assert np.array_equal(focus.histogram01(xd, 256).cpu().numpy()[0], np.histogram(v, 256, range=(0, 1))[0])


@pytest.mark.parametrize("bins", [64, 256, 4096])
def test_image_entropy_against_scipy_on_the_devices_counts(bins):
    x = np.concatenate([with_edges((3, 40, 70), bins, seed=5), 0.5 + 0.1 * images("gauss", 2, 40, 70)]).astype(np.float32)
    xd = torch.from_numpy(x).to(dev())
    for normalize in (False, True):
        for eps in (1e-6, 0.5):
            counts = focus.histogram01(xd, bins, normalize).cpu().numpy()
            got = focus.image_entropy(xd, bins, eps, normalize)
            assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (5,)
            got = got.cpu().numpy()
            want = np.array([scipy.stats.entropy(c + eps, base=2) for c in counts])
            d = rel(got, want)
            print(f"bins {bins} normalize {normalize} eps {eps}: {d.max():.3e} (bar {bins / 4 * U:.3e}); entropy {want}")
            assert np.all(d <= bins / 4 * U)
            assert np.array_equal(focus.image_entropy(x, bins, eps, normalize), got)
    # the reference's call: 256 bins whatever num_bins says -- here num_bins counts
    assert not np.array_equal(focus.image_entropy(x, 64), focus.image_entropy(x, 256))


# ---- the spline ------------------------------------------------------------------------------------------------------------------
def knots(N, uniform):
    rng = np.random.default_rng(40 + N)
    return np.linspace(-3.0, 5.0, N) if uniform else np.cumsum(rng.uniform(0.2, 1.7, N)) - 4.0


def series(N, uniform, B):
    z = knots(N, uniform)
    rng = np.random.default_rng(N + 100 * B + uniform)
    centre = rng.uniform(z[0], z[-1], (B, 1))
    return z, 0.3 * (z[None, :] - centre) ** 2 + 0.4 * rng.standard_normal((B, N)) + 2.0


def spline_c(z, s, interp_factor):
    B, N = s.shape
    G = interp_factor * N
    zd = torch.from_numpy(z).to(dev())
    sd = torch.from_numpy(s).to(dev())
    zbest, g1 = guarded(B, torch.float64, dev(), name="zbest")
    curve, g2 = guarded(B * G, torch.float64, dev(), name="curve")
    index = torch.full((B + 2,), -77, dtype=torch.int64, device=dev())
    _lib.check(_lib.load().emd_spline_argmin_f64(C.c_void_p(zd.data_ptr()), C.c_void_p(sd.data_ptr()), B, N, interp_factor,
                                                 C.c_void_p(zbest.data_ptr()), C.c_void_p(curve.data_ptr()),
                                                 C.c_void_p(index.data_ptr() + 8), _lib.stream_ptr()), "emd_spline_argmin_f64")
    torch.cuda.synchronize()
    g1()
    g2()
    assert_written(zbest)
    assert_written(curve)
    i = index.cpu().numpy()
    assert i[0] == -77 and i[-1] == -77
    return zbest.cpu().numpy(), curve.view(B, G).cpu().numpy(), i[1:-1]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "nonuniform"])
@pytest.mark.parametrize("N", [4, 5, 21, 64])
def test_optimal_focus_against_scipy(N, uniform, B):
    z, s = series(N, uniform, B)
    for factor in (10, 3):
        zbest, curve, index = spline_c(z, s, factor)
        g = R.grid(z, factor)
        for b in range(B):
            ius = scipy.interpolate.InterpolatedUnivariateSpline(z, s[b])(g)
            cs = scipy.interpolate.CubicSpline(z, s[b], bc_type="not-a-knot")(g)
            top = np.abs(ius).max()
            yard, dist = np.abs(cs - ius).max() / top, np.abs(curve[b] - ius).max() / top
            bar = max(4.0 * yard, N * 2.0 ** -52)
            print(f"N {N} uniform {uniform} series {b} factor {factor}: device {dist:.3e}  CubicSpline {yard:.3e}  bar {bar:.3e}")
            assert dist <= bar
            two = np.sort(ius)[:2]
            assert two[1] - two[0] > 1e-9 * (ius.max() - ius.min()), "the reference's minimum is not unique enough: change the seed"
            assert index[b] == int(np.argmin(ius))
            assert zbest[b].view(np.int64) == g[index[b]].view(np.int64)
    # the wrapper: the same numbers, numpy and device, one series and several
    zb, cv, ix = focus.optimal_focus(z, s, 3, return_curve=True)
    assert np.array_equal(zb, zbest) and np.array_equal(cv, curve) and np.array_equal(ix, index)
    one = focus.optimal_focus(torch.from_numpy(z).to(dev()), torch.from_numpy(s[0]).to(dev()), 3)
    assert one.is_cuda and one.dim() == 0 and float(one) == zbest[0]


@pytest.mark.parametrize("N", [4, 9])
def test_optimal_focus_returns_the_end_points(N):
    z = knots(N, False)
    rising = 2.0 + (z - z[0]) + 0.1 * (z - z[0]) ** 2                         # a cubic spline reproduces a quadratic
    s = np.stack([rising, rising[::-1].copy(), -rising])
    zbest, curve, index = spline_c(z, s, 10)
    assert zbest[0] == z[0] and index[0] == 0
    assert index[1] == 10 * N - 1 and zbest[1] == z[-1] and index[2] == 10 * N - 1 and zbest[2] == z[-1]


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def test_autofocus_end_to_end_and_in_a_graph():
    stack, z = R.focal_series(9, 64, z0=0.3, seed=13)
    other, _ = R.focal_series(9, 64, z0=-0.9, seed=14)
    sd, od, zd = torch.from_numpy(stack).to(dev()), torch.from_numpy(other).to(dev()), torch.from_numpy(z).to(dev())
    want = {}
    for name, xd in (("first", sd), ("second", od)):
        zbest, scores = focus.autofocus(xd, zd)
        assert zbest.is_cuda and zbest.dim() == 0 and tuple(scores.shape) == (9,)
        assert torch.equal(scores, focus.fresnel_quantifier(xd))
        sc = scores.cpu().numpy()
        ref_z, ref_curve, ref_i = R.optimal_focus(z, sc, 10, scipy.interpolate.InterpolatedUnivariateSpline)
        two = np.sort(ref_curve)[:2]
        assert two[1] - two[0] > 1e-9 * (ref_curve.max() - ref_curve.min())
        print(f"{name}: scores {sc}, zbest {float(zbest)} (restatement {ref_z}, grid point {ref_i})")
        assert np.float64(float(zbest)).view(np.int64) == np.float64(ref_z).view(np.int64)
        want[name] = (zbest.clone(), scores.clone())
    zn, sn = focus.autofocus(stack, z)                                        # numpy in, numpy out
    assert np.array_equal(zn, want["first"][0].cpu().numpy()) and np.array_equal(sn, want["first"][1].cpu().numpy())
    assert float(want["first"][0]) != float(want["second"][0])

    static = sd.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        focus.autofocus(static, zd)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gz, gs = focus.autofocus(static, zd)
    static.copy_(od)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(gz, want["second"][0]) and torch.equal(gs, want["second"][1])
    static.copy_(sd)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(gz, want["first"][0]) and torch.equal(gs, want["first"][1])
