"""GPU tests of the affine registration by mutual information and of the warp (csrc/affine.hip, emdenoise.affine)
against the float64 numpy restatement of tests/affine_ref.py.  MATLAB is not available: nothing is compared with it, the formulas of
include/emdenoise.h are the specification.

What is compared how.  The bars are not derived from the device's output.

* Warps, sample indices, histograms, chained transforms, limits, and the optimizer's x and A under teacher forcing: bit for bit.  They
  go through correctly rounded operations only, one at a time, or are sums of integers.
* MI: absolute; the bar is FACTOR = 4 times YARD_MI, the LARGEST distance, over the metric cases of this file, between two float64
  evaluations of the same integer histogram: the header's (one accumulator in row-major order, P log(P / (pf pm))) and
  P (log P - log pf - log pm) under numpy's pairwise sum; with a floor of bins^2 2^-53 max(1, MI) for the bins^2 rounded terms.
  ``python -m tests.test_affine_gpu`` computes YARD_MI on the CPU.
* Normals: 8 ulps of the largest possible |z| = sqrt(-2 ln 2^-33) = 6.77: 7.2e-15 absolute (three chained library functions).
* Decisions: wherever the device's accepted count is held to the restatement's, the restatement's decision margins |MI - f| / f are
  asserted on the CPU first to be >= 1e-9, seven orders above the MI bar.

An integer translation is a bitwise shifted copy only while u h returns to the integer it came from: where h = max(H, W) / 2 is no
power of two the product can miss by an ulp, and a coordinate that should be W exactly then lands an ulp inside the image (33 x 47,
shift (-1, 2): one border column reads 5e-15 of its neighbour instead of the fill).  That is the arithmetic the header specifies; the
translation used here, (3, -2), is one for which the restatement, asserted first, is the shifted copy at all four shapes.

Every figure is printed before it is asserted."""
import functools

import numpy as np
import pytest
import torch

from emdenoise import _lib, affine
from tests import affine_ref as R
from tests.synth_inputs import synthetic_lq
from tests.test_exitwave_gpu import Guarded, SENTINEL, dev, up

pytestmark = pytest.mark.gpu

FACTOR = 4.0
YARD_MI = 1.6e-15                                            # python -m tests.test_affine_gpu, rounded up
NORMAL_BAR = 7.2e-15
MARGIN_MIN = 1e-9
WARP_SHAPES = [(2, 8, 8), (3, 24, 40), (1, 33, 47), (1, 64, 64)]
SHIFT = (3, -2)


def mi_bar(bins, mi):
    return max(FACTOR * YARD_MI, bins * bins * 2.0 ** -53 * max(1.0, abs(mi)))


@functools.lru_cache(maxsize=None)
def images(N, H, W, seed=0):
    """Broadband float32 images in [0.5, 1.5).  Cached: do not write into the result."""
    return np.random.default_rng(1000 * seed + 7 * H + W).random((N, H, W), dtype=np.float32) + np.float32(0.5)


@functools.lru_cache(maxsize=None)
def smooth(H, W, seed=0):
    """A smooth float32 image in [0, 1] with noise on it: mutual information has something to find.  Cached."""
    S = max(H, W)
    return synthetic_lq(1, S, S, seed=2200 + seed)[0, :H, :W, 0].copy()


def rot(H, W, angle=2.0, scale=1.02, shift=(0.0, 0.0)):
    return R.similarity(angle, scale, shift, H, W)


# ---- the warp -----------------------------------------------------------------------------------------------------------------------

def c_warp(x, T, shared, fill):
    """The C call on a guarded output."""
    N, H, W = x.shape
    out = Guarded(N * H * W * 4)
    t = up(np.asarray(T, np.float64))
    _lib.check(_lib.load().emd_warp_affine_f32(x.data_ptr(), N, H, W, t.data_ptr(), int(shared), float(fill), out.ptr(), _lib.stream_ptr()),
               "emd_warp_affine_f32")
    torch.cuda.synchronize()
    assert out.intact(), "wrote outside the output"
    return out.view.reshape(N, H, W).cpu().numpy()


@pytest.mark.parametrize("shape", WARP_SHAPES, ids=str)
def test_warp(shape):
    N, H, W = shape
    x = images(N, H, W)
    xd = up(x)
    h = max(H, W) / 2
    eye = np.stack([R.identity()] * N)
    assert np.array_equal(c_warp(xd, eye, False, 0.0), x)                   # the identity: a bitwise copy
    dx, dy = SHIFT
    Ts = np.array([[1, 0, dx / h], [0, 1, dy / h]], np.float64)
    for fill in (0.0, 0.25):
        want = np.full_like(x, fill)
        want[:, max(0, -dy):min(H, H - dy), max(0, -dx):min(W, W - dx)] = x[:, max(0, dy):min(H, H + dy), max(0, dx):min(W, W + dx)]
        assert np.array_equal(R.warp(x, Ts, fill), want)                    # the restatement first
        assert np.array_equal(c_warp(xd, Ts, True, fill), want)             # an integer translation: a bitwise shifted copy
    Tr = np.stack([rot(H, W, 2.0 + n, 1.02, (0.7 * n, -0.4)) for n in range(N)])
    want = R.warp(x, Tr, 0.25)
    got = c_warp(xd, Tr, False, 0.25)
    assert (want == np.float32(0.25)).any() or H * W <= 64                  # the rotated frame leaves the image somewhere
    assert np.array_equal(got, want)
    assert np.array_equal(affine.warp(xd, up(Tr), 0.25).cpu().numpy(), want)
    assert np.array_equal(affine.warp(x, Tr, 0.25), want)                   # numpy in, numpy out
    far = np.array([[1, 0, 5.0], [0, 1, 0]], np.float64)                    # everything outside
    assert (c_warp(xd, far, True, 0.25) == np.float32(0.25)).all()
    for k in range(6):                                                      # a NaN anywhere in T: all fill, no fault
        Tn = R.identity().ravel()
        Tn[k] = np.nan
        got = c_warp(xd, Tn, True, 0.25)
        rows_hit = got == np.float32(0.25)
        assert rows_hit.all(), f"NaN at {k}"
    inf = np.array([[np.inf, 0, 0], [0, 1, -np.inf]], np.float64)
    assert (c_warp(xd, inf, True, 0.0) == 0.0).all()


def test_one_transform_shared_by_three_images():
    x = images(3, 24, 40)
    T = rot(24, 40, -3.0, 0.98, (1.25, 0.5))
    want = R.warp(x, T, 0.0)
    assert np.array_equal(c_warp(up(x), T, True, 0.0), want)
    assert np.array_equal(affine.warp(up(x), T).cpu().numpy(), want)
    assert np.array_equal(affine.warp(x[1], T), want[1])                    # one [H,W] image


# ---- the samples --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 5, 1000])
def test_samples(n):
    H, W = 33, 47
    out = Guarded(n * 4)
    _lib.check(_lib.load().emd_mi_samples_u32(n, H, W, 12345678901234, out.ptr(), _lib.stream_ptr()), "emd_mi_samples_u32")
    torch.cuda.synchronize()
    want = R.draw_samples(n, H, W, 12345678901234)
    assert out.intact() and np.array_equal(out.bits().cpu().numpy().astype(np.uint32)[:n], want)
    assert np.array_equal(affine.draw_samples(n, H, W, 3).cpu().numpy().astype(np.uint32), R.draw_samples(n, H, W, 3))
    assert int(want.max()) < H * W and (n < 1000 or len(np.unique(want)) < n)


# ---- the metric ---------------------------------------------------------------------------------------------------------------------

def inverted(x):
    return R.invert_contrast(x, float(x.max()) * 1.0001)


@functools.lru_cache(maxsize=None)
def metric_cases():
    """name -> (fixed [P,H,W], moving, T [P,2,3], samples or None, bins).  One workgroup (16 x 16), two (33 x 47), four (64 x 64), the cap
    of 64 partials with more than 1024 samples each (320 x 320); bins 8, 50 and 64; an image against itself, against its inverted
    copy, and under a candidate that puts about half the samples outside."""
    cases = {}
    for H, W, bins in ((16, 16, 8), (33, 47, 50), (64, 64, 64), (64, 64, 50), (320, 320, 50)):
        a = smooth(H, W)[None]
        half = np.array([[[1, 0, 1.0], [0, 1, 0]]], np.float64)             # shifted by half the image
        cases[f"{H}x{W} itself, bins {bins}"] = (a, a, R.identity()[None], None, bins)
        cases[f"{H}x{W} inverted, rotated, bins {bins}"] = (a, inverted(a), rot(H, W)[None], None, bins)
        cases[f"{H}x{W} half outside, bins {bins}"] = (a, inverted(a), half, None, bins)
    a = smooth(64, 64)[None]
    cases["64x64 1000 samples, bins 50"] = (a, inverted(a), rot(64, 64)[None], tuple(R.draw_samples(1000, 64, 64, 5).tolist()), 50)
    three = np.stack([smooth(64, 64, k) for k in range(3)])
    cands = np.stack([R.identity(), rot(64, 64), rot(64, 64, -4.0, 0.95, (3.0, 1.0))])
    cases["three pairs, three candidates, bins 50"] = (three, np.stack([three[1], inverted(three[1]), inverted(three[2])]), cands, None, 50)
    return cases


def restated_histograms(case):
    f, m, T, samples, bins = metric_cases()[case]
    s = None if samples is None else np.array(samples, np.uint32)
    return [R.joint_histogram(f[p], m[p], T[p], s, bins) for p in range(len(f))]


def yardstick():
    worst = 0.0
    for case in metric_cases():
        for p, h in enumerate(restated_histograms(case)):
            a, b = R.mi_of_histogram(h), R.mi_of_histogram_logs(h)
            inside = int(h.sum()) / 2.0 ** 32
            print(f"yardstick {case} pair {p}: MI {a:.15f}, the two evaluations {abs(a - b):.3e} apart; {inside:.1f} samples inside")
            worst = max(worst, abs(a - b))
    return worst


@pytest.mark.parametrize("case", list(metric_cases()), ids=lambda c: c.replace(" ", "_").replace(",", ""))
def test_mutual_information(case):
    f, m, T, samples, bins = metric_cases()[case]
    P, H, W = f.shape
    hists = restated_histograms(case)
    smp = None if samples is None else up(np.array(samples, np.int32))
    if samples is not None:
        assert len(set(samples)) < len(samples)                             # drawn with replacement: duplicates
    if "half outside" in case:
        assert 0.3 * H * W <= hists[0].sum() / 2.0 ** 32 <= 0.7 * H * W
    mi, hist, status = affine.mutual_information(up(f), up(m), up(T), smp, bins, return_histogram=True, return_status=True)
    assert mi.dtype == torch.float64 and tuple(mi.shape) == (P,) and hist.dtype == torch.int64 and tuple(hist.shape) == (P, bins, bins)
    for p in range(P):
        assert np.array_equal(hist[p].cpu().numpy(), hists[p]), f"{case} pair {p}: the histogram"
        want = R.mi_of_histogram(hists[p])
        e = abs(float(mi[p]) - want)
        print(f"{case} pair {p}: MI {float(mi[p]):.15f} against {want:.15f}: {e:.3e} (bar {mi_bar(bins, want):.3e})")
        assert e <= mi_bar(bins, want) and int(status[p]) == 0
    if "itself" in case and bins >= 50:
        assert float(mi[0]) > 0.5
    again = affine.mutual_information(up(f), up(m), up(T), smp, bins)
    assert torch.equal(again, mi)                                           # the same bits twice


def test_everything_outside_and_constant_images():
    a = smooth(33, 47)[None]
    far = np.array([[[1, 0, 9.0], [0, 1, 0]]], np.float64)
    nan = np.array([[[np.nan, 0, 0], [0, 1, 0]]], np.float64)
    for T in (far, nan):
        mi, hist, status = affine.mutual_information(up(a), up(inverted(a)), up(T), None, 50, return_histogram=True, return_status=True)
        assert float(mi[0]) == 0.0 and int(hist.sum()) == 0 and int(status[0]) == affine.MI_EMPTY
    flat = np.full_like(a, 0.75)
    two_f, two_m = np.concatenate([a, a]), np.concatenate([flat, inverted(a)])
    mi, hist, status = affine.mutual_information(up(two_f), up(two_m), up(np.stack([R.identity()] * 2)), None, 50, return_histogram=True,
                                                 return_status=True)
    assert float(mi[0]) == 0.0 and int(hist[0].sum()) == 0 and status.tolist() == [affine.MI_CONSTANT, 0] and float(mi[1]) > 0.1
    mi = affine.mutual_information(flat[0], a[0], R.identity())            # numpy in, one [H,W] pair: a 0-d numpy result
    assert isinstance(mi, np.ndarray) and mi.shape == () and float(mi) == 0.0


def test_the_metric_stays_inside_its_buffers():
    f, m, T, samples, bins = metric_cases()["three pairs, three candidates, bins 50"]
    lib = _lib.load()
    P, H, W = f.shape
    nbytes = lib.emd_mattes_mi_workspace_bytes(P, H, W, 0, bins)
    mi, status, hist, ws = Guarded(P * 8), Guarded(P * 4), Guarded(P * bins * bins * 8), Guarded(nbytes, fill=float("nan"))
    fd, md, td = up(f), up(m), up(T)
    _lib.check(lib.emd_mattes_mi_f64(fd.data_ptr(), md.data_ptr(), P, H, W, td.data_ptr(), None, 0, bins, mi.ptr(), status.ptr(), hist.ptr(),
                                     ws.ptr(), nbytes, _lib.stream_ptr()), "emd_mattes_mi_f64")
    torch.cuda.synchronize()
    assert mi.intact() and status.intact() and hist.intact() and ws.intact()
    want = affine.mutual_information(fd, md, td, None, bins)
    assert torch.equal(mi.f64(), want) and status.bits().tolist() == [0, 0, 0]


# ---- the normals --------------------------------------------------------------------------------------------------------------------

def test_normals():
    got = affine.normals(64, 3, seed=77).cpu().numpy()
    want = R.normals(64, 3, seed=77)
    e = float(np.abs(got - want).max())
    print(f"normals, 64 iterations x 3 pairs: {e:.3e} from the restatement (bar {NORMAL_BAR:.1e}); largest |z| {np.abs(want).max():.3f}")
    assert got.shape == (64, 3, 6) and e <= NORMAL_BAR
    later = affine.normals(4, 3, seed=77, first_iteration=60).cpu().numpy()
    assert np.array_equal(later, got[60:])


# ---- the optimizer, teacher-forced --------------------------------------------------------------------------------------------------

ITERS = 40


@functools.lru_cache(maxsize=None)
def forced_inputs():
    """Two pairs of different images at 64 x 64, and variates [ITERS, 2, 6]."""
    a, b = smooth(64, 64, 3), smooth(64, 64, 4)
    fixed = np.stack([a, b])
    moving = np.stack([inverted(R.warp(a[None], rot(64, 64, 1.0, 1.01, (0.5, -0.5)))[0]), R.warp(b[None], rot(64, 64, -1.5, 0.99, (-1.0, 0.25)))[0]])
    variates = np.random.default_rng(40).standard_normal((ITERS, 2, 6))
    return fixed, moving, variates


def forced_truth():
    """The pull maps that align forced_inputs: the inverses of the maps the moving images were made with.  Started there, the optimizer
    rejects most children, and A shrinks."""
    return np.stack([R.inverse(rot(64, 64, 1.0, 1.01, (0.5, -0.5))), R.inverse(rot(64, 64, -1.5, 0.99, (-1.0, 0.25)))])


@functools.lru_cache(maxsize=None)
def forced_ref(epsilon=1.5e-6, initial_radius=6.25e-3, at_truth=False):
    fixed, moving, variates = forced_inputs()
    T0 = forced_truth() if at_truth else [None, None]
    return [R.register(fixed[p], moving[p], ITERS, variates, epsilon=epsilon, initial_radius=initial_radius, T0=T0[p], pair=p) for p in range(2)]


def check_margins(refs, what):
    for p, r in enumerate(refs):
        m = min(r["margins"]) if r["margins"] else np.inf
        print(f"{what} pair {p}: {r['iterations']} evaluations, {r['accepted']} accepted, status {r['status']}, smallest decision margin {m:.3e} "
              f"(>= {MARGIN_MIN})")
        assert m >= MARGIN_MIN, what


def check_state(fields, refs, what):
    for p, r in enumerate(refs):
        assert np.array_equal(fields["x"][p].cpu().numpy(), r["x"]), f"{what} pair {p}: x"
        assert np.array_equal(fields["A"][p].cpu().numpy(), r["A"]), f"{what} pair {p}: A"
        assert int(fields["accepted"][p]) == r["accepted"] and int(fields["iterations"][p]) == r["iterations"]
        assert int(fields["status"][p]) == r["status"]
        e = abs(float(fields["f"][p]) - r["f"])
        print(f"{what} pair {p}: x and A bitwise equal, {r['accepted']} accepted; f {float(fields['f'][p]):.15f} against {r['f']:.15f}: {e:.3e} "
              f"(bar {mi_bar(50, r['f']):.3e})")
        assert e <= mi_bar(50, r["f"])


def test_optimizer_teacher_forced():
    fixed, moving, variates = forced_inputs()
    refs = forced_ref()
    check_margins(refs, "teacher-forced")
    assert all(r["status"] == 0 and r["iterations"] == ITERS and 0 < r["accepted"] < ITERS - 1 for r in refs)
    fd, md, vd = up(fixed), up(moving), up(variates)
    state = affine.iterate(fd, md, None, ITERS, variates=vd, reset=True)
    check_state(affine.state_fields(state), refs, "teacher-forced")
    again = affine.iterate(fd, md, None, ITERS, variates=vd, reset=True)
    assert torch.equal(again.view(torch.int64), state.view(torch.int64))    # the same bits twice
    # register() with the same variates, one level: the same transforms
    T, st = affine.register(fd, md, iterations=ITERS, samples=None, levels=1, variates=vd, return_state=True)
    assert torch.equal(st.view(torch.int64), state.view(torch.int64)) and tuple(T.shape) == (2, 2, 3)
    assert np.array_equal(T.cpu().numpy(), np.stack([r["T"] for r in refs]))
    # one more evaluation than there are rows: the stream has run out, and the state says so
    more = affine.iterate(fd, md, state.clone(), 2, variates=vd)
    assert affine.state_fields(more)["status"].tolist() == [affine.EXHAUSTED] * 2 and affine.state_fields(more)["iterations"].tolist() == [ITERS + 1] * 2


def test_optimizer_stops_early_and_stays_stopped():
    fixed, moving, variates = forced_inputs()
    refs = forced_ref(epsilon=1e-2, initial_radius=4.2e-3, at_truth=True)
    check_margins(refs, "early stop")
    assert all(r["status"] == R.CONVERGED and 1 < r["iterations"] < ITERS for r in refs)
    fd, md, vd = up(fixed), up(moving), up(variates)
    state = affine.iterate(fd, md, None, ITERS, variates=vd, epsilon=1e-2, initial_radius=4.2e-3, reset=True, T0=up(forced_truth()))
    check_state(affine.state_fields(state), refs, "early stop")
    kept = state.clone()
    affine.iterate(fd, md, state, 7, variates=vd, epsilon=1e-2, initial_radius=4.2e-3)
    assert torch.equal(state.view(torch.int64), kept.view(torch.int64))     # untouched by further iterations


def test_a_constant_image_is_degenerate():
    fixed, moving, variates = forced_inputs()
    moving = moving.copy()
    moving[0] = 0.5
    state = affine.iterate(up(fixed), up(moving), None, 5, variates=up(variates), reset=True)
    f = affine.state_fields(state)
    assert f["status"].tolist() == [affine.DEGENERATE, 0] and float(f["f"][0]) == 0.0 and int(f["iterations"][0]) == 0
    assert not f["x"][0].any() and int(f["iterations"][1]) == 5
    ref = R.register(fixed[1], moving[1], 5, variates, pair=1)
    assert np.array_equal(f["x"][1].cpu().numpy(), ref["x"]) and np.array_equal(f["A"][1].cpu().numpy(), ref["A"])


def test_the_optimizer_stays_inside_its_buffers():
    fixed, moving, variates = forced_inputs()
    lib = _lib.load()
    nbytes = lib.emd_mattes_mi_workspace_bytes(2, 64, 64, 0, 50)
    state, ws = Guarded(2 * affine.STATE_DOUBLES * 8), Guarded(nbytes, fill=float("nan"))
    fd, md, vd = up(fixed), up(moving), up(variates)
    _lib.check(lib.emd_affine_register_f64(fd.data_ptr(), md.data_ptr(), 2, 64, 64, None, 0, 50, 6.25e-3, 1.05, 1.5e-6, 0, vd.data_ptr(), ITERS,
                                           affine.RESET, None, 0, ITERS, state.ptr(), ws.ptr(), nbytes, _lib.stream_ptr()),
               "emd_affine_register_f64")
    torch.cuda.synchronize()
    assert state.intact() and ws.intact()
    check_state(affine.state_fields(state.f64().reshape(2, affine.STATE_DOUBLES)), forced_ref(), "guarded")


# ---- capture ------------------------------------------------------------------------------------------------------------------------

def test_a_captured_block_of_iterations_replays_on_other_images():
    fixed, moving, variates = forced_inputs()
    fd, md, vd = up(fixed), up(moving), up(variates)
    eager = affine.iterate(fd, md, None, ITERS, variates=vd, reset=True)
    start = affine.iterate(fd, md, None, 0, reset=True)                     # the initial state alone
    sf, sm = up(fixed[::-1].copy()), up(moving[::-1].copy())                # other images while capturing
    st = affine.iterate(sf, sm, None, 3, variates=vd, reset=True)           # and another state
    ws = torch.empty(_lib.load().emd_mattes_mi_workspace_bytes(2, 64, 64, 0, 50) // 8 + 1, dtype=torch.float64, device=dev())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        affine.iterate(sf, sm, st, 10, variates=vd, workspace=ws)
        with pytest.raises(RuntimeError, match="capture"):                  # crop=True would read the limits back
            affine.warp_stack(sf, vd[0, :1].reshape(1, 2, 3), crop=True)
    sf.copy_(fd)
    sm.copy_(md)
    st.copy_(start)
    for _ in range(4):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(st.view(torch.int64), eager.view(torch.int64))


# ---- recovery, end to end -----------------------------------------------------------------------------------------------------------

def test_recovery_of_a_rotated_scaled_shifted_and_inverted_image():
    """register with Philox, seed 0, one level, 600 evaluations, every pixel, on the input of tests/affine_ref.recovery_inputs."""
    fixed, moving, T = R.recovery_inputs()
    ref = R.recovery_run()
    want = R.corner_error(ref["T"], T, 64, 64)
    print(f"recovery, the restatement: {want:.3f} px, {ref['accepted']} accepted, smallest margin {min(ref['margins']):.3e}")
    assert want <= 0.5 and min(ref["margins"]) >= MARGIN_MIN                # on the CPU first
    got, state = affine.register(up(fixed[None]), up(moving[None]), iterations=600, samples=None, levels=1, seed=0, return_state=True)
    f = affine.state_fields(state)
    err = R.corner_error(got[0].cpu().numpy(), T, 64, 64)
    print(f"recovery, the device: {err:.3f} px, {int(f['accepted'][0])} accepted, MI {float(f['f'][0]):.6f} (the restatement: {ref['f']:.6f}); "
          f"from the restatement's transform {R.corner_error(got[0].cpu().numpy(), ref['T'], 64, 64):.3e} px")
    assert int(f["accepted"][0]) == ref["accepted"] and int(f["iterations"][0]) == 600 and err <= 0.5


# ---- the series ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def series():
    """Four 64 x 64 images, each a known small affine of the first, and the pair transforms [3,2,3] that align them."""
    from tests.synth_inputs import synthetic_pair

    field = synthetic_pair(1, 128, 128, seed=5)[1][0, :, :, 0]
    sampling = [R.identity(), R.similarity(1.0, 1.01, (1.0, -0.5), 64, 64), R.similarity(-1.5, 0.99, (-0.75, 1.25), 64, 64),
                R.similarity(2.0, 1.02, (1.5, -2.0), 64, 64)]
    stack = np.stack([R.sample_field(field, s, 64, 64, (32, 32)) for s in sampling]).astype(np.float32)
    hom = [np.vstack([s, [0, 0, 1]]) for s in sampling]
    pairs = np.stack([(np.linalg.inv(hom[k + 1]) @ hom[k])[:2] for k in range(3)])   # image k+1 sampled there shows what image k shows
    return stack, np.ascontiguousarray(pairs)


def test_series_chain_limits_and_warp():
    stack, pairs = series()
    xd, pd = up(stack), up(pairs)
    for middle in (None, 0, 3):
        Cm = affine.chain_to_middle(pd, middle)
        want = R.chain_to_middle(pairs, middle)
        assert Cm.dtype == torch.float64 and tuple(Cm.shape) == (4, 2, 3) and np.array_equal(Cm.cpu().numpy(), want)
        lim = affine.common_limits(Cm, 64, 64)
        assert lim.dtype == torch.int32 and lim.tolist() == R.common_limits(want, 64, 64).tolist()
    Cm = affine.chain_to_middle(pd).cpu().numpy()
    lim = R.common_limits(Cm, 64, 64).tolist()
    print(f"series: the common rectangle (x0, y0, w, h) = {lim}")
    assert (lim[0] > 0 or lim[1] > 0) and 48 <= lim[2] < 64 and 48 <= lim[3] < 64
    warped = affine.warp_stack(xd, pd, fill=0.25)
    assert np.array_equal(warped.cpu().numpy(), R.warp(stack, Cm, 0.25))    # the restatement fed the device's transforms
    # aligned: what is left is bilinear interpolation, twice over, of a field of Gaussians no narrower than 3 px and no higher than 1:
    # 2 x (1/8) x |f''| <= 2 / (8 x 9) = 0.028; the unaligned images differ by several times that
    inner = warped[:, 8:56, 8:56].cpu().numpy().astype(np.float64)
    worst, before = float(np.abs(inner - inner[2]).max()), float(np.abs(stack[:, 8:56, 8:56] - stack[2, 8:56, 8:56]).max())
    print(f"series: the warped images differ from the middle one by at most {worst:.4f} (<= 0.028), the unwarped ones by {before:.4f}")
    assert worst <= 0.028 < before
    cropped = affine.warp_stack(xd, pd, crop=True, fill=0.25)
    assert tuple(cropped.shape) == (4, lim[3], lim[2])
    assert torch.equal(cropped, warped[:, lim[1]:lim[1] + lim[3], lim[0]:lim[0] + lim[2]]) and not bool((cropped == 0.25).any())
    assert np.array_equal(affine.warp_stack(stack, pairs, fill=0.25), warped.cpu().numpy())          # numpy in, numpy out
    assert np.array_equal(affine.chain_to_middle(pairs), Cm) and affine.common_limits(Cm, 64, 64).tolist() == lim
    # guarded outputs of the two one-thread kernels
    cg, lg = Guarded(4 * 6 * 8), Guarded(16)
    lib = _lib.load()
    _lib.check(lib.emd_affine_chain_f64(pd.data_ptr(), 4, 2, cg.ptr(), _lib.stream_ptr()), "emd_affine_chain_f64")
    _lib.check(lib.emd_affine_limits_i32(cg.ptr(), 4, 64, 64, lg.ptr(), _lib.stream_ptr()), "emd_affine_limits_i32")
    torch.cuda.synchronize()
    assert cg.intact() and lg.intact() and lg.bits().tolist() == lim and np.array_equal(cg.f64().reshape(4, 2, 3).cpu().numpy(), Cm)


def test_a_singular_pair_transform_gives_fill_and_limits_of_zero_size():
    stack, pairs = series()
    bad = pairs.copy()
    bad[2] = [[1, 2, 0], [2, 4, 0]]                                          # the last pair: image 3
    Cm = affine.chain_to_middle(up(bad))
    want = R.chain_to_middle(bad)
    assert np.array_equal(Cm.cpu().numpy(), want, equal_nan=True) and np.isnan(want[3]).all() and np.isfinite(want[:3]).all()
    warped = affine.warp_stack(up(stack), up(bad), fill=0.25)
    assert bool((warped[3] == 0.25).all()) and np.array_equal(warped[:3].cpu().numpy(), R.warp(stack[:3], want[:3], 0.25))
    assert affine.common_limits(Cm, 64, 64).tolist() == [0, 0, 0, 0]
    assert tuple(affine.warp_stack(up(stack), up(bad), crop=True).shape) == (4, 0, 0)
    bad[2] = pairs[2]
    bad[0, 0, 0] = np.inf                                                    # below the middle: images 0 and, through it, none other
    want = R.chain_to_middle(bad)
    assert np.array_equal(affine.chain_to_middle(up(bad)).cpu().numpy(), want, equal_nan=True) and np.isnan(want[0]).all()


def test_align_registers_and_warps_a_series_through_a_pyramid():
    """The whole path on two levels (64 -> 32) with drawn samples: shapes, types, the same bits twice, and the pairs it returns are the
    ones it warps with.  How well 60 evaluations align is not asserted."""
    stack, _ = series()
    xd = up(stack)
    kw = dict(iterations=60, samples=1500, levels=2, seed=4)
    aligned, pairs = affine.align(xd, fill=0.25, **kw)
    assert aligned.is_cuda and aligned.dtype == torch.float32 and tuple(aligned.shape) == (4, 64, 64) and tuple(pairs.shape) == (3, 2, 3)
    assert pairs.dtype == torch.float64 and bool(torch.isfinite(pairs).all()) and float((pairs - up(R.identity())).abs().max()) > 0
    again, pairs2 = affine.align(xd, fill=0.25, **kw)
    assert torch.equal(pairs2, pairs) and torch.equal(again, aligned)
    assert np.array_equal(aligned.cpu().numpy(), R.warp(stack, R.chain_to_middle(pairs.cpu().numpy()), 0.25))
    state = affine.register_series(xd, return_state=True, **kw)[1]
    assert affine.state_fields(state)["iterations"].tolist() == [60] * 3
    n_aligned, n_pairs = affine.align(stack, fill=0.25, **kw)               # numpy in, numpy out
    assert isinstance(n_aligned, np.ndarray) and np.array_equal(n_pairs, pairs.cpu().numpy())


if __name__ == "__main__":
    w = yardstick()
    print(f"MI: the two float64 evaluations' largest distance {w:.3e} (bar {FACTOR * w:.3e}, with the floor of bins^2 2^-53 max(1, MI): "
          f"{2500 * 2.0 ** -53:.3e} at 50 bins)")
    for what, refs in (("teacher-forced", forced_ref()), ("early stop", forced_ref(1e-2, 4.2e-3, True))):
        check_margins(refs, what)
    print("series limits:", R.common_limits(R.chain_to_middle(series()[1]), 64, 64).tolist())
