"""GPU tests of the registration of a focal series (csrc/register.hip, emdenoise.exitwave) against the float64 numpy
restatement of tests/register_ref.py.  OpenCV is not installed: nothing is compared with cv2, the formulas of include/emdenoise.h are
the specification.

Inputs: broadband images (``synthetic_lq``; uniform noise from 512 x 512 up, where ``synthetic_lq`` takes seconds), displaced circularly
by integers (``numpy.roll``) or by fractions (a Fourier phase ramp on the CPU, rounded to float32).  Conditions, asserted on the CPU
before a case goes to the GPU: the peak of the restated surface exceeds the runner-up by >= 1e-3 of the peak (rounding cannot move the
argmax), and sum |v| / |sum v| over the 5 x 5 window is <= 8 (the centroid does not cancel).

The bars are not derived from the device's output.

* Surfaces: relative L2 against the restatement; the bar is FACTOR = 4 times YARD_SURFACE, the LARGEST distance, over the cases of
  this file, between the restatement on ``numpy.fft`` and on the plain float64 radix-2 FFT of tests/fft_ref.py.
* Shifts, responses and centres: absolute; 4 times YARD_SHIFT, the same two-back-end distance of the shifts, responses and centres,
  with a floor of S 2^-50 (a coordinate up to S carries S 2^-53 of rounding; the floor is eight of those).  YARD_SHIFT is 5.7e-14
  and 4 times that is 256 x 2^-50: the floor binds from S = 256 up, the yardstick below.
* One case has a yardstick of its own, which the others do not inherit: the half-pixel shift (0.5, 0.5) without the window.  A real
  image shifted by half a pixel has no Nyquist row or column (cos(pi / 2) = 0): after the rounding to float32 those 2 S - 1 terms of
  F(b) are noise eight orders below the rest, and R = P / |P| lifts their rounding error to full weight.  The two restatements are
  8.9e-10 (surface) and 1.3e-11 (shift) apart there and 5.4e-15 / 5.7e-14 everywhere else; a single largest distance would have
  widened every bar by five orders.
* Crops: bit for bit against the restatement fed the device's centres.

``python -m tests.test_register_gpu`` computes the yardsticks on the CPU.  Every figure is printed before it is asserted."""
import functools

import numpy as np
import pytest
import torch

from emdenoise import _lib, exitwave
from emdenoise.exitwave import PC_CHAIN, PC_WINDOW                      # absent before the registration existed: nothing here runs without it
from tests import exitwave_ref as ER
from tests import register_ref as R
from tests.synth_inputs import synthetic_lq
from tests.test_exitwave_gpu import Guarded, SENTINEL, bits, dev, up, wave_bar

pytestmark = pytest.mark.gpu

FACTOR = 4.0
YARD_SURFACE, YARD_SHIFT = 5.382e-15, 5.685e-14            # python -m tests.test_register_gpu, rounded up
YARD_SURFACE_HALF, YARD_SHIFT_HALF = 8.871e-10, 1.336e-11  # the half-pixel shift without the window, see above
MARGIN_MIN, CANCEL_MAX = 1e-3, 8.0
PAIR_CASES = {8: [(0, 0), (3, -3), (-3, 3)], 16: [(7, 7), (-2, 1)], 32: [(0, 0), (15, -15), (-15, 15)], 64: [(31, 31), (-31, -31)],
              256: [(127, -127), (-5, 9)]}
SUBPIXEL = [(2.3, -1.6), (0.5, 0.5), (-4.25, 3.75)]        # at S = 64
CHAIN_CASES = [(2, 64), (3, 64), (5, 64), (2, 512), (2, 1024), (2, 2048)]
CHAIN_OFFSETS = [(0, 0), (3, -2), (-4, 1), (6, 5), (-1, -7)]
# Their mean is whole, (1, 1): the four crops are copies of one window of the field.  With a fractional mean (quarters, N = 4) a bilinear
# sample of float32 pixels is a short dyadic number that sits on a float32 rounding tie every few pixels, and the 1e-15 by which two
# centres differ tips those ties: 1.5e-8 relative between crops, measured.  The bilinear arithmetic is checked bit for bit in test_crop_stack.
SIGN_OFFSETS = [(0, 0), (2, -1), (-1, 3), (3, 2)]
SERIES_OFFSETS = [(0, 0), (2, -1), (-3, 1)]
SERIES_OFFSETS_2 = [(1, 2), (-2, 3), (0, -3)]


def surface_bar(half=False):
    return FACTOR * (YARD_SURFACE_HALF if half else YARD_SURFACE)


def shift_bar(S, half=False):
    return max(FACTOR * (YARD_SHIFT_HALF if half else YARD_SHIFT), S * 2.0 ** -50)


@functools.lru_cache(maxsize=None)
def image(S, k=0):
    """A broadband float32 image [S,S].  Cached: do not write into the result."""
    if S >= 512:
        return np.random.default_rng(S + k).random((S, S), dtype=np.float32)
    return synthetic_lq(1, S, S, seed=1100 + S + 17 * k)[0, :, :, 0]


def rolled(x, dx, dy):
    """x displaced by (+dx, +dy), circularly."""
    return np.roll(x, (dy, dx), (0, 1))


@functools.lru_cache(maxsize=None)
def pair_inputs(S):
    a = np.stack([image(S, k) for k in range(len(PAIR_CASES[S]))])
    return a, np.stack([rolled(a[k], *d) for k, d in enumerate(PAIR_CASES[S])])


@functools.lru_cache(maxsize=None)
def subpixel_inputs():
    a = np.stack([image(64, 10 + k) for k in range(len(SUBPIXEL))])
    return a, np.stack([R.fourier_shift(a[k], *d) for k, d in enumerate(SUBPIXEL)]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def chain_inputs(N, S):
    return np.stack([rolled(image(S, 20), *CHAIN_OFFSETS[k]) for k in range(N)])


@functools.lru_cache(maxsize=None)
def shifted_series(offsets=tuple(SERIES_OFFSETS)):
    """The simulated focal series of test_exitwave_gpu at 64 x 64, image k rolled by offsets[k]."""
    images, df = ER.series(len(offsets), 64)
    return np.stack([rolled(images[k], *o) for k, o in enumerate(offsets)]), df


def sign_inputs():
    """A 96 x 96 field, its central 64 x 64 part, and that part rolled by SIGN_OFFSETS.  The cut comes BEFORE the roll: rolling the
    96 x 96 field and cutting afterwards gives images that are no circular shifts of one another, and the restatement is then up to
    0.77 px away from the offsets' differences (measured on the CPU), far from the 1e-9 that this test asserts before it touches the GPU."""
    field = synthetic_lq(1, 96, 96, seed=77)[0, :, :, 0]
    return field, np.stack([rolled(field[16:80, 16:80], *o) for o in SIGN_OFFSETS])


def restate(a, b, window=None, fft=R.NumpyFFT):
    return [R.phase_correlate(x, y, window, fft) for x, y in zip(a, b)]


def check_conditions(refs, what):
    for p, r in enumerate(refs):
        print(f"{what} pair {p}: margin (peak - runner-up) / peak {r['margin']:.3e} (>= {MARGIN_MIN}); sum |v| / |sum v| "
              f"{r['cancellation']:.3f} (<= {CANCEL_MAX})")
        assert r["margin"] >= MARGIN_MIN and r["cancellation"] <= CANCEL_MAX, what


def check_pairs(got_shifts, got_resp, got_surf, refs, S, what, half=()):
    for p, r in enumerate(refs):
        h = p in half
        es = R.rel_l2(got_surf[p], r["surface"])
        ed = float(np.abs(got_shifts[p] - r["shift"]).max())
        er = abs(float(got_resp[p]) - r["response"])
        print(f"{what} pair {p}: surface rel L2 {es:.3e} (bar {surface_bar(h):.3e}); shift {got_shifts[p]} against {r['shift']}: {ed:.3e}, "
              f"response {er:.3e} (bar {shift_bar(S, h):.3e})")
        assert es <= surface_bar(h) and ed <= shift_bar(S, h) and er <= shift_bar(S, h), what


def yardstick():
    """The largest distances between the restatement on numpy.fft and on the radix-2 FFT over this file's cases (CPU)."""
    worst = {"surface": 0.0, "shift": 0.0, "surface_half": 0.0, "shift_half": 0.0}
    conditions = []                                                         # (case, margin, cancellation) of every pair

    def note(what, a, b, win=None, half=()):
        for p, (x, y) in enumerate(zip(restate(a, b, win), restate(a, b, win, R.Radix2FFT))):
            es = R.rel_l2(y["surface"], x["surface"])
            ed = max(float(np.abs(y["shift"] - x["shift"]).max()), abs(y["response"] - x["response"]))
            print(f"yardstick {what} pair {p}: surface {es:.3e}, shift / response {ed:.3e}; margin {x['margin']:.3e}, cancellation "
                  f"{x['cancellation']:.3f}")
            conditions.append((f"{what} pair {p}", x["margin"], x["cancellation"]))
            k = "_half" if p in half else ""
            worst["surface" + k] = max(worst["surface" + k], es)
            worst["shift" + k] = max(worst["shift" + k], ed)

    for S in PAIR_CASES:
        a, b = pair_inputs(S)
        note(f"pairs {S}", a, b)
    a, b = subpixel_inputs()
    note("sub-pixel", a, b, half=(1,))
    note("sub-pixel, window", a, b, R.hanning_window(64))
    stacks = [(f"chain {c}", chain_inputs(*c)) for c in CHAIN_CASES] + [("sign", sign_inputs()[1]), ("series", shifted_series()[0]),
                                                                       ("series 2", shifted_series(tuple(SERIES_OFFSETS_2))[0])]
    for what, st in stacks:
        note(what, st[:-1], st[1:])
        S = st.shape[-1]
        c0, c1 = R.centres_of(R.chain_shifts(st), S), R.centres_of(R.chain_shifts(st, fft=R.Radix2FFT), S)
        print(f"yardstick {what}: centres {np.abs(c1 - c0).max():.3e}")
        worst["shift"] = max(worst["shift"], float(np.abs(c1 - c0).max()))
    return worst, conditions


# ---- the window ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [8, 64, 256, 4096])
def test_hanning_window(S):
    w1, w2 = exitwave.hanning_window(S, one_d=True), exitwave.hanning_window(S)
    assert w1.dtype == np.float64 and w1.shape == (S,) and w2.shape == (S, S)
    e1 = float(np.abs(w1 - R.hanning_1d(S)).max())
    e2 = float(np.abs(w2 - np.sqrt(w1[:, None] * w1[None, :])).max())
    print(f"Hann table {S}: against numpy's formula {e1:.3e}; the 2-D window against sqrt(w[y] w[x]) of the device's table {e2:.3e}; "
          f"bar {2.0 ** -52:.3e}")
    assert e1 <= 2.0 ** -52 and e2 <= 2.0 ** -52 and w1[0] == 0.0 and w2[0, 0] == 0.0


# ---- phase correlation, pair mode ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", sorted(PAIR_CASES))
def test_phase_correlate_pairs(S):
    a, b = pair_inputs(S)
    refs = restate(a, b)
    check_conditions(refs, f"pairs {S}")
    for r, d in zip(refs, PAIR_CASES[S]):
        print(f"  the restatement against the true shift {d}: {np.abs(r['shift'] - np.array(d)).max():.3e}")
    shifts, resp, surf = exitwave.phase_correlate(up(a), up(b), return_response=True, return_surface=True)
    B = len(PAIR_CASES[S])
    assert shifts.is_cuda and shifts.dtype == torch.float64 and tuple(shifts.shape) == (B, 2) and tuple(resp.shape) == (B,)
    assert tuple(surf.shape) == (B, S, S)
    check_pairs(shifts.cpu().numpy(), resp.cpu().numpy(), surf.cpu().numpy(), refs, S, f"pairs {S}")
    for p, d in enumerate(PAIR_CASES[S]):                                   # the peak sits at S/2 - d of the shifted surface
        assert int(surf[p].argmax()) == (S // 2 - d[1]) * S + (S // 2 - d[0])
    alone = exitwave.phase_correlate(up(a), up(b))
    assert torch.equal(alone, shifts)


def test_images_of_zeros_give_no_shift_and_no_response():
    S = 16
    a, b = pair_inputs(S)
    a, b = a.copy(), b.copy()
    a[0], b[0] = 0.0, 0.0
    shifts, resp, surf = exitwave.phase_correlate(up(a), up(b), return_response=True, return_surface=True)
    assert shifts[0].tolist() == [0.0, 0.0] and float(resp[0]) == 0.0 and not surf[0].any()
    ref = R.phase_correlate(a[1], b[1])
    assert np.abs(shifts[1].cpu().numpy() - ref["shift"]).max() <= shift_bar(S)
    assert R.phase_correlate(a[0], b[0])["shift"].tolist() == [0.0, 0.0]


def test_the_two_inputs_may_share_bytes():
    """a == b is an autocorrelation: a delta at the centre, shift 0, response 1.  Overlapping views of one stack in pair mode give the
    bits of chain mode."""
    S = 64
    x = up(chain_inputs(3, S))
    shifts, resp, surf = exitwave.phase_correlate(x, x, return_response=True, return_surface=True)
    delta = torch.zeros_like(surf)
    delta[:, S // 2, S // 2] = 1.0
    e = float(torch.linalg.norm((surf - delta).reshape(-1)) / 3 ** 0.5)
    print(f"autocorrelation: surface against the delta {e:.3e} (bar {surface_bar():.3e}); shifts {shifts.abs().max():.3e}, responses "
          f"{(resp - 1).abs().max():.3e} (bar {shift_bar(S):.3e})")
    assert e <= surface_bar() and float(shifts.abs().max()) <= shift_bar(S) and float((resp - 1).abs().max()) <= shift_bar(S)
    views = exitwave.phase_correlate(x[:-1], x[1:])
    assert torch.equal(views, exitwave.rel_pos_estimate(x, as_cropping_centres=False))


@pytest.mark.parametrize("S", [8, 64])
def test_a_flat_surface_takes_the_first_peak_in_row_major_order(S):
    """Two constant images: the line transform of a constant is exact (one term, the others sums of zeros), so R is 1 at the origin and
    0 elsewhere and the surface is 1 / S^2 everywhere, bit for bit.  The first peak is (0, 0) of the shifted surface; the window is
    clipped to 3 x 3 there: centroid (1, 1), shift (S/2 - 1, S/2 - 1), response 9 / S^2, all exact."""
    a, b = np.full((1, S, S), 3.0, np.float32), np.full((1, S, S), 0.5, np.float32)
    shifts, resp, surf = exitwave.phase_correlate(up(a), up(b), return_response=True, return_surface=True)
    assert bool((surf == 1.0 / (S * S)).all())
    assert shifts[0].tolist() == [S / 2 - 1.0, S / 2 - 1.0] and float(resp[0]) == 9.0 / (S * S)


@pytest.mark.parametrize("window", [False, True], ids=["plain", "window"])
def test_phase_correlate_sub_pixel(window):
    S = 64
    a, b = subpixel_inputs()
    win = exitwave.hanning_window(S) if window else None                     # the device's bits
    refs = restate(a, b, win)
    check_conditions(refs, f"sub-pixel, window {window}")
    for r, d in zip(refs, SUBPIXEL):
        print(f"  the restatement against the true shift {d}: {r['shift']}, {np.abs(r['shift'] - np.array(d)).max():.3e} (not asserted: the "
              f"5 x 5 centroid of a Dirichlet kernel is no sub-pixel estimator of that accuracy)")
    shifts, resp, surf = exitwave.phase_correlate(up(a), up(b), window=window, return_response=True, return_surface=True)
    check_pairs(shifts.cpu().numpy(), resp.cpu().numpy(), surf.cpu().numpy(), refs, S, f"sub-pixel, window {window}",
                half=() if window else (1,))


# ---- chain mode ---------------------------------------------------------------------------------------------------------------------

def c_correlate(x, P, S, flags, b=None, want_surface=True, fill=float("nan")):
    """The C call on guarded buffers and a workspace of exactly the advertised size, NaN-filled."""
    lib = _lib.load()
    nbytes = lib.emd_phase_correlate_workspace_bytes(P, S, flags)
    shifts, surface, ws = Guarded(P * 3 * 8), Guarded(P * S * S * 8), Guarded(nbytes, fill=fill)
    rc = lib.emd_phase_correlate_f64(x.data_ptr(), b.data_ptr() if b is not None else None, P, S, flags, shifts.ptr(),
                                     surface.ptr() if want_surface else None, ws.ptr(), nbytes, _lib.stream_ptr())
    _lib.check(rc, "emd_phase_correlate_f64")
    torch.cuda.synchronize()
    return shifts, surface, ws


@pytest.mark.parametrize("case", CHAIN_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_chain_mode(case):
    N, S = case
    st = chain_inputs(N, S)
    refs = restate(st[:-1], st[1:])
    check_conditions(refs, f"chain {case}")
    x = up(st)
    shifts, surface, ws = c_correlate(x, N - 1, S, PC_CHAIN)
    assert shifts.intact() and surface.intact() and ws.intact()
    got = shifts.f64().reshape(N - 1, 3).cpu().numpy()
    check_pairs(got[:, :2], got[:, 2], surface.f64().reshape(N - 1, S, S).cpu().numpy(), refs, S, f"chain {case}")
    for k in range(N - 1):
        d = np.array(CHAIN_OFFSETS[k + 1]) - np.array(CHAIN_OFFSETS[k])
        assert np.abs(got[k, :2] - d).max() <= shift_bar(S)                 # circular integer shifts come out as they went in
    # pair mode on the same pairs: the same bits
    ps, psurf, _ = c_correlate(x[:-1].clone(), N - 1, S, 0, b=x[1:].clone())
    assert torch.equal(ps.bits(), shifts.bits()) and torch.equal(psurf.bits(), surface.bits())
    # rel_pos_estimate
    sh = exitwave.rel_pos_estimate(x, as_cropping_centres=False)
    assert torch.equal(sh, shifts.f64().reshape(N - 1, 3)[:, :2])
    centres = exitwave.rel_pos_estimate(x)
    want = R.centres_of([r["shift"] for r in refs], S)
    e = float(np.abs(centres.cpu().numpy() - want).max())
    print(f"chain {case}: centres against the restatement {e:.3e}; bar {shift_bar(S):.3e}")
    assert tuple(centres.shape) == (N, 2) and e <= shift_bar(S)
    assert np.array_equal(exitwave.rel_pos_estimate(st), centres.cpu().numpy())     # numpy in, numpy out


def test_chain_mode_at_4096():
    """NU = 16 and the 64 KiB line.  A circular integer shift: the surface is a delta at S/2 - d, to the surface's bar."""
    S, d = 4096, (37, -1000)
    a = np.random.default_rng(4096).random((S, S), dtype=np.float32)
    x = up(np.stack([a, rolled(a, *d)]))
    lib = _lib.load()
    flags = PC_CHAIN
    nbytes = lib.emd_phase_correlate_workspace_bytes(1, S, flags)
    shifts = torch.full((3,), SENTINEL, dtype=torch.float64, device=dev())
    surf = torch.empty((S, S), dtype=torch.float64, device=dev())
    ws = torch.full((nbytes // 8,), float("nan"), dtype=torch.float64, device=dev())
    _lib.check(lib.emd_phase_correlate_f64(x.data_ptr(), None, 1, S, flags, shifts.data_ptr(), surf.data_ptr(), ws.data_ptr(), nbytes,
                                           _lib.stream_ptr()), "emd_phase_correlate_f64")
    peak = (S // 2 - d[1], S // 2 - d[0])
    assert int(surf.argmax()) == peak[0] * S + peak[1]
    delta = torch.zeros_like(surf)
    delta[peak] = 1.0
    e = float(torch.linalg.norm((surf - delta).reshape(-1)))
    got = shifts.cpu().numpy()
    print(f"4096: surface against the delta, rel L2 {e:.3e} (bar {surface_bar():.3e}); shift {got[:2]}, response {got[2]!r}; bar "
          f"{shift_bar(S):.3e}")
    assert e <= surface_bar() and np.abs(got[:2] - np.array(d)).max() <= shift_bar(S) and abs(got[2] - 1.0) <= shift_bar(S)


# ---- bits and safety ----------------------------------------------------------------------------------------------------------------

def test_outputs_stay_inside_their_sizes_and_two_runs_give_the_same_bits():
    lib = _lib.load()
    for N, S, flags in ((3, 8, PC_CHAIN), (3, 32, PC_CHAIN | PC_WINDOW), (2, 256, PC_CHAIN)):
        x = up(np.stack([rolled(image(S, 30), k, -2 * k) for k in range(N)]))
        first = c_correlate(x, N - 1, S, flags)
        again = c_correlate(x, N - 1, S, flags)
        assert all(g.intact() for g in first), f"{N} x {S}, flags {flags}: wrote outside shifts, surface or workspace"
        assert not torch.isnan(first[0].f64()).any() and not torch.isnan(first[1].f64()).any()
        assert torch.equal(first[0].bits(), again[0].bits()) and torch.equal(first[1].bits(), again[1].bits())
        none = c_correlate(x, N - 1, S, flags, want_surface=False)
        assert torch.equal(none[0].bits(), first[0].bits()) and bool((none[1].view == SENTINEL).all()) and none[2].intact()
        # the pair-mode workspace holds two transforms per pair
        pairs = c_correlate(x[:-1].clone(), N - 1, S, flags & ~PC_CHAIN, b=x[1:].clone())
        assert all(g.intact() for g in pairs) and torch.equal(pairs[0].bits(), first[0].bits())
        centres, out = Guarded(N * 2 * 8), Guarded(N * 5 * 5 * 4)
        _lib.check(lib.emd_stack_centres_f64(first[0].ptr(), N, S, centres.ptr(), _lib.stream_ptr()), "emd_stack_centres_f64")
        _lib.check(lib.emd_crop_stack_f32(x.data_ptr(), N, S, centres.ptr(), 5, 0.0, out.ptr(), _lib.stream_ptr()), "emd_crop_stack_f32")
        torch.cuda.synchronize()
        assert centres.intact() and out.intact() and not (out.view == SENTINEL).any()
        want = R.crop_stack(x.cpu().numpy(), centres.f64().reshape(N, 2).cpu().numpy(), 5)
        assert np.array_equal(out.view.reshape(N, 5, 5).cpu().numpy(), want)


# ---- the sign -----------------------------------------------------------------------------------------------------------------------

def test_the_crops_of_a_shifted_series_coincide():
    field, st = sign_inputs()
    offs = np.array(SIGN_OFFSETS, np.float64)
    shifts = R.chain_shifts(st)
    e = float(np.abs(shifts - np.diff(offs, axis=0)).max())
    print(f"sign: the restatement against the offsets' differences {e:.3e} (<= 1e-9)")
    assert e <= 1e-9                                                        # before the GPU is touched
    crops, centres = exitwave.align(up(st), side=32)
    assert crops.is_cuda and crops.dtype == torch.float32 and tuple(crops.shape) == (4, 32, 32) and tuple(centres.shape) == (4, 2)
    # image k shows the field displaced by offset k, so centre_k - offset_k is one point of the field: 48 - mean(offsets)
    c = 48.0 - offs.mean(0)
    want = R.crop_stack(field[None], [c], 32)[0].astype(np.float64)
    for k in range(4):
        ek = R.rel_l2(crops[k].cpu().numpy().astype(np.float64), want)
        print(f"sign: crop {k} (centre {centres[k].tolist()}) against the crop of the unshifted field at {c.tolist()}: rel L2 {ek:.3e} (<= 1e-12)")
        assert ek <= 1e-12
    against = R.crop_stack(st, 2 * 32.0 - centres.cpu().numpy(), 32)        # the reference's sign: S/2 + mean - pos
    assert R.rel_l2(against[1], against[0]) > 1e-2                          # moves the crops apart


# ---- crop_stack ---------------------------------------------------------------------------------------------------------------------

CROP_CASES = [(16, 1), (16, 8), (32, 8), (64, 32), (33, 8), (16, 16), (64, 64)]


@pytest.mark.parametrize("case", CROP_CASES, ids=lambda c: f"{c[0]}to{c[1]}")
@pytest.mark.parametrize("pad_val", [0.0, 7.5])
def test_crop_stack(case, pad_val):
    S, side = case
    x = (synthetic_lq(1, 64, 64, seed=1300)[0, :S, :S, 0] + np.float32(0.25))[None].repeat(9, 0)
    x = (x * np.arange(1, 10, dtype=np.float32)[:, None, None]).astype(np.float32)   # nine different images
    h = S / 2
    centres = np.array([(h, h), (h + 0.25, h - 0.5), (h + 1.5, h + 2.25),          # inside: fractions 0, 0.25 and 0.5
                        (side / 2 - 1.25, h), (S - side / 2 + 0.5, h), (h, side / 2 - 2.0), (h + 0.25, S - side / 2 + 1.75),
                        (side / 2 - 1.5, side / 2 - 0.75), (S + 0.5 * side, S + 0.5 * side + 3.0)])   # the corner; all outside
    want = R.crop_stack(x, centres, side, pad_val)
    got = exitwave.crop_stack(up(x), up(centres), side, pad_val)             # centres on the device
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (9, side, side)
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(exitwave.crop_stack(x, centres, side, pad_val), want)      # numpy in, numpy out
    if float(h - side / 2).is_integer():                                    # an integer centre: a bitwise copy of the window
        o = int(h - side / 2)
        assert np.array_equal(want[0], x[0, o:o + side, o:o + side])
    assert (want[8] == np.float32(pad_val)).all() and not (want[0] == np.float32(pad_val)).any()
    if side == S:
        assert np.array_equal(got[0].cpu().numpy(), x[0])


# ---- end to end ---------------------------------------------------------------------------------------------------------------------

def series_bar(st, centres_bar):
    """The exit-wave bar plus the centres' bar times the largest bilinear gradient of the images: every crop is bitwise given its
    centre, and a centre within centres_bar on each of the two axes moves a bilinear sample by at most centres_bar times the largest
    difference of two neighbouring pixels per axis; taken relative to the root mean square of the images, as the wave bar is relative."""
    x = st.astype(np.float64)
    grad = max(np.abs(np.diff(x, axis=1)).max(), np.abs(np.diff(x, axis=2)).max())
    return wave_bar() + 2.0 * centres_bar * grad / np.sqrt((x ** 2).mean())


def numpy_chain(st, df, side, iters):
    centres = R.centres_of(R.chain_shifts(st), st.shape[-1])
    return ER.reconstruct(R.crop_stack(st, centres, side), df, ER.WAVELENGTH, ER.PX, 0.0, iters), centres


def test_reconstruct_series_against_the_numpy_chain_and_in_one_graph():
    side, iters = 32, 3
    st, df = shifted_series()
    st2, _ = shifted_series(tuple(SERIES_OFFSETS_2))
    check_conditions(restate(st[:-1], st[1:]), "series")
    check_conditions(restate(st2[:-1], st2[1:]), "series 2")
    want, centres = numpy_chain(st, df, side, iters)
    want2, _ = numpy_chain(st2, df, side, iters)
    assert want["ratio"] >= 0.2 and want2["ratio"] >= 0.2 and ER.rel_l2(want2["E"], want["E"]) > 1e-3
    bar = series_bar(st, shift_bar(64))
    x, d = up(st), up(df)
    E = exitwave.reconstruct_series(x, d, ER.WAVELENGTH, side, px=ER.PX, iterations=iters)
    e = ER.rel_l2(E.cpu().numpy(), want["E"])
    ec = float(np.abs(exitwave.align(x, side)[1].cpu().numpy() - centres).max())
    print(f"reconstruct_series: centres {ec:.3e} (bar {shift_bar(64):.3e}); E rel L2 {e:.3e}; bar {bar:.3e} (exit-wave bar {wave_bar():.3e})")
    assert E.is_cuda and tuple(E.shape) == (side, side) and ec <= shift_bar(64) and e <= bar
    En = exitwave.reconstruct_series(st, df, ER.WAVELENGTH, side, px=ER.PX, iterations=iters)
    assert isinstance(En, np.ndarray) and np.array_equal(En, E.cpu().numpy())
    # one graph, replayed on a differently shifted stack
    E2 = exitwave.reconstruct_series(up(st2), d, ER.WAVELENGTH, side, px=ER.PX, iterations=iters)
    sx = x.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = exitwave.reconstruct_series(sx, d, ER.WAVELENGTH, side, px=ER.PX, iterations=iters)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(E))
    sx.copy_(up(st2))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(E2)) and not torch.equal(bits(E2), bits(E))
    assert ER.rel_l2(E2.cpu().numpy(), want2["E"]) <= series_bar(st2, shift_bar(64))


def test_numpy_and_tensor_conventions():
    a, b = pair_inputs(16)
    n = exitwave.phase_correlate(a, b, return_response=True, return_surface=True)
    t = exitwave.phase_correlate(up(a), up(b), return_response=True, return_surface=True)
    assert all(isinstance(v, np.ndarray) and v.dtype == np.float64 for v in n) and all(v.is_cuda for v in t)
    assert all(np.array_equal(p, q.cpu().numpy()) for p, q in zip(n, t))
    one = exitwave.phase_correlate(a[1], b[1], window=True, return_response=True, return_surface=True)
    assert one[0].shape == (2,) and one[1].shape == () and one[2].shape == (16, 16)
    both = exitwave.phase_correlate(a, b, window=True)
    assert np.array_equal(both[1], one[0])
    crops, centres = exitwave.align(chain_inputs(3, 64))                    # side from largest_crop_side
    assert isinstance(crops, np.ndarray) and crops.shape == (3, 32, 32) and centres.shape == (3, 2)
    assert exitwave.largest_crop_side(centres, 64) == 32


if __name__ == "__main__":
    w, _ = yardstick()
    print(f"surfaces: the two float64 restatements' largest distance {w['surface']:.3e} (bar {FACTOR * w['surface']:.3e}); "
          f"shifts, responses, centres {w['shift']:.3e}; the half-pixel case alone: {w['surface_half']:.3e}, {w['shift_half']:.3e}")
