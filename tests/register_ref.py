"""The float64 numpy restatement of the registration of a focal series (emdenoise.exitwave; include/emdenoise.h "Registration of a
focal series"): ``cv2.phaseCorrelate`` with ``cv2.createHanningWindow``'s window, the chain of the shifts into cropping centres and
the bilinear sub-pixel crop, written from the formulas of the header and independent of the library.  OpenCV is not installed and is
not run: the formulas are the specification.

Two FFT back ends evaluate the same formulas, as in tests/exitwave_ref.py: ``numpy.fft`` and the plain recursive radix-2 transform of
tests/fft_ref.py; their distance is the yardstick of the surface's and the shifts' bars (tests/test_register_gpu.py)."""
import numpy as np

from tests.exitwave_ref import NumpyFFT, Radix2FFT, rel_l2   # noqa: F401  (the back ends are this module's too)


def hanning_1d(S):
    return 0.5 * (1 - np.cos(2 * np.pi * np.arange(S) / (S - 1)))


def hanning_window(S):
    """cv2.createHanningWindow((S, S), CV_64F): sqrt(w[y] w[x])."""
    w = hanning_1d(S)
    return np.sqrt(w[:, None] * w[None, :])


def surface(a, b, window=None, fft=NumpyFFT):
    """c = Re ifft2(P / |P|), P = F(a) conj F(b), 0 where |P| = 0, in fftshift order ((i + S/2) mod S on both axes)."""
    a, b = np.asarray(a, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    S = a.shape[-1]
    if window is not None:
        a, b = a * window, b * window
    P = fft.fft2(a) * np.conj(fft.fft2(b))
    m = np.abs(P)
    with np.errstate(invalid="ignore", divide="ignore"):
        R = np.where(m > 0, P / m, 0)
    c = fft.ifft2(R).real
    i = (np.arange(S) + S // 2) % S          # c_s[y][x] = c[(y + S/2) mod S][(x + S/2) mod S]
    return c[np.ix_(i, i)]


def peak_of(cs):
    """(row, col) of the largest value; on a tie the first in row-major order (numpy's argmax)."""
    return np.unravel_index(int(np.argmax(cs)), cs.shape)


def centroid(cs):
    """-> (dx, dy, response, cancellation = sum |v| / |sum v| over the clipped 5 x 5 window, margin = (peak - runner-up) / peak)."""
    S = cs.shape[0]
    py, px = peak_of(cs)
    sv = sx = sy = sa = 0.0
    for y in range(max(py - 2, 0), min(py + 2, S - 1) + 1):
        for x in range(max(px - 2, 0), min(px + 2, S - 1) + 1):
            v = float(cs[y, x])
            sv += v
            sx += float(x) * v
            sy += float(y) * v
            sa += abs(v)
    flat = np.sort(cs.ravel())
    margin = float((flat[-1] - flat[-2]) / flat[-1]) if flat[-1] > 0 else 0.0
    if sv == 0.0:
        return 0.0, 0.0, 0.0, np.inf, margin
    return S / 2 - sx / sv, S / 2 - sy / sv, sv, sa / abs(sv), margin


def phase_correlate(a, b, window=None, fft=NumpyFFT):
    """-> dict(shift (dx, dy), response, surface, cancellation, margin)."""
    cs = surface(a, b, window, fft)
    dx, dy, resp, cancel, margin = centroid(cs)
    return {"shift": np.array([dx, dy]), "response": resp, "surface": cs, "cancellation": cancel, "margin": margin}


def chain_shifts(stack, window=None, fft=NumpyFFT):
    """[N-1, 2]: the shifts of the pairs (k, k + 1)."""
    return np.stack([phase_correlate(stack[k], stack[k + 1], window, fft)["shift"] for k in range(len(stack) - 1)])


def centres_of(shifts, S):
    """pos_0 = 0, pos_k = pos_{k-1} + shift_{k-1}; m = (ascending sum of pos) / N; centre_k = (S/2 + pos_k) - m.  [N,2] = (x, y)."""
    N = len(shifts) + 1
    pos = [(0.0, 0.0)]
    for dx, dy in np.asarray(shifts, np.float64)[:, :2]:
        pos.append((pos[-1][0] + float(dx), pos[-1][1] + float(dy)))
    sx = sy = 0.0
    for x, y in pos:
        sx += x
        sy += y
    mx, my = sx / N, sy / N
    return np.array([((S / 2 + x) - mx, (S / 2 + y) - my) for x, y in pos])


def crop_stack(stack, centres, side, pad_val=0.0):
    """The bilinear crop, operation by operation in float64, rounded to float32 at the end."""
    stack = np.asarray(stack, np.float32)
    N, S = stack.shape[0], stack.shape[-1]
    out = np.empty((N, side, side), np.float32)
    for n in range(N):
        p = np.full((S + 2 * side + 4, S + 2 * side + 4), np.float32(pad_val), np.float64)
        o = side + 2                                                        # the image's origin inside the padded array
        p[o:o + S, o:o + S] = stack[n]
        x0, y0 = float(centres[n][0]) - side / 2, float(centres[n][1]) - side / 2
        ix, iy = int(np.floor(x0)), int(np.floor(y0))
        fx, fy = x0 - np.floor(x0), y0 - np.floor(y0)
        ix, iy = min(max(ix, -side - 1), S), min(max(iy, -side - 1), S)     # further out every tap is the pad value as well
        t = lambda j, k: p[o + iy + j:o + iy + j + side, o + ix + k:o + ix + k + side]
        v = (1 - fy) * ((1 - fx) * t(0, 0) + fx * t(0, 1)) + fy * ((1 - fx) * t(1, 0) + fx * t(1, 1))
        out[n] = v.astype(np.float32)
    return out


def largest_crop_side(centres, S, power_of_two=True):
    side = int(2 * min(min(x, y, S - x, S - y) for x, y in centres))
    return 2 ** int(np.log2(side)) if power_of_two else side


def fourier_shift(img, dx, dy):
    """img displaced by (+dx, +dy) pixels (circularly) through a phase ramp; the Nyquist terms are kept real for fractional shifts."""
    S = img.shape[-1]
    k = np.fft.fftfreq(S)
    ramp = np.exp(-2j * np.pi * (k[None, :] * dx + k[:, None] * dy))
    return np.fft.ifft2(np.fft.fft2(np.asarray(img, np.float64)) * ramp).real
