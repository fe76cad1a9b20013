"""The float64 numpy restatement of the refinement of crop centres and defocuses (emdenoise.exitwave.refine_params;
include/emdenoise.h "Candidate stacks and the refinement"): the compass search over ANY loss function
``loss(centres [N,2], defocus [N]) -> float``; ``recon_loss`` builds the library's from tests/register_ref.py's ``crop_stack`` and
tests/exitwave_ref.py's ``reconstruct``.  Every operation is a separate numpy float64 operation, as the device rounds them.

``refine_series`` is the series of the tests: frames of an object confined to the middle, drifted by whole pixels, and a seed near
the truth."""
import functools

import numpy as np

from tests import exitwave_ref as R
from tests import register_ref as G

NONFINITE = 1


def polls(N, anchor):
    """[(axis, k)] of parameter p = axis (N - 1) + j: axis 0 = x, 1 = y, 2 = defocus; the free images in ascending k."""
    free = [k for k in range(N) if k != anchor]
    return [(axis, k) for axis in range(3) for k in free]


def candidate(centres, defocus, steps, q, N, anchor):
    """The state with poll q applied: (centres, defocus), copies."""
    axis, k = polls(N, anchor)[q // 2]
    c, d = np.array(centres, np.float64), np.array(defocus, np.float64)
    step = np.float64(steps[1 if axis == 2 else 0])
    if axis == 2:
        d[k] = d[k] - step if q & 1 else d[k] + step
    else:
        c[k, axis] = c[k, axis] - step if q & 1 else c[k, axis] + step
    return c, d


def compass_search(loss, centres0, defocus0, steps0, anchor, rounds, choices=None):
    """-> dict(centres, defocus, best, loss0, history_losses [R,Q], history_choice [R], history_steps [R,2], states [R+1]: (centres,
    defocus) before every round and after the last, bests [R+1], status, moves).  ``choices``: replay these decisions (a device's own
    history_choice) instead of deciding; then ``loss`` may be None and the losses are not evaluated."""
    c, d = np.array(centres0, np.float64), np.array(defocus0, np.float64)
    steps = np.array(steps0, np.float64)
    N = len(d)
    Q = 6 * (N - 1)
    status, moves = 0, 0
    loss0 = np.float64(loss(c, d)) if loss is not None else np.float64("nan")
    best = loss0 if np.isfinite(loss0) else np.float64("inf")
    if loss is not None and not np.isfinite(loss0):
        status |= NONFINITE
    hl, hc, hs, states, bests = [], [], [], [(c.copy(), d.copy())], [best]
    for r in range(rounds):
        hs.append(steps.copy())
        if choices is None:
            l = np.array([loss(*candidate(c, d, steps, q, N, anchor)) for q in range(Q)], np.float64)
            finite = np.isfinite(l)
            if not finite.any():
                i = -2
            else:
                j = int(np.argmin(np.where(finite, l, np.inf)))             # the first of the smallest finite
                i = j if l[j] < best else -1
            hl.append(l)
        else:
            i = int(choices[r])
        if i == -2:
            status |= NONFINITE
        elif i == -1:
            steps = steps * np.float64(0.5)
        else:
            c, d = candidate(c, d, steps, i, N, anchor)
            if choices is None:
                best = hl[-1][i]
            moves += 1
        hc.append(i)
        states.append((c.copy(), d.copy()))
        bests.append(best)
    return {"centres": c, "defocus": d, "best": best, "loss0": loss0, "history_losses": np.array(hl), "history_choice": hc,
            "history_steps": np.array(hs), "states": states, "bests": bests, "status": status, "moves": moves}


def recon_loss(stack, wavelength, side, pad_val=0.0, **kw):
    """loss(centres, defocus) = the largest loss over the images of the restated reconstruction of the restated crops."""
    return lambda c, d: float(R.reconstruct(G.crop_stack(stack, c, side, pad_val), d, wavelength, **kw)["losses"].max())


def round_gaps(ref):
    """Per round (the relative distance of the two smallest candidate losses, that of the smallest from ``best`` before the round)."""
    out = []
    for l, best in zip(ref["history_losses"], ref["bests"]):
        a, b = np.sort(l)[:2]
        out.append(((b - a) / a, abs(a - best) / best))
    return out


@functools.lru_cache(maxsize=None)
def refine_series(N, S0, side, seed=0):
    """-> (frames [N,S0,S0] float32, true centres [N,2], true defocuses [N], seed centres, seed defocuses, anchor).  The frames are
    |P(wave, df_k)| of exitwave_ref.true_wave(S0) with wave - 1 under a Gaussian envelope of width side / 5, every frame but the anchor
    rolled by an integer drift in -2..2; the seed is the truth perturbed by -1..1 px and up to 4e-9.  Cached: do not write into it."""
    rng = np.random.default_rng(seed)
    anchor = N // 2
    df = R.series_defocuses(N)
    y, x = np.mgrid[:S0, :S0].astype(np.float64) - S0 / 2
    wave = 1.0 + (R.true_wave(S0) - 1.0) * np.exp(-(x * x + y * y) / (2.0 * (side / 5.0) ** 2))
    drift = rng.integers(-2, 3, size=(N, 2))
    drift[anchor] = 0
    frames = np.stack([np.roll(np.abs(R.propagate(wave, d, R.WAVELENGTH, R.PX)), (int(dy), int(dx)), (0, 1))
                       for d, (dx, dy) in zip(df, drift)]).astype(np.float32)
    centres = S0 / 2.0 + drift.astype(np.float64)
    c0 = centres + rng.uniform(-1.0, 1.0, size=(N, 2))
    d0 = df + rng.uniform(-4e-9, 4e-9, size=N)
    c0[anchor], d0[anchor] = centres[anchor], df[anchor]
    return frames, centres, df, c0, d0, anchor
