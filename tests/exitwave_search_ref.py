"""The float64 numpy restatement of the defocus search (emdenoise.exitwave.defocus_search; include/emdenoise.h "Candidates and the
defocus search"), over ANY loss function ``loss(increment) -> float``; ``recon_loss`` builds the one of the library
from tests/exitwave_ref.py's ``reconstruct``.  Every operation is a separate numpy float64 operation, as the device rounds them."""
import numpy as np

from tests import exitwave_ref as R

NONFINITE, UNFINISHED = 1, 2


def candidate_increments(lo, hi, C):
    """inc_c = lo + c ((hi - lo) / (C - 1)) for c < C - 1, inc_{C-1} = hi."""
    lo, hi = np.float64(lo), np.float64(hi)
    step = (hi - lo) / np.float64(C - 1)
    return np.array([lo + np.float64(c) * step for c in range(C - 1)] + [hi], np.float64)


def section_search(loss, lo, hi, C, rounds):
    """-> dict(increment, loss, history_increments [R,C], history_losses [R,C], argmins [R], brackets [R+1,2], status, steps)."""
    best_inc, best_loss, status, steps = np.nan, np.inf, 0, 0
    hi_, hl_, argmins, brackets = [], [], [], [(np.float64(lo), np.float64(hi))]
    for _ in range(rounds):
        inc = candidate_increments(*brackets[-1], C)
        l = np.array([loss(v) for v in inc], np.float64)
        hi_.append(inc)
        hl_.append(l)
        finite = np.isfinite(l)
        if not finite.any():
            status |= NONFINITE
            argmins.append(-1)
            brackets.append(brackets[-1])
            continue
        i = int(np.argmin(np.where(finite, l, np.inf)))                    # the first of the smallest
        if l[i] < best_loss:
            best_inc, best_loss = inc[i], l[i]
        argmins.append(i)
        brackets.append((inc[max(i - 1, 0)], inc[min(i + 1, C - 1)]))
        steps += 1
    return {"increment": best_inc, "loss": best_loss, "history_increments": np.stack(hi_), "history_losses": np.stack(hl_),
            "argmins": argmins, "brackets": np.array(brackets), "status": status, "steps": steps}


def plateau_seed(increments, losses):
    """(incr1, incr2, prev): incr2 at the first smallest loss, incr1 its neighbour (the only one at an end, else the one with the
    smaller loss, the left one on a tie)."""
    i = int(np.argmin(losses))
    n = len(increments)
    j = 1 if i == 0 else i - 1 if i == n - 1 else (i - 1 if losses[i - 1] <= losses[i + 1] else i + 1)
    return float(increments[j]), float(increments[i]), float(losses[i])


def plateau_search(loss, incr1, incr2, prev, max_steps):
    incr1, incr2, prev = np.float64(incr1), np.float64(incr2), np.float64(prev)
    done, status, steps, hi_, hl_ = False, 0, 0, [], []
    for _ in range(max_steps):
        inc = incr2 if done else np.float64(0.5) * (incr1 + incr2)
        l = np.float64(loss(inc))
        hi_.append(inc)
        hl_.append(l)
        if done:
            continue
        if not np.isfinite(l):
            status |= NONFINITE
            done = True
        elif l < prev:
            incr1, incr2, prev = incr2, inc, l
            steps += 1
        else:
            done = True
    if not done:
        status |= UNFINISHED
    return {"increment": incr2, "loss": prev, "history_increments": np.array(hi_), "history_losses": np.array(hl_), "status": status,
            "steps": steps}


def recon_loss(images, ramp, wavelength, **kw):
    """loss(increment) = the largest loss over the images of the restated reconstruction at increment * ramp."""
    ramp = np.asarray(ramp, np.float64)
    return lambda inc: float(R.reconstruct(images, np.float64(inc) * ramp, wavelength, **kw)["losses"].max())
