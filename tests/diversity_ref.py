"""numpy restatement of emdenoise.diversity (include/emdenoise.h, "Dataset diversity"), written from the formulas:

    n_i = sum_k x[i,k]^2        G[i,j] = sum_k x[i,k] x[j,k]        D[i,j] = n_i + n_j - 2 G[i,j] = |x_i - x_j|^2
    ssd(a, b) = mean((D(a) - D(b))^2)

``row_distances`` / ``gram_ssd`` evaluate them in one number format throughout (float64: the yardstick; float32: what numpy gives the
reference's script).  ``chain_product`` emulates the device's product, a float32 fused-multiply-add chain over k that is folded into a
float32 total every ``chain`` columns, and ``device_distances`` / ``device_ssd`` put the double norms and the double combination of
the header around it.  Nothing here is run by the library and the reference is not run."""
import numpy as np

LANES = 64


def brute_distances(x):
    """|x_i - x_j|^2 from the differences themselves, float64."""
    x = np.asarray(x, np.float64)
    d = x[:, None, :] - x[None, :, :]
    return (d * d).sum(axis=2)


def row_sq_norms(x):
    """[.., H] float64 in the device's order: lane l adds the squares of the columns l, l + 64, .. in turn; the 64 lanes are then
    added as an xor butterfly with the offsets 32, 16, .., 1."""
    x = np.asarray(x, np.float64)
    W = x.shape[-1]
    sq = np.zeros(x.shape[:-1] + (-(-W // LANES) * LANES,))
    sq[..., :W] = x * x
    sq = sq.reshape(x.shape[:-1] + (-1, LANES))
    v = np.zeros(x.shape[:-1] + (LANES,))
    for r in range(sq.shape[-2]):
        v = v + sq[..., r, :]
    lane = np.arange(LANES)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    return v[..., 0]


def nonfinite_count(x):
    return int((~np.isfinite(x)).sum())


def row_distances(x, dtype=np.float64):
    """The script's ``gram`` with every operation in ``dtype``."""
    x = np.asarray(x, dtype)
    n = (x * x).sum(axis=1)
    return n[:, None] + n[None, :] - dtype(2) * (x @ x.T)


def difference(a, b, dtype=np.float64):
    """D(a) - D(b) in ``dtype``."""
    return row_distances(a, dtype) - row_distances(b, dtype)


def gram_ssd(a, b, dtype=np.float64):
    d = difference(a, b, dtype)
    return (d * d).mean(dtype=dtype)


def chain_product(x, chain):
    """x x^T as the float32 chain acc = fmaf(x[i,k], x[j,k], acc) over ascending k, the accumulator added to a float32 total and
    cleared every ``chain`` columns (chain >= W: one unbroken chain) -> float32 [H,H].  The fused step is formed in double (the
    product of two float32 is exact there) and rounded to float32: equal to fmaf but for a double rounding on rare near-ties."""
    x = np.asarray(x, np.float32)
    H, W = x.shape
    xd = x.astype(np.float64)
    total = np.zeros((H, H), np.float32)
    for c0 in range(0, W, chain):
        acc = np.zeros((H, H), np.float32)
        for k in range(c0, min(c0 + chain, W)):
            acc = (acc.astype(np.float64) + np.multiply.outer(xd[:, k], xd[:, k])).astype(np.float32)
        total = total + acc
    return total


def device_distances(x, chain):
    """D as the device forms it: double norms, the chained float32 product, the combination in double rounded once to float32."""
    n = row_sq_norms(x)
    return ((n[:, None] + n[None, :]) - 2.0 * chain_product(x, chain).astype(np.float64)).astype(np.float32)


def rel_l2(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))


# ---- integer arithmetic (exact) and the test images

def int_distances(x):
    """D of an integer-valued image in int64."""
    xi = np.asarray(x).astype(np.int64)
    n = (xi * xi).sum(axis=1)
    return n[:, None] + n[None, :] - 2 * (xi @ xi.T)


def int_ssd(a, b):
    """(sum (D(a) - D(b))^2, H^2) in Python integers."""
    d = int_distances(a) - int_distances(b)
    return int((d * d).sum()), int(d.size)


KINDS = ("uniform", "poisson", "fringe")


def images(kind, B, H, W, seed=0):
    """float32 [B,H,W]: uniform [0,1); Poisson counts near 3000, the odd images 1.1 x the counts of the image before them (near-equal
    statistics: D(a) - D(b) is a small difference of large numbers); a smooth fringe pattern plus noise."""
    rng = np.random.default_rng([seed, H, W, KINDS.index(kind)])
    if kind == "uniform":
        return rng.random((B, H, W), dtype=np.float32)
    if kind == "poisson":
        x = rng.poisson(3000.0, (B, H, W)).astype(np.float32)
        x[1::2] = np.float32(1.1) * x[:-1:2][: x[1::2].shape[0]]
        return x
    if kind == "fringe":
        r, c = np.mgrid[0:H, 0:W].astype(np.float64)
        out = np.empty((B, H, W), np.float32)
        for b in range(B):
            out[b] = 0.5 + 0.4 * np.cos(0.07 * (1 + 0.1 * b) * r + 0.045 * c + 0.3 * b) + 0.05 * rng.standard_normal((H, W))
        return out
    raise ValueError(kind)
