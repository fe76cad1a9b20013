"""CPU tests of emdenoise.diversity: the restatement of tests/diversity_ref.py against the distances themselves, the
pair schedule against hand-written lists, every refusal -- of the Python layer (before anything moves to a device) and of the C entry
points (before any launch) -- and the reason for the chain length, in the restatement's emulation of the device's product.  No GPU is
used."""
import ctypes as C

import numpy as np
import pytest

import emdenoise
from emdenoise import _lib, diversity
from tests import diversity_ref as R


def test_diversity_is_exported():
    assert "diversity" in emdenoise.__all__ and emdenoise.diversity is diversity
    assert (diversity.TILE, diversity.TILE_K, diversity.CHAIN) == (128, 32, 256)
    assert diversity.CHAIN % diversity.TILE_K == 0
    assert (diversity.OK, diversity.NONFINITE, diversity.BAD_INDEX) == (0, 1, 2)


@pytest.mark.parametrize("H,W", [(7, 5), (40, 33)])
def test_restatement_equals_the_distances_themselves(H, W):
    x = np.random.default_rng(H).standard_normal((H, W))
    want = R.brute_distances(x)
    got = R.row_distances(x)
    # n_i + n_j - 2 G loses up to (n_i + n_j) eps to cancellation: a few eps of the largest norm sum, per element
    bound = 8 * np.finfo(np.float64).eps * 2 * (x * x).sum(axis=1).max()
    assert np.abs(got - want).max() <= bound, (np.abs(got - want).max(), bound)
    assert np.array_equal(got, got.T)
    n = R.row_sq_norms(x)
    assert np.abs(n - (x * x).sum(axis=1)).max() <= 4 * np.finfo(np.float64).eps * n.max()
    # integer images: the int64 arithmetic, the float64 restatement and the differences agree exactly
    xi = np.random.default_rng(W).integers(0, 16, (H, W))
    assert np.array_equal(R.int_distances(xi), R.brute_distances(xi)) and np.array_equal(R.int_distances(xi), R.row_distances(xi))
    assert np.array_equal(R.row_sq_norms(xi), (xi * xi).sum(axis=1))


def test_restatement_ssd_of_an_image_with_itself_is_zero():
    x = R.images("uniform", 2, 40, 33)
    for dtype in (np.float32, np.float64):
        assert R.gram_ssd(x[0], x[0], dtype) == 0.0
        assert R.gram_ssd(x[0], x[1], dtype) > 0.0 and R.gram_ssd(x[0], x[1], dtype) == R.gram_ssd(x[1], x[0], dtype)
    xi = np.random.default_rng(1).integers(0, 16, (2, 9, 11))
    s, cnt = R.int_ssd(xi[0], xi[1])
    assert R.int_ssd(xi[0], xi[0]) == (0, 81) and s / cnt == R.gram_ssd(xi[0], xi[1])


def test_pair_schedule_by_hand():
    all4 = [(0, 1), (1, 2), (2, 3), (0, 2), (1, 3), (0, 3)]
    all5 = [(0, 1), (1, 2), (2, 3), (3, 4), (0, 2), (1, 3), (2, 4), (0, 3), (1, 4), (0, 4)]
    for n, full in ((4, all4), (5, all5)):
        for limit in (0, 1, len(full) - 1, len(full), len(full) + 1, 100, None):
            got = diversity.pair_schedule(n, limit)
            want = full if limit is None else full[:limit]
            assert got.dtype == np.int32 and got.shape == (len(want), 2)
            assert [tuple(r) for r in got.tolist()] == want
            assert got.size == 0 or (got.max() < n and got.min() >= 0)
    assert diversity.pair_schedule(5, None, first_offset=3).tolist() == [[0, 3], [1, 4], [0, 4]]
    assert diversity.pair_schedule(5, 2, first_offset=2).tolist() == [[0, 2], [1, 3]]
    for n in (0, 1):
        assert diversity.pair_schedule(n, 10).shape == (0, 2)
    assert diversity.pair_schedule(3, None, first_offset=7).shape == (0, 2)
    for call in (lambda: diversity.pair_schedule(-1, 3), lambda: diversity.pair_schedule(4, -3), lambda: diversity.pair_schedule(4, 3, 0),
                 lambda: diversity.pair_schedule(4.5, 3)):
        with pytest.raises(ValueError, match="^pair_schedule: "):
            call()


def test_python_refusals_name_the_function():
    img = np.zeros((8, 8), np.float32)
    stack = np.zeros((3, 8, 8), np.float32)
    pairs = np.zeros((2, 2), np.int32)
    bad = [
        (lambda: diversity.row_sq_norms(img.astype(np.float64)), "row_sq_norms"),                                # dtype
        (lambda: diversity.row_sq_norms(np.zeros(8, np.float32)), "row_sq_norms"),                               # rank
        (lambda: diversity.row_sq_norms([[1.0, 2.0]]), "row_sq_norms"),
        (lambda: diversity.row_sq_norms(np.zeros((8193, 1), np.float32)), "row_sq_norms"),                       # H over the limit
        (lambda: diversity.row_sq_norms(np.zeros((1, 32769), np.float32)), "row_sq_norms"),                      # W over the limit
        (lambda: diversity.row_sq_norms(np.zeros((0, 4), np.float32)), "row_sq_norms"),
        (lambda: diversity.row_distances(img.astype(np.int32)), "row_distances"),
        (lambda: diversity.row_distances(np.zeros((1, 2, 3, 4), np.float32)), "row_distances"),
        (lambda: diversity.row_distances(np.zeros((4097, 1), np.float32)), "row_distances"),                     # its own limit on H
        (lambda: diversity.row_distances(np.zeros((2, 1, 32769), np.float32)), "row_distances"),
        (lambda: diversity.gram_ssd(stack, stack.astype(np.float64)), "gram_ssd"),
        (lambda: diversity.gram_ssd(stack.astype(np.float16), stack), "gram_ssd"),
        (lambda: diversity.gram_ssd(stack, stack[:2]), "gram_ssd"),                                              # unequal shapes
        (lambda: diversity.gram_ssd(stack, np.zeros((3, 8, 9), np.float32)), "gram_ssd"),
        (lambda: diversity.gram_ssd(img, img[None]), "gram_ssd"),
        (lambda: diversity.gram_ssd(np.zeros((1, 8193, 1), np.float32), np.zeros((1, 8193, 1), np.float32)), "gram_ssd"),
        (lambda: diversity.gram_ssd(np.zeros(8, np.float32), np.zeros(8, np.float32)), "gram_ssd"),
        (lambda: diversity.gram_ssd_pairs(stack.astype(np.float64), pairs), "gram_ssd_pairs"),
        (lambda: diversity.gram_ssd_pairs(np.zeros((3, 1, 32769), np.float32), pairs), "gram_ssd_pairs"),
        (lambda: diversity.gram_ssd_pairs(stack, pairs.astype(np.int64)), "gram_ssd_pairs"),                     # pairs not int32
        (lambda: diversity.gram_ssd_pairs(stack, np.zeros((2, 3), np.int32)), "gram_ssd_pairs"),                 # not [P,2]
        (lambda: diversity.gram_ssd_pairs(stack, np.zeros(4, np.int32)), "gram_ssd_pairs"),
        (lambda: diversity.gram_ssd_pairs(stack, [[0, 1]]), "gram_ssd_pairs"),
        (lambda: diversity.gram_ssd_pairs(stack, np.zeros((2, 2), np.float32)), "gram_ssd_pairs"),
        (lambda: diversity.dataset_diversity(img), "dataset_diversity"),                                         # not a stack
        (lambda: diversity.dataset_diversity(stack.astype(np.float64)), "dataset_diversity"),
        (lambda: diversity.dataset_diversity(np.zeros((2, 8193, 2), np.float32)), "dataset_diversity"),
    ]
    for call, name in bad:
        with pytest.raises(ValueError, match=rf"^{name}: "):
            call()


def test_device_tensor_arguments_are_refused_before_any_launch():
    import torch

    with pytest.raises(ValueError, match="^row_distances: images are float32"):
        diversity.row_distances(torch.zeros(4, 4, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"^gram_ssd_pairs: pairs are int32 \[P,2\]"):
        diversity.gram_ssd_pairs(torch.zeros(2, 4, 4), torch.zeros(2, 2, dtype=torch.int64))
    with pytest.raises(ValueError, match="^gram_ssd: the two stacks have one shape"):
        diversity.gram_ssd(torch.zeros(2, 4, 4), torch.zeros(2, 4, 5))


def test_c_refusals_need_no_gpu():
    lib = _lib.load()
    M = 1 << 20
    null, x, o1, o2, ws, pr = (C.c_void_p(v) for v in (0, 16 * M, 64 * M, 128 * M, 256 * M, 8 * M))
    err = lib.emd_last_error

    # row norms
    assert lib.emd_row_sq_norms_f64(x, 2, 0, 8, o1, o2, null) == -1 and b"emd_row_sq_norms_f64" in err()
    assert lib.emd_row_sq_norms_f64(x, 2, 8, 0, o1, o2, null) == -1
    assert lib.emd_row_sq_norms_f64(x, 2, 8193, 8, o1, o2, null) == -1 and b"8192" in err()
    assert lib.emd_row_sq_norms_f64(x, 2, 8, 32769, o1, o2, null) == -1 and b"32768" in err()
    assert lib.emd_row_sq_norms_f64(x, -1, 8, 8, o1, o2, null) == -1
    assert lib.emd_row_sq_norms_f64(x, 65536, 8, 8, o1, o2, null) == -1
    for args in ((null, o1, o2), (x, null, o2), (x, o1, null)):
        assert lib.emd_row_sq_norms_f64(args[0], 2, 8, 8, args[1], args[2], null) == -1 and b"null" in err()
    assert lib.emd_row_sq_norms_f64(x, 2, 8, 8, x, o2, null) == -1 and b"overlap" in err()                  # norms on x
    assert lib.emd_row_sq_norms_f64(x, 2, 8, 8, o1, C.c_void_p(16 * M + 8), null) == -1 and b"overlap" in err()
    assert lib.emd_row_sq_norms_f64(x, 2, 8, 8, o1, o1, null) == -1                                         # the two outputs
    assert lib.emd_row_sq_norms_f64(x, 2, 8, 8, C.c_void_p(64 * M + 4), o2, null) == -3
    assert lib.emd_row_sq_norms_f64(null, 0, 8, 8, null, null, null) == 0                                   # B = 0: no-op

    # distances
    need = lib.emd_row_distances_workspace_bytes(2, 40, 70)
    assert need > 0 and need % 256 == 0
    assert lib.emd_row_distances_workspace_bytes(2, 4097, 70) == 0 and lib.emd_row_distances_workspace_bytes(0, 40, 70) == 0
    assert lib.emd_row_distances_workspace_bytes(2, 40, 32769) == 0
    assert lib.emd_row_distances_f32(x, 2, 4097, 70, o1, ws, need, null) == -1 and b"4096" in err()
    assert lib.emd_row_distances_f32(x, 2, 40, 32769, o1, ws, need, null) == -1 and b"emd_row_distances_f32" in err()
    assert lib.emd_row_distances_f32(x, 2, 0, 70, o1, ws, need, null) == -1
    for args in ((null, o1, ws), (x, null, ws), (x, o1, null)):
        assert lib.emd_row_distances_f32(args[0], 2, 40, 70, args[1], args[2], need, null) == -1 and b"null" in err()
    assert lib.emd_row_distances_f32(x, 2, 40, 70, o1, ws, need - 8, null) == -1 and b"too small" in err()
    assert lib.emd_row_distances_f32(x, 2, 40, 70, o1, C.c_void_p(256 * M + 8), need, null) == -3
    assert lib.emd_row_distances_f32(x, 2, 40, 70, x, ws, need, null) == -1 and b"overlap" in err()         # D on x
    assert lib.emd_row_distances_f32(x, 2, 40, 70, o1, x, need, null) == -1 and b"overlap" in err()         # workspace on x
    assert lib.emd_row_distances_f32(x, 2, 40, 70, ws, ws, need, null) == -1                                # D on the workspace
    assert lib.emd_row_distances_f32(null, 0, 40, 70, null, null, 0, null) == 0

    # the pair statistic
    need = lib.emd_gram_ssd_workspace_bytes(3, 40, 70, 4)
    assert need > 0 and need % 256 == 0
    assert lib.emd_gram_ssd_workspace_bytes(3, 8193, 70, 4) == 0 and lib.emd_gram_ssd_workspace_bytes(3, 40, 70, 0) == 0
    assert lib.emd_gram_ssd_f64(x, 3, 8193, 70, pr, 4, o1, o2, ws, need, null) == -1 and b"8192" in err()
    assert lib.emd_gram_ssd_f64(x, 3, 40, 32769, pr, 4, o1, o2, ws, need, null) == -1 and b"emd_gram_ssd_f64" in err()
    assert lib.emd_gram_ssd_f64(x, 3, 40, 70, pr, -1, o1, o2, ws, need, null) == -1 and b"P" in err()
    assert lib.emd_gram_ssd_f64(x, 3, 40, 70, pr, (1 << 20) + 1, o1, o2, ws, need, null) == -1
    assert lib.emd_gram_ssd_f64(x, 3, 8192, 70, pr, 1 << 20, o1, o2, ws, need, null) == -1 and b"2^31" in err()   # P * tiles
    for args in ((null, pr, o1, o2, ws), (x, null, o1, o2, ws), (x, pr, null, o2, ws), (x, pr, o1, null, ws), (x, pr, o1, o2, null)):
        assert lib.emd_gram_ssd_f64(args[0], 3, 40, 70, args[1], 4, args[2], args[3], args[4], need, null) == -1 and b"null" in err()
    assert lib.emd_gram_ssd_f64(x, 3, 40, 70, pr, 4, o1, o2, ws, need - 8, null) == -1 and b"too small" in err()
    assert lib.emd_gram_ssd_f64(x, 3, 40, 70, pr, 4, o1, o2, C.c_void_p(256 * M + 8), need, null) == -3
    assert lib.emd_gram_ssd_f64(x, 3, 40, 70, pr, 4, C.c_void_p(64 * M + 4), o2, ws, need, null) == -3
    assert lib.emd_gram_ssd_f64(x, 3, 40, 70, pr, 4, x, o2, ws, need, null) == -1 and b"overlap" in err()   # ssd on the images
    assert lib.emd_gram_ssd_f64(x, 3, 40, 70, pr, 4, o1, pr, ws, need, null) == -1 and b"overlap" in err()  # status on the pairs
    assert lib.emd_gram_ssd_f64(x, 3, 40, 70, pr, 4, o1, o1, ws, need, null) == -1                          # the two outputs
    assert lib.emd_gram_ssd_f64(x, 3, 40, 70, pr, 4, ws, o2, ws, need, null) == -1                          # ssd on the workspace
    assert lib.emd_gram_ssd_f64(null, 3, 40, 70, null, 0, null, null, null, 0, null) == 0                   # P = 0: no-op
    assert lib.emd_gram_ssd_f64(null, 0, 40, 70, null, 4, null, null, null, 0, null) == 0                   # B = 0: no-op


def test_workspace_sizes_are_monotone():
    lib = _lib.load()
    last = 0
    for P in (1, 2, 7, 64, 1000, 100000):
        n = lib.emd_gram_ssd_workspace_bytes(9, 2048, 2048, P)
        assert n > last
        last = n
    last = 0
    for H in (1, 127, 128, 129, 1000, 2048, 8192):
        n = lib.emd_gram_ssd_workspace_bytes(9, H, 2048, 8)
        assert n > last or (H == 128 and n >= last)
        last = n
    last = 0
    for H in (1, 128, 129, 2048, 4096):
        n = lib.emd_row_distances_workspace_bytes(4, H, 64)
        assert n >= last and n > 0
        last = n
    # the parts: norms [B][H] doubles, the counts, a double per pair and upper tile, each rounded up to 256 bytes
    r256 = lambda n: (n + 255) // 256 * 256
    T = -(-300 // diversity.TILE)
    assert lib.emd_gram_ssd_workspace_bytes(5, 300, 77, 11) == r256(5 * 300 * 8) + r256(5 * 4) + r256(11 * T * (T + 1) // 2 * 8)
    assert lib.emd_row_distances_workspace_bytes(5, 300, 77) == r256(5 * 300 * 8) + r256(5 * 4)


def test_chains_of_CHAIN_columns_are_no_worse_than_float32_numpy():
    """Why the product is cut into chains: at 96 x 600 the device's arithmetic with chains of CHAIN columns must be no further from
    the float64 distances than the float32 restatement (numpy's float32 arithmetic, what the reference's script computes); one
    unbroken chain is measured beside it and printed."""
    x = R.images("uniform", 1, 96, 600, seed=7)[0]
    want = R.row_distances(x, np.float64)
    f32 = R.rel_l2(R.row_distances(x, np.float32), want)
    chained = R.rel_l2(R.device_distances(x, diversity.CHAIN), want)
    unbroken = R.rel_l2(R.device_distances(x, 1 << 30), want)
    print(f"relative L2 distance from float64 at 96 x 600: float32 numpy {f32:.3e}, chains of {diversity.CHAIN} {chained:.3e}, "
          f"one chain {unbroken:.3e}")
    assert chained <= f32, (chained, f32)
    assert chained <= unbroken, (chained, unbroken)
    # the chain boundaries are where the header puts them: a chain length >= W is the unbroken chain
    assert np.array_equal(R.chain_product(x[:8], 600), R.chain_product(x[:8], 4096))
