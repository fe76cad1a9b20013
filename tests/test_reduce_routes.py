"""CPU proof that every case of tests/test_reduce_routes_gpu.py runs the instance of the second-stage reduction it claims to.

The geometry of bn_stats_final / chan_reduce_final (CL channels x 256 / CL slab lanes per workgroup) is picked from the number of
partials per channel alone, by emd::reduce_final_cl (csrc/emd_common.hpp), exported as the host-only development hook
emd_debug_reduce_final_cl.  tests/reduce_route_cases.py restates each producer's partial count (one line each, with the source
line); here the library's own rule is asked which class that count selects.  A case list that no longer reaches a route -- after a
change of a tile height, a slab rule or the thresholds -- fails here, not silently on the GPU."""
import pytest

from emdenoise import _lib
from tests import reduce_route_cases as R


def cl_of(nslab):
    return _lib.load().emd_debug_reduce_final_cl(nslab)


def test_the_rule_itself():
    assert [cl_of(n) for n in (1, 127, 128, 1023, 1024, 1 << 20)] == [16, 16, 4, 4, 1, 1]


def test_reduce_slabs_restatement():
    """reduce_slabs against the workspace size the library reports (emd_chan_reduce_workspace_bytes = slabs * 2 * C doubles,
    csrc/bn_train.hip:604), at the pixel counts of the case list and around the 32 768-pixel clamp."""
    lib = _lib.load()
    for npix in sorted({c.H * c.W * (1 if c.images else c.B) for c in R.STATS + R.BWD} | {1, 63, 64, 65, 32767, 32768, 32769, 33123, 1 << 18}):
        assert lib.emd_chan_reduce_workspace_bytes(npix, 4) == R.reduce_slabs(npix) * 2 * 4 * 8, npix


@pytest.mark.parametrize("c", R.STATS, ids=R.case_id)
def test_statistics_case_selects_its_class(c):
    n = R.stat_nslab(c)
    assert cl_of(n) == c.cl, (c, n)
    if c.kind in ("conv", "deconv"):   # the workspace the library sizes holds every partial the epilogues write
        # (the deconv's four phases write 4 * ceil(B * H * W / 128) rows, more than ceil(4 * B * H * W / 128) on a ragged last tile)
        rows = n * (c.B if c.images else 1)
        M = 4 * c.B * c.H * c.W if c.kind == "deconv" else c.B * -(-c.H // c.stride) * -(-c.W // c.stride)
        assert _lib.load().emd_conv_stats_workspace_bytes(M, R.CO) >= rows * 2 * R.CO * 8, (c, rows)
    if c.images:   # per-image statistics need whole 128-row tiles per image (ops.conv_stats_supported; the deconv's rule on its input grid)
        assert c.kind == "stats" or (-(-c.H // c.stride) * -(-c.W // c.stride)) % 128 == 0


@pytest.mark.parametrize("c", R.BWD, ids=R.case_id)
def test_backward_case_selects_its_class(c):
    n = R.bwd_nslab(c)
    assert cl_of(n) == c.cl, (c, n)
    if c.kind == "dw":   # the workspace the library sizes holds the partials of either form (csrc/dw_bn_bwd.hip:374-379)
        per_image = R.nslab_dw(1, c.H, c.W, c.stride, c.rate, True)
        assert _lib.load().emd_dw3x3_bn_bwd_workspace_bytes(c.B, c.H, c.W, c.C) >= c.B * per_image * 2 * c.C * 8


# (producer, boundary) -> distance of the nearest count below the boundary that the producer's formula can give
STEP = {"deconv": 4}
REACH = {"conv": (128, 1024), "split32": (128, 1024), "deconv": (128, 1024), "stats": (128,), "dw_roll": (128, 1024),
         "dw_gather": (128, 1024), "slabs": (128,), "cout1": (128,), "accum": (128,)}


def test_both_sides_of_each_threshold_for_every_producer():
    """127 | 128 and 1023 | 1024 (the deconv's counts are multiples of four: 124 | 128, 1020 | 1024; the slab rule stops at 512)."""
    counts = {}
    for c in R.STATS:
        counts.setdefault(c.kind, set()).add(R.stat_nslab(c))
    for c in R.BWD:
        counts.setdefault(R.bwd_producer(c), set()).add(R.bwd_nslab(c))
    assert set(counts) == set(REACH)
    for prod, bounds in REACH.items():
        for b in bounds:
            assert b in counts[prod] and b - STEP.get(prod, 1) in counts[prod], (prod, b, sorted(counts[prod]))


def test_per_producer_edges():
    """Per producer: a ragged case in CL = 1 (where the producer reaches CL = 1), a per-image case with B >= 2, ill-conditioned
    channels in at least one statistics case, and 36 channels (a tail against CL = 16 and CL = 4; C % 64 != 0) for the backward ones."""
    for kind in ("conv", "split32", "deconv"):
        cs = [c for c in R.STATS if c.kind == kind]
        div = 256 if kind == "split32" else 128
        assert any(c.cl == 1 and (c.B * -(-c.H // c.stride) * -(-c.W // c.stride)) % div for c in cs), kind
        assert any(c.ill for c in cs), kind
        assert kind == "split32" or any(c.images and c.B >= 2 for c in cs), kind
    assert any(c.ill for c in R.STATS if c.kind == "stats") and any(c.images and c.B >= 2 for c in R.STATS if c.kind == "stats")
    slab = [c for c in R.STATS + R.BWD if c.kind in ("stats", "cout1") and c.H * c.W > 32768]
    assert all(c.H * c.W % max(64, -(-c.H * c.W // 512)) for c in slab) and {c.kind for c in slab} == {"stats", "cout1"}   # ragged last slab
    for prod in ("dw_roll", "dw_gather"):
        cs = [c for c in R.BWD if R.bwd_producer(c) == prod]
        assert any(c.images and c.B >= 2 for c in cs) and any(not c.images and c.B >= 2 for c in cs), prod
        assert {c.cl for c in cs if c.C == 36} >= ({16, 4} if prod == "dw_roll" else {4}), prod
        assert {c.wg for c in cs} == {True, False} and {c.double_bn for c in cs} == {True, False}, prod
        assert any(c.cl == 1 and ((c.H % 16 or c.W % 16) if prod == "dw_roll" else (c.H * c.W) % 512) for c in cs), prod
    assert {c.cl for c in R.BWD if c.C == 36} == {16, 4}


def test_every_instance_is_launched():
    """The nine bn_stats_final<FOLD, TRAIN, CL> and the three chan_reduce_final<CL> (the latter plain, with the per-channel step and
    accumulating) are each launched with one image list and, where the form allows it, with B >= 2 lists."""
    seen = set()
    for c in R.STATS:
        seen |= {(f, t, cl, min(b, 2)) for f, t, cl, b in R.stat_instances(c)}
    for cl in (16, 4, 1):
        assert {(0, 0, cl, 1), (0, 0, cl, 2), (0, 1, cl, 1), (0, 1, cl, 2), (1, 0, cl, 1)} <= seen, (cl, sorted(seen))
    assert not any(f and b > 1 for f, _, _, b in seen)          # the inference fold has no per-image form
    got = set()
    for c in R.BWD:
        got |= {(form, cl, min(b, 2)) for form, cl, b in R.bwd_instances(c)}
    for cl in (16, 4, 1):
        assert {("prep", cl, 1), ("prep", cl, 2), ("plain", cl, 1), ("plain", cl, 2)} <= got, (cl, sorted(got))
    assert {("accumulate", 16, 1), ("accumulate", 4, 1)} <= got     # (the accumulating entry takes at most 512 slabs: no CL = 1)


SWEEP = sorted(set(range(1, 41)) | {63, 64, 65, 127, 128, 129})


def test_size_functions_hold_every_partial_over_a_sweep_of_shapes():
    """The three size functions whose callers pass a workspace pointer and no size, against the producers' partial counts, for B in 1..4
    and H, W in 1..40 and around 64 and 128, stride 1 / 2 and rate 1 / 2 where the producer takes them (the listed cases above are 52
    points of this grid).  The transposed conv's four phases write 4 * ceil(m / 128) rows against the ceil(4 * m / 128) its M suggests:
    at most three more, which emd_conv_stats_workspace_bytes adds -- held here for every m of the grid, not only on paper."""
    lib = _lib.load()
    row = 2 * R.CO * 8
    n = 0
    for B in range(1, 5):
        for H in SWEEP:
            for W in SWEEP:
                for stride in (1, 2):       # conv_stats (1x1 at either stride; the dense 3x3 is the stride-1 count at any rate)
                    Ho, Wo = R.cdiv(H, stride), R.cdiv(W, stride)
                    have = lib.emd_conv_stats_workspace_bytes(B * Ho * Wo, R.CO)
                    assert have >= R.nslab_conv(B, H, W, stride, False) * row, (B, H, W, stride)
                    if (Ho * Wo) % 128 == 0:
                        assert have >= B * R.nslab_conv(B, H, W, stride, True) * row, (B, H, W, stride)
                m = B * H * W                # deconv_stats (H, W: the input grid)
                have = lib.emd_conv_stats_workspace_bytes(4 * m, R.CO)
                need = R.nslab_deconv(B, H, W, False)
                assert 0 <= need - R.cdiv(4 * m, 128) <= 3 and need * row <= have <= (need + 3) * row, (B, H, W)
                if (H * W) % 128 == 0:
                    assert have >= B * R.nslab_deconv(B, H, W, True) * row, (B, H, W)
                assert lib.emd_conv1x1_split32_stats_workspace_bytes(m, R.CO) == R.nslab_split32(B, H, W) * row, (B, H, W)
                have = lib.emd_dw3x3_bn_bwd_workspace_bytes(B, H, W, R.CO)
                for stride, rate in ((1, 1), (2, 1), (1, 2)):     # bn_backward_dw: rolling, strided gather, dilated gather
                    for images in (False, True):
                        rows = R.nslab_dw(B, H, W, stride, rate, images) * (B if images else 1)
                        assert have >= rows * row, (B, H, W, stride, rate, images)
                n += 1
    assert n == 4 * 46 * 46
