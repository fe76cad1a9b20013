"""The two size-selected launch rules that the op tests could not see into, without a GPU: which instance of the pointwise split32 GEMM
(csrc/gemm_split.hip, emd_debug_split32_plan) and which strip height of the rolling depthwise kernel (csrc/dw_misc.hip, emd_debug_dw_plan)
a shape gets.  Both hooks call the function the launcher itself calls.  The tables are written out by hand from the rules:

  split32 GEMM    nt = tiles(Cout, 128), tiles(n, t) = ceil(n / t).  256 x 128 tiles (512 threads) where tiles(M, 256) * nt >= 192 or
                  statistics are asked for; else 128 x 128 (256 threads) where tiles(M, 128) * nt >= 256 or the output is split32; else
                  128 x 64 (knob split_narrow).  Knob split_wide: 256 x 192 where tiles(M, 256) * tiles(Cout, 192) >= 256 and
                  tiles(Cout, 192) * 192 <= nt * 128, fp32 output without statistics only.
                  Rows: (M, Cin, Cout, flags) -> (kernel, tile rows, tile columns, threads, row tiles, column tiles, wide, steps ahead).
  depthwise       wg(t) = B * tiles(H, t) * tiles(W, 16) * tiles(Q, 16), Q = C / 4, or ceil32(C) / 4 for a split32 output.  16 rows where
                  H >= 64, or H >= 16 and wg(16) >= 1024; else 8, and 4 where wg(8) < 1024.  Knob dw_th: 4, 8, 16, 32.  REFLECT: 16 where
                  H >= 64, else 8.  XCD-contiguous tile order up to H * W = 128 * 128 (knob dw_xcd: 0 never, 2 always), never for REFLECT.
                  Rows: (kind, B, H, W, C) -> (strip height, xcd, workgroups, strips, channel blocks, Q).
"""
import ctypes as C

import pytest

from emdenoise import _lib

# kernel ids (include/emdenoise_dev.h)
S3_PLAIN, S2, PERSIST, S2_128, WIDE4W, WIDE8W, N64_L2, N128_L2, N256_L2, N64, N128, N256, WREG, DIRECT, S3 = range(1, 16)
OSPLIT, STATS = 1, 2
PLAIN, SPLIT, PRE, PRE_SPLIT, REFLECT, REFLECT_SPLIT, UP = range(7)
KNOB_DEFAULTS = {"split_narrow": 1, "split_wide": 0, "split_lead": 2, "split_variant": -1, "dw_th": 0, "dw_xcd": 1}


@pytest.fixture
def lib():
    h = _lib.load()
    yield h
    h.emd_debug_split_variant(-1)
    for k, v in KNOB_DEFAULTS.items():
        _lib.knob(k, v)


def gemm_plan(h, M, cin, cout, flags=0):
    out = (C.c_int * 8)(*[-1] * 8)
    k = h.emd_debug_split32_plan(M, cin, cout, flags, out)
    if k == 0:
        assert list(out) == [-1] * 8
        return 0
    assert k == out[0]
    return tuple(out)


def dw_plan(h, kind, B, H, W, Cc):
    out = (C.c_int * 6)(*[-1] * 6)
    th = h.emd_debug_dw_plan(kind, B, H, W, Cc, out)
    if th == 0:
        assert list(out) == [-1] * 6
        return 0
    assert th == out[0]
    return tuple(out)


def narrow(mt, nt):
    return (N64_L2, 128, 64, 256, mt, nt, 0, 2)


def small(mt, nt):
    return (N128_L2, 128, 128, 256, mt, nt, 0, 2)


def big(mt, nt):
    return (N256_L2, 256, 128, 512, mt, nt, 0, 2)


GEMM = [
    # Cout = 3076: 25 column tiles of 128, 49 of 64.  10 * 25 = 250 | 11 * 25 = 275 tiles of 128 rows; 7 * 25 = 175 | 8 * 25 = 200 of 256
    ((1280, 160, 3076, 0), narrow(10, 49)),
    ((1281, 160, 3076, 0), small(11, 25)),
    ((1792, 160, 3076, 0), small(14, 25)),
    ((1793, 160, 3076, 0), big(8, 25)),
    # tests/test_split_forms_gpu.py's three row prefixes
    ((1000, 48, 3076, 0), narrow(8, 49)),
    ((1400, 48, 3076, 0), small(11, 25)),
    ((2000, 48, 3076, 0), big(8, 25)),
    # Cout = 728 (graph D's middle flow): 6 column tiles.  42 * 6 = 252 | 43 * 6 = 258; 31 * 6 = 186 | 32 * 6 = 192
    ((5376, 728, 728, 0), narrow(42, 12)),
    ((5377, 728, 728, 0), small(43, 6)),
    ((7936, 728, 728, 0), small(62, 6)),
    ((7937, 728, 728, 0), big(32, 6)),
    ((1, 728, 728, 0), narrow(1, 12)),
    ((32768, 728, 728, 0), big(128, 6)),
    # a split32 output: never 128 x 64
    ((1, 48, 3076, OSPLIT), small(1, 25)),
    ((1000, 48, 3076, OSPLIT), small(8, 25)),
    ((1400, 48, 3076, OSPLIT), small(11, 25)),
    ((1792, 48, 3076, OSPLIT), small(14, 25)),
    ((2000, 48, 3076, OSPLIT), big(8, 25)),
    ((64, 64, 36, OSPLIT), small(1, 1)),
    # statistics: always 256 rows (one partial per 256 rows)
    ((1, 48, 3076, STATS), big(1, 25)),
    ((1000, 48, 3076, STATS), big(4, 25)),
    ((256, 64, 36, STATS), big(1, 1)),
    ((874, 96, 132, STATS), big(4, 2)),
    # what the entry refuses, and an empty batch
    ((1000, 48, 3076, OSPLIT | STATS), 0),
    ((0, 48, 3076, 0), 0),
    ((1000, 48, 3078, 0), 0),
    ((1000, 0, 3076, 0), 0),
    ((1000, 48, 3076, 4), 0),
    ((1 << 37, 48, 3076, 0), 0),                               # 2^29 row tiles x 25: the grid is refused
]

# every "tiles" comment of tests/test_split_gpu.py: (test, M, Cin, Cout) -> plan
CLAIMS = [
    ("full_size_identity d", 32 * 1024, 728, 728, big(128, 6)),          # "256-row tiles"
    ("full_size_identity d4", 4 * 1024, 728, 728, narrow(32, 12)),       # "128 x 64 tiles"
    ("full_size_identity d8", 8 * 1024, 728, 728, big(32, 6)),           # 32 * 6 = 192: "256 x 128 tiles"
    ("full_size_identity d1", 1024, 728, 728, narrow(8, 12)),
    ("two_steps_ahead 0", 16 * 1024, 728, 728, big(64, 6)),              # "256 x 128 tiles"
    ("two_steps_ahead 1", 4 * 1024, 728, 728, narrow(32, 12)),           # "128 x 64 tiles (the small-batch form)"
    ("two_steps_ahead 2", 2 * 1024, 96, 192, narrow(16, 3)),             # 16 * 2 = 32 < 256: "128 x 64 tiles"
    ("two_steps_ahead 3", 256, 32, 64, narrow(2, 1)),
    ("two_steps_ahead 4", 3 * 23 * 23, 64, 40, narrow(13, 1)),
    ("two_steps_ahead 5", 20 * 1024, 96, 192, small(160, 2)),            # 80 * 2 = 160 < 192; 160 * 2 = 320 >= 256: "128 x 128 tiles"
    ("wide_tiles 3, knob 0", 20 * 1024, 96, 192, small(160, 2)),
]
# the same test's cases under split_wide = 1: (M, Cin, Cout) -> plan ("64 x 4 tiles of 256 x 192", "a ragged last row tile", "two column tiles")
WIDE_CLAIMS = [
    ((16 * 1024, 728, 728), (WIDE8W, 256, 192, 512, 64, 4, 1, 0)),
    ((33 * 23 * 23, 728, 728), (WIDE8W, 256, 192, 512, 69, 4, 1, 0)),
    ((32 * 1024, 256, 384), (WIDE8W, 256, 192, 512, 128, 2, 1, 0)),
    ((20 * 1024, 96, 192), small(160, 2)),                               # 80 * 1 < 256: the knob selects nothing here
]

DW = [
    # H = 9 < 16: 8 rows, 4 where 8 leave fewer than 1024 workgroups.  Q = 250: 16 channel blocks; W = 17: 2 column blocks
    ((PLAIN, 15, 9, 17, 1000), (4, 1, 1440, 3, 16, 250)),               # wg(8) = 15 * 2 * 2 * 16 = 960
    ((PLAIN, 16, 9, 17, 1000), (8, 1, 1024, 2, 16, 250)),               # 1024
    ((PRE, 15, 9, 17, 1000), (4, 1, 1440, 3, 16, 250)),
    ((PRE, 16, 9, 17, 1000), (8, 1, 1024, 2, 16, 250)),
    # a split32 output: the padding quads have threads, Q = 1024 / 4 (here in the same 16 blocks)
    ((SPLIT, 15, 9, 17, 1000), (4, 1, 1440, 3, 16, 256)),
    ((SPLIT, 16, 9, 17, 1000), (8, 1, 1024, 2, 16, 256)),
    ((PRE_SPLIT, 16, 9, 17, 1000), (8, 1, 1024, 2, 16, 256)),
    ((SPLIT, 1, 1, 1, 4), (4, 1, 1, 1, 1, 8)),
    ((SPLIT, 1, 1, 1, 36), (4, 1, 1, 1, 1, 16)),
    ((SPLIT, 1, 1, 1, 68), (4, 1, 2, 1, 2, 24)),
    ((PLAIN, 1, 1, 1, 68), (4, 1, 2, 1, 2, 17)),
    # 16 <= H < 64: 16 rows from 1024 workgroups of 16 rows on.  wg(16) = 15 * 2 * 2 * 16 = 960 | 1024
    ((PLAIN, 15, 17, 17, 1024), (8, 1, 1440, 3, 16, 256)),
    ((PLAIN, 16, 17, 17, 1024), (16, 1, 1024, 2, 16, 256)),
    ((SPLIT, 15, 17, 17, 1024), (8, 1, 1440, 3, 16, 256)),
    ((SPLIT, 16, 17, 17, 1024), (16, 1, 1024, 2, 16, 256)),
    ((PRE, 16, 17, 17, 1024), (16, 1, 1024, 2, 16, 256)),
    ((PRE_SPLIT, 16, 17, 17, 1024), (16, 1, 1024, 2, 16, 256)),
    ((PLAIN, 64, 15, 17, 1024), (8, 1, 4096, 2, 16, 256)),              # H = 15: never 16 rows, however many workgroups
    # H = 63 | 64 | 65
    ((PLAIN, 1, 63, 17, 40), (4, 1, 32, 16, 1, 10)),
    ((PLAIN, 1, 64, 17, 40), (16, 1, 8, 4, 1, 10)),
    ((PLAIN, 1, 65, 17, 40), (16, 1, 10, 5, 1, 10)),
    ((SPLIT, 1, 65, 17, 40), (16, 1, 10, 5, 1, 16)),
    # graph D's 728-channel maps at 4, 16 and 32 images: 384 workgroups of 8 rows; 1536 of 8 (768 of 16); 1536 of 16
    ((SPLIT, 4, 32, 32, 728), (4, 1, 768, 8, 12, 184)),
    ((SPLIT, 16, 32, 32, 728), (8, 1, 1536, 4, 12, 184)),
    ((SPLIT, 32, 32, 32, 728), (16, 1, 1536, 2, 12, 184)),
    ((PLAIN, 16, 32, 32, 728), (8, 1, 1536, 4, 12, 182)),
    # dw_xcd: H * W = 16384 | 16512
    ((PLAIN, 1, 128, 128, 8), (16, 1, 64, 8, 1, 2)),
    ((PLAIN, 1, 129, 128, 8), (16, 0, 72, 9, 1, 2)),
    ((PRE_SPLIT, 1, 129, 128, 8), (16, 0, 72, 9, 1, 8)),
    # a grid that is no multiple of 8
    ((PLAIN, 1, 3, 3, 384), (4, 1, 6, 1, 6, 96)),
    ((PRE_SPLIT, 1, 3, 3, 384), (4, 1, 6, 1, 6, 96)),
    # REFLECT: its own rule, no 4-row strips, launch order
    ((REFLECT, 1, 63, 17, 40), (8, 0, 16, 8, 1, 10)),
    ((REFLECT, 1, 64, 17, 40), (16, 0, 8, 4, 1, 10)),
    ((REFLECT_SPLIT, 1, 63, 17, 40), (8, 0, 16, 8, 1, 16)),
    ((REFLECT_SPLIT, 1, 64, 17, 40), (16, 0, 8, 4, 1, 16)),
    ((REFLECT, 64, 32, 32, 1024), (8, 0, 64 * 4 * 2 * 16, 4, 16, 256)),  # 4096 workgroups of 16 rows would not make it 16
    ((REFLECT, 1, 3, 3, 384), (8, 0, 6, 1, 6, 96)),
    # the upsampling form follows dw_strip_height on the split32 quads
    ((UP, 1, 128, 128, 384), (16, 1, 384, 8, 6, 96)),
    ((UP, 4, 8, 8, 132), (4, 1, 24, 2, 3, 40)),
    ((UP, 16, 17, 17, 1024), (16, 1, 1024, 2, 16, 256)),
    # refused: no such kind, an empty batch, channels no multiple of 4, a grid beyond 2^31 - 1 workgroups
    ((7, 1, 8, 8, 8), 0), ((-1, 1, 8, 8, 8), 0), ((PLAIN, 0, 8, 8, 8), 0), ((PLAIN, 1, 8, 8, 6), 0), ((PLAIN, 1, 0, 8, 8), 0),
    ((PLAIN, 1 << 20, 1024, 1024, 8), 0),                               # 2^20 * 64 * 64 = 2^32 workgroups
]


def test_split32_plan_table(lib):
    for r, want in GEMM:
        assert gemm_plan(lib, *r) == want, r
    for name, M, ci, co, want in CLAIMS:
        assert gemm_plan(lib, M, ci, co) == want, name


def test_split32_tiles_cover_the_problem(lib):
    """Row tiles x column tiles is the grid: they are the ceilings of M and Cout over the tile the plan names."""
    for M in (1, 127, 128, 129, 1000, 1400, 2000, 5377, 7937, 17457):
        for co in (4, 36, 64, 68, 128, 132, 728, 3076):
            for flags in (0, OSPLIT, STATS):
                _, bm, bn, threads, mt, nt, _, _ = gemm_plan(lib, M, 64, co, flags)
                assert (mt, nt) == (-(-M // bm), -(-co // bn)) and threads == 2 * bm, (M, co, flags)


def test_split32_output_is_never_narrow_and_statistics_always_256_rows(lib):
    for M in (1, 200, 1000, 1280, 1792, 1793, 5376, 40000):
        for co in (4, 64, 728, 3076):
            assert gemm_plan(lib, M, 64, co, OSPLIT)[2] == 128, (M, co)
            assert gemm_plan(lib, M, 64, co, STATS)[:4] == (N256_L2, 256, 128, 512), (M, co)


def test_split32_plan_under_the_knobs(lib):
    _lib.knob("split_narrow", 0)
    assert gemm_plan(lib, 1000, 48, 3076) == small(8, 25)
    assert gemm_plan(lib, 1, 728, 728) == small(1, 6)
    assert gemm_plan(lib, 2000, 48, 3076) == big(8, 25)
    _lib.knob("split_narrow", 1)
    _lib.knob("split_lead", 1)
    assert gemm_plan(lib, 1000, 48, 3076) == (N64, 128, 64, 256, 8, 49, 0, 1)
    assert gemm_plan(lib, 1400, 48, 3076) == (N128, 128, 128, 256, 11, 25, 0, 1)
    assert gemm_plan(lib, 2000, 48, 3076) == (N256, 256, 128, 512, 8, 25, 0, 1)
    _lib.knob("split_lead", 2)
    for form, kernel, threads in ((1, WIDE8W, 512), (2, WIDE4W, 256)):
        _lib.knob("split_wide", form)
        wide = lambda mt, nt: (kernel, 256, 192, threads, mt, nt, form, 0)
        # Cout = 728: four tiles of 192 = 768 = 6 * 128.  64 * 4 = 256 | 63 * 4 = 252 (63 * 6 = 378 tiles of 256 x 128)
        assert gemm_plan(lib, 16384, 728, 728) == wide(64, 4)
        assert gemm_plan(lib, 16384 - 256 + 1, 728, 728) == wide(64, 4)
        assert gemm_plan(lib, 16384 - 256, 728, 728) == big(63, 6)
        # one column tile (Cout = 192 <= 256): 256 row tiles | 255
        assert gemm_plan(lib, 65536, 96, 192) == wide(256, 1)
        assert gemm_plan(lib, 65536 - 256, 96, 192) == big(255, 2)
        # 17 * 192 = 3264 > 25 * 128 = 3200 and 2 * 192 = 384 > 2 * 128: past the padded weight planes, never; Cout = 132, 260: inside them
        assert gemm_plan(lib, 65536, 48, 3076) == big(256, 25)
        assert gemm_plan(lib, 65536, 48, 200) == big(256, 2)
        assert gemm_plan(lib, 65536, 48, 132) == wide(256, 1)
        assert gemm_plan(lib, 65536, 48, 260) == wide(256, 2)
        # never with a split32 output or statistics
        assert gemm_plan(lib, 16384, 728, 728, OSPLIT) == big(64, 6)
        assert gemm_plan(lib, 16384, 728, 728, STATS) == big(64, 6)
        if form == 1:
            for (M, ci, co), want in WIDE_CLAIMS:
                assert gemm_plan(lib, M, ci, co) == want, (M, ci, co)
    _lib.knob("split_wide", 0)
    for r, want in GEMM:   # and the defaults are back
        assert gemm_plan(lib, *r) == want, r


def test_split32_plan_under_a_forced_variant(lib):
    """emd_debug_split_variant and the knob split_variant: one kernel per variant, 256-row tiles but for variant 2; the statistics
    epilogue and the split32 output exist in variants 3, 5, 6 (and 7 for the output) only -- anything else becomes 3."""
    v = lambda k, bm=256: (k, bm, 128, 2 * bm, -(-1000 // bm), 25, 0, 0)
    for variant, want in ((0, v(S2)), (1, v(S3_PLAIN)), (2, v(S2_128, 128)), (3, v(S3)), (4, v(S3)), (6, v(WREG)), (7, v(DIRECT)), (8, v(S3))):
        lib.emd_debug_split_variant(variant)
        assert gemm_plan(lib, 1000, 160, 3076) == want, variant
        lib.emd_debug_split_variant(-1)
        _lib.knob("split_variant", variant)
        assert gemm_plan(lib, 1000, 160, 3076) == want, variant
        _lib.knob("split_variant", -1)
    lib.emd_debug_split_variant(4)       # the persistent form: whole tiles of 256 rows, Cin >= 64
    assert gemm_plan(lib, 1024, 160, 3076) == (PERSIST, 256, 128, 512, 4, 25, 0, 0)
    assert gemm_plan(lib, 1024, 48, 3076) == (S3, 256, 128, 512, 4, 25, 0, 0)
    for variant, flags, want in ((2, STATS, S3), (2, OSPLIT, S3), (0, STATS, S3), (7, STATS, S3), (7, OSPLIT, DIRECT), (6, STATS, WREG),
                                 (6, OSPLIT, WREG), (4, OSPLIT, S3), (5, OSPLIT, N128_L2), (5, STATS, N256_L2)):
        lib.emd_debug_split_variant(variant)
        assert gemm_plan(lib, 1000, 160, 3076, flags)[0] == want, (variant, flags)
    lib.emd_debug_split_variant(-1)
    assert gemm_plan(lib, 1000, 160, 3076) == narrow(8, 49)


def test_dw_plan_table(lib):
    for r, want in DW:
        assert dw_plan(lib, *r) == want, r


def test_dw_th_forces_four_heights_and_nothing_else(lib):
    shape = (16, 17, 17, 1024)          # the rule: 16 rows, 1024 workgroups
    forced = {4: (4, 1, 2560, 5, 16, 256), 8: (8, 1, 1536, 3, 16, 256), 16: (16, 1, 1024, 2, 16, 256), 32: (32, 1, 512, 1, 16, 256)}
    for th, want in forced.items():
        _lib.knob("dw_th", th)
        for kind in (PLAIN, SPLIT, PRE, PRE_SPLIT, UP):
            assert dw_plan(lib, kind, *shape) == want, (th, kind)
        assert dw_plan(lib, PLAIN, 1, 5, 3, 8) == (th, 1, -(-5 // th), -(-5 // th), 1, 2)
        # the REFLECT launcher has no knob
        assert dw_plan(lib, REFLECT, 1, 63, 17, 40) == (8, 0, 16, 8, 1, 10) and dw_plan(lib, REFLECT_SPLIT, 1, 64, 17, 40) == (16, 0, 8, 4, 1, 16)
    for other in (-4, 1, 2, 5, 12, 24, 64):
        _lib.knob("dw_th", other)
        for r, want in DW:
            assert dw_plan(lib, *r) == want, (other, r)
    _lib.knob("dw_th", 0)


def test_dw_xcd_knob(lib):
    at, above = (PLAIN, 1, 128, 128, 8), (PLAIN, 1, 129, 128, 8)
    for knob, want in ((1, (1, 0)), (0, (0, 0)), (2, (1, 1))):
        _lib.knob("dw_xcd", knob)
        assert (dw_plan(lib, *at)[1], dw_plan(lib, *above)[1]) == want, knob
        assert dw_plan(lib, UP, 1, 129, 128, 64)[1] == want[1] and dw_plan(lib, SPLIT, 1, 64, 256, 8)[1] == want[0]
        assert dw_plan(lib, REFLECT, 1, 8, 8, 8)[1] == 0 and dw_plan(lib, REFLECT_SPLIT, 1, 8, 8, 8)[1] == 0
        # the knob moves nothing else
        assert dw_plan(lib, *at)[2:] == (64, 8, 1, 2) and dw_plan(lib, *above)[2:] == (72, 9, 1, 2)
    _lib.knob("dw_xcd", 1)
