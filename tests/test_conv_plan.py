"""The host side of the dense and transposed convolutions and of the pointwise ones on fp32 input (csrc/conv_entry.hip), without a GPU: which kernel a layer gets, on
which tiles and with which grid (emd_debug_conv_plan against a table written out by hand from the routing rules), that the predicates say
what the plan says, that a layer's route does not depend on the batch size, and every step of the entry points' argument checks with its
return code and message.

Table rows: (op, B, H, W, Cin, Cout, stride, rate, precision, flags, ldx, ldy) -> (route, tile rows, tile columns, threads, grid x, y, z,
launches, tpw, epilogue width, nt, form), or 0 where the entry refuses.  Rules, in short (M = B * Ho * Wo rows; tiles(n, t) = ceil(n / t)):
  fp32 input      128-row tiles; 64 columns where Cout <= 64 or tiles(M, 128) * tiles(Cout, 128) < 192, else 128; 256 threads; form = flat
                  (1x1, stride 1); the transposed conv is four launches.
  3x3 split32     conv3_pipe (8 x 32 pixel tiles, 64 columns, 512 threads) at stride 1, rate 1, no residual, H % 8 == 0, W % 32 == 0,
                  Cout <= 256, 9 * W * ldy < 2^31; else gemm_split_conv_kernel: 256 rows, 64 (Cout <= 64) or 128 columns, 512 threads.
  transposed      one launch: deconv_pipe where Cin % 32 == 0, H % 8 == 0, W % 32 == 0; else deconv4_split (a split32 output: <., true>).
  patch kernels   tpw = the largest of 8, 4, 2 that divides W / 32 and leaves 1024 workgroups; grid = (W / 32 / tpw * tiles(Cout, 64), H / 8,
                  B); epilogue 4 wide from four column tiles on (conv3_pipe), 1 (deconv_pipe).
"""
import ctypes as C

import pytest

from emdenoise import _lib

GEMM, GEMM_UP, CSPLIT, C3PIPE, DFOUR, DSPLIT, DHALF, DPIPE = range(1, 9)
CONV1, CONV3, DECONV, BWD, SCONV3, SDECONV, SFUSED = range(7)
RES, AFF2, OSPLIT, STATS, UP = (1 << i for i in range(5))
OK, E_INVALID, E_UNSUPPORTED, E_ALIGN = 0, -1, -2, -3

KNOB_DEFAULTS = {"conv3_pipe": 1, "deconv_direct": 3, "epi_width": 0, "sep_tpw": 0, "nt_mask": 7}


@pytest.fixture
def lib():
    h = _lib.load()
    yield h
    for k, v in KNOB_DEFAULTS.items():
        _lib.knob(k, v)


def row(op, B, H, W, cin, cout, stride=1, rate=1, flags=0, ldx=0, ldy=0, prec=3):
    return (op, B, H, W, cin, cout, stride, rate, prec, flags, ldx, ldy)


def plan(h, r):
    out = (C.c_int * 12)(*[-1] * 12)
    route = h.emd_debug_conv_plan(*r, out)
    if route == 0:
        assert list(out) == [-1] * 12
        return 0
    assert route == out[0]
    return tuple(out)


def gemm(bn, grid, flat=0, launches=1, route=GEMM):
    return (route, 128, bn, 256, grid, 1, 1, launches, 0, 0, 0, flat)


def csplit(bn, grid, route=CSPLIT, launches=1, bm=256, nt=1):
    return (route, bm, bn, 2 * bm, grid, 1, 1, launches, 0, 0, nt, 0)


def patch(route, gx, gy, gz, tpw, epi, osplit=0, launches=1, nt=1):
    return (route, 256, 64, 512, gx, gy, gz, launches, tpw, epi, nt, osplit)


# ---- graph D (machine_learning/denoiser.py) at [B, 512, 512, 1]: its dense, pointwise and transposed layers in the order of the graph.
# (The 728-channel separable layers run as depthwise + the pointwise split32 GEMM, whose entries are gemm_split.hip's.)
def graph_d(B):
    big = B == 32
    return [
        (row(CONV1, B, 256, 256, 128, 256, 2), gemm(128, B * 128 * 2)),                          # residual1: M = B * 128^2, two column tiles
        (row(CONV1, B, 128, 128, 256, 728, 2), gemm(128, B * 32 * 6)),                           # residual2
        (row(CONV1, B, 64, 64, 728, 728, 2), gemm(128, B * 8 * 6)),                              # residual3 (B = 4: 192 tiles, still 128 columns)
        (row(SCONV3, B, 32, 32, 728, 728, 1, 2), csplit(128, B * 4 * 6)),                        # D': a dilated dense ASPP branch
        (row(CONV1, B, 32, 32, 3640, 256), gemm(128, 512, 1) if big else gemm(64, 32 * 4, 1)),   # aspp_reduce
        (row(CONV1, B, 32, 32, 256, 256), gemm(128, 512, 1) if big else gemm(64, 32 * 4, 1)),    # residual2_d at 1/16 resolution
        (row(CONV1, B, 128, 128, 128, 256, flags=UP), gemm(128, B * 128 * 2, 1, route=GEMM_UP)),  #   and with the upsampled shift
        (row(SFUSED, B, 128, 128, 256, 256), patch(DPIPE, 4, 16, B, 4, 1) if big else patch(DPIPE, 16, 16, B, 1, 1)),   # deconv2to1
        (row(SFUSED, B, 256, 256, 128, 128), patch(DPIPE, 2, 32, B, 8, 1) if big else patch(DPIPE, 8, 32, B, 2, 1)),    # deconv1to0
    ]


# ---- graph X's decoder (misc_py/modified_Xception.py:538-621) at [8, 512, 512, 1]: fp32 input up to 32 x 32, split32 from 64 x 64 on
GRAPH_X = [
    (row(CONV1, 8, 8, 8, 32, 728), gemm(64, 4 * 12, 1)),
    (row(CONV3, 8, 8, 8, 728, 728, flags=AFF2), gemm(64, 4 * 12)),
    (row(DECONV, 8, 8, 8, 728, 728), gemm(64, 4 * 12, launches=4)),
    (row(CONV3, 8, 16, 16, 728, 512, flags=AFF2), gemm(64, 16 * 8)),
    (row(DECONV, 8, 16, 16, 512, 512), gemm(64, 16 * 8, launches=4)),
    (row(CONV3, 8, 32, 32, 512, 384, flags=AFF2), gemm(128, 64 * 3)),          # 64 x 3 = 192 tiles: 128 columns
    (row(DECONV, 8, 32, 32, 384, 384), gemm(128, 64 * 3, launches=4)),
    (row(SCONV3, 8, 64, 64, 384, 256, flags=AFF2), patch(C3PIPE, 8, 8, 8, 1, 4)),
    (row(SCONV3, 8, 64, 64, 256, 256, flags=AFF2 | OSPLIT), patch(C3PIPE, 8, 8, 8, 1, 4, 1)),
    (row(SFUSED, 8, 64, 64, 256, 256), patch(DPIPE, 8, 8, 8, 1, 1)),
    (row(SCONV3, 8, 128, 128, 256, 192, flags=AFF2), patch(C3PIPE, 12, 16, 8, 1, 1)),
    (row(SFUSED, 8, 128, 128, 192, 192, flags=OSPLIT), patch(DPIPE, 12, 16, 8, 1, 1, 1)),
    (row(SCONV3, 8, 256, 256, 192, 128, flags=AFF2), patch(C3PIPE, 4, 32, 8, 4, 1)),
    (row(SFUSED, 8, 256, 256, 128, 128), patch(DPIPE, 4, 32, 8, 4, 1)),
    (row(SCONV3, 8, 512, 512, 128, 64, flags=AFF2), patch(C3PIPE, 2, 64, 8, 8, 1)),
    (row(SCONV3, 8, 512, 512, 64, 64, flags=AFF2), patch(C3PIPE, 2, 64, 8, 8, 1)),
]
# ---- graph G's generator (misc_py/gan-infilling-100.py) at [4, 512, 512, 1]: a pointwise half that runs on fp32 input
GRAPH_G = [
    (row(CONV1, 4, 256, 256, 32, 64), gemm(64, 2048, 1)),                      # a stride-2 REFLECT block below the split32 GEMM's shapes
]
# ---- the training tower (32 x 32 maps) on an image pair: M = 2048
TOWER = [
    (row(CONV1, 2, 32, 32, 728, 728, flags=STATS), gemm(64, 16 * 12, 1)),
    (row(CONV3, 2, 32, 32, 728, 728, flags=STATS), gemm(64, 16 * 12)),
    (row(DECONV, 2, 32, 32, 256, 256, flags=STATS), gemm(64, 16 * 4, launches=4)),
    (row(BWD, 2, 64, 64, 728, 256), gemm(64, 16 * 4)),
]
C3 = row(SCONV3, 1, 8, 32, 32, 64)
DF = row(SFUSED, 1, 8, 32, 32, 64)
EDGES = [
    # fp32 input: N = 64 | 68; tiles128 = 191 | 192
    (row(CONV1, 32, 64, 64, 64, 64), gemm(64, 1024, 1)),
    (row(CONV1, 32, 64, 64, 64, 68), gemm(128, 1024, 1)),
    (row(CONV1, 191, 8, 16, 64, 128), gemm(64, 191 * 2, 1)),
    (row(CONV1, 192, 8, 16, 64, 128), gemm(128, 192, 1)),
    (row(CONV1, 1, 10, 13, 64, 68), gemm(64, 2 * 2, 1)),                       # M = 130
    (row(CONV1, 1, 10, 13, 64, 68, prec=1), gemm(64, 2 * 2, 1)),
    # conv3_pipe: N = 256 | 260, W = 32 | 24, H = 8 | 4, a residual, rate 2, stride 2, the pitch gate
    (C3, patch(C3PIPE, 1, 1, 1, 1, 1)),
    (row(SCONV3, 1, 8, 32, 32, 256), patch(C3PIPE, 4, 1, 1, 1, 4)),
    (row(SCONV3, 1, 8, 32, 32, 260), csplit(128, 3)),
    (row(SCONV3, 1, 8, 24, 32, 64), csplit(64, 1)),
    (row(SCONV3, 1, 4, 32, 32, 64), csplit(64, 1)),
    (row(SCONV3, 1, 8, 32, 32, 64, flags=RES), csplit(64, 1)),
    (row(SCONV3, 1, 8, 32, 32, 64, 1, 2), csplit(64, 1)),
    (row(SCONV3, 1, 8, 32, 32, 64, 2), csplit(64, 1)),
    (row(SCONV3, 1, 8, 32, 32, 64, ldy=7456536), patch(C3PIPE, 1, 1, 1, 1, 1)),
    (row(SCONV3, 1, 8, 32, 32, 64, ldy=7456544), csplit(64, 1)),               # 9 * 32 * ldy = 2^31 + ...
    (row(SCONV3, 65536, 8, 32, 32, 64), csplit(64, 65536)),                    # grid.z: B <= 65535
    # the transposed conv: four launches; one launch at Cin = 32 | 48, B = 65535 | 65536, a pitch deconv_pipe cannot address
    (row(SDECONV, 1, 8, 32, 32, 64), csplit(64, 1, launches=4)),
    (DF, patch(DPIPE, 1, 1, 1, 1, 1)),
    (row(SFUSED, 1, 8, 32, 48, 64), csplit(64, 1, DSPLIT)),
    (row(SFUSED, 1, 8, 32, 48, 64, flags=OSPLIT), csplit(64, 1, DFOUR)),
    (row(SFUSED, 1, 8, 24, 32, 132), csplit(128, 2, DSPLIT)),
    (row(SFUSED, 65535, 8, 32, 32, 64), patch(DPIPE, 1, 1, 65535, 1, 1)),
    (row(SFUSED, 65536, 8, 32, 32, 64), patch(DPIPE, 1, 1, 65535, 1, 1, launches=2)),
    (row(SFUSED, 1, 8, 32, 32, 64, ldx=4194304), 0),                           # H * W * ldx * 4 = 2^32
    (row(SFUSED, 1, 8, 32, 32, 64, ldy=1864136), 0),                           # 36 * W * ldy >= 2^31
    (row(SFUSED, 1, 8, 32, 32, 64, ldy=1864128), patch(DPIPE, 1, 1, 1, 1, 1)),
    (row(SFUSED, 4, 8, 64, 32, 64), patch(DPIPE, 2, 1, 4, 1, 1)),
]
# knob, value, row, plan
KNOBS = [
    ("conv3_pipe", 0, C3, csplit(64, 1)),
    ("conv3_pipe", 2, row(SCONV3, 1, 8, 32, 32, 260), patch(C3PIPE, 5, 1, 1, 1, 4)),
    ("conv3_pipe", 2, row(SCONV3, 1, 8, 32, 32, 1028), csplit(128, 9)),
    ("deconv_direct", 0, DF, csplit(64, 1, DFOUR)),
    ("deconv_direct", 1, DF, csplit(64, 1, DSPLIT)),
    ("deconv_direct", 2, DF, csplit(64, 2, DHALF, bm=128)),
    ("deconv_direct", 2, row(SFUSED, 1, 8, 32, 32, 64, flags=OSPLIT), csplit(64, 1, DFOUR)),
    ("deconv_direct", 0, row(SDECONV, 1, 8, 32, 32, 64), csplit(64, 1, launches=4)),
    ("epi_width", 4, C3, patch(C3PIPE, 1, 1, 1, 1, 4)),
    ("epi_width", 1, row(SCONV3, 1, 8, 32, 32, 256), patch(C3PIPE, 4, 1, 1, 1, 1)),
    ("epi_width", 4, DF, patch(DPIPE, 1, 1, 1, 1, 4)),
    ("epi_width", 1, DF, patch(DPIPE, 1, 1, 1, 1, 1)),
    ("sep_tpw", 2, row(SFUSED, 4, 8, 64, 32, 64), patch(DPIPE, 1, 1, 4, 2, 1)),
    ("sep_tpw", 2, row(SCONV3, 4, 8, 64, 32, 64), patch(C3PIPE, 1, 1, 4, 2, 1)),
    ("sep_tpw", 2, C3, patch(C3PIPE, 1, 1, 1, 1, 1)),                          # one tile in a row: 2 does not divide it
    ("sep_tpw", 1, row(SFUSED, 32, 256, 256, 128, 128), patch(DPIPE, 16, 32, 32, 1, 1)),
    ("nt_mask", 6, C3, patch(C3PIPE, 1, 1, 1, 1, 1, nt=0)),
    ("nt_mask", 6, row(SFUSED, 1, 8, 32, 48, 64), csplit(64, 1, DSPLIT, nt=0)),
    ("nt_mask", 3, C3, patch(C3PIPE, 1, 1, 1, 1, 1)),
]
TABLE = graph_d(32) + graph_d(4) + GRAPH_X + GRAPH_G + TOWER + EDGES


def test_plan_table(lib):
    for r, want in TABLE:
        assert plan(lib, r) == want, r


def test_plan_under_each_knob(lib):
    for name, value, r, want in KNOBS:
        _lib.knob(name, value)
        assert plan(lib, r) == want, (name, value, r)
        _lib.knob(name, KNOB_DEFAULTS[name])
    for r, want in TABLE:   # and the defaults are back
        assert plan(lib, r) == want, r


def test_predicates_agree_with_the_plan(lib):
    for (op, B, H, W, ci, co, stride, rate, prec, flags, ldx, ldy), _ in TABLE:
        if op == SFUSED and not ldx and not ldy:
            # the one launch is preferred wherever deconv_pipe takes the layer, else from 192 row tiles on
            p = plan(lib, row(SFUSED, B, H, W, ci, co))
            assert bool(lib.emd_deconv3x3s2_fused_preferred(B, H, W, ci, co)) == (p[0] == DPIPE or B * H * W >= 192 * 256)
            assert lib.emd_deconv3x3s2_fused_preferred(1, H, W, ci, co) == (p[0] == DPIPE)
    _lib.knob("deconv_direct", 1)
    assert not lib.emd_deconv3x3s2_fused_preferred(1, 8, 32, 32, 64) and lib.emd_deconv3x3s2_fused_preferred(192, 16, 16, 32, 64)


def test_the_route_of_a_layer_does_not_depend_on_the_batch_size(lib):
    """conv3_pipe and deconv_pipe sum in another order than their siblings: image b of a batch == the image alone."""
    kernel = lambda r: plan(lib, r)[0]
    assert kernel(row(SCONV3, 1, 64, 64, 384, 256)) == kernel(row(SCONV3, 32, 64, 64, 384, 256)) == C3PIPE
    assert kernel(row(SFUSED, 1, 128, 128, 256, 256)) == kernel(row(SFUSED, 32, 128, 128, 256, 256)) == DPIPE


# ---- argument checks: (parameter name, kind, a value that passes) in the order of the C signature; kind p: a pointer that is never
# dereferenced, t: a table of four of them, i: an integer, f: a float.  B = 0 / M = 0, so that a call that passes every check returns
# EMD_OK without a launch; the statistics entries have no empty batch: every probe of theirs fails a check.
P, Q, NUL = 4096, 8192, 0
T4 = (P, P, P, P)
_F32 = [("x", "p", P), ("ldx", "i", 64), ("whi", "p", P), ("wlo", "p", P), ("scale1", "p", P), ("shift1", "p", P), ("scale2", "p", NUL),
        ("shift2", "p", NUL), ("res", "p", NUL), ("ldres", "i", 64), ("y", "p", Q), ("ldy", "i", 64), ("B", "i", 0), ("H", "i", 8), ("W", "i", 8),
        ("Cin", "i", 64), ("Cout", "i", 64)]
_TAIL = [("act", "i", 1), ("precision", "i", 3), ("stream", "p", NUL)]
_STATS_HEAD = [a for a in _F32[:12] if a[0] not in ("scale2", "shift2", "res", "ldres")] + [("B", "i", 1)] + _F32[13:]
_STATS_TAIL = [("precision", "i", 3), ("images", "i", 0), ("mean", "p", P), ("var", "p", P), ("workspace", "p", NUL)]   # (no workspace: refused)
_TABLE = lambda sig: [(n, "t", T4) if n in ("whi", "wlo") else (n, k, v) for n, k, v in sig]
_SPLIT = [("xs", "p", P), ("ldx", "i", 64), ("whi", "p", P), ("wlo", "p", P), ("scale1", "p", P), ("shift1", "p", P), ("scale2", "p", NUL),
          ("shift2", "p", NUL), ("res", "p", NUL), ("ldres", "i", 64), ("y", "p", Q), ("ldy", "i", 64)]
_SDECONV = _TABLE(_SPLIT[:6]) + [("y", "p", Q), ("ldy", "i", 64), ("B", "i", 0), ("H", "i", 8), ("W", "i", 32), ("Cin", "i", 32), ("Cout", "i", 64),
                                ("act", "i", 1), ("out_split", "i", 0), ("stream", "p", NUL)]
SIGS = {
    "emd_conv1x1_f32": _F32 + [("stride", "i", 1)] + _TAIL,
    "emd_conv3x3_f32": _F32 + [("stride", "i", 1), ("rate", "i", 1)] + _TAIL,
    "emd_conv1x1_up_f32": _F32[:5] + [("up", "p", P), ("ldup", "i", 64), ("Hu", "i", 2), ("Wu", "i", 2)] + _F32[6:] + _TAIL,
    "emd_deconv3x3s2_f32": _TABLE(_F32[:6]) + _F32[10:] + _TAIL,
    "emd_conv1x1_s2_bwd_data_f32": [("dy", "p", P), ("ldd", "i", 64)] + _F32[2:6] + _F32[8:10] + [("dx", "p", Q), ("ldx", "i", 64)] + _F32[12:15] +
                                   [("Cout", "i", 64), ("Cin", "i", 64), ("precision", "i", 3), ("stream", "p", NUL)],
    "emd_conv1x1_stats_f32": _STATS_HEAD + [("stride", "i", 1)] + _STATS_TAIL + [("stream", "p", NUL)],
    "emd_conv1x1_stats_fold_f32": _STATS_HEAD + [("stride", "i", 1)] + _STATS_TAIL + [("fold", "p", NUL), ("stream", "p", NUL)],
    "emd_conv3x3_stats_f32": _STATS_HEAD + [("rate", "i", 1)] + _STATS_TAIL + [("stream", "p", NUL)],
    "emd_conv3x3_stats_fold_f32": _STATS_HEAD + [("rate", "i", 1)] + _STATS_TAIL + [("fold", "p", NUL), ("stream", "p", NUL)],
    "emd_deconv3x3s2_stats_f32": _TABLE(_STATS_HEAD) + _STATS_TAIL + [("stream", "p", NUL)],
    "emd_deconv3x3s2_stats_fold_f32": _TABLE(_STATS_HEAD) + _STATS_TAIL + [("fold", "p", NUL), ("stream", "p", NUL)],
    "emd_conv3x3_split32_f32": _SPLIT + [("B", "i", 0), ("H", "i", 8), ("W", "i", 32), ("Cin", "i", 64), ("Cout", "i", 64), ("stride", "i", 1),
                                         ("rate", "i", 1), ("act", "i", 1), ("out_split", "i", 0), ("stream", "p", NUL)],
    "emd_deconv3x3s2_split32_f32": _SDECONV,
    "emd_deconv3x3s2_fused_split32_f32": _SDECONV,
}
# the fp32 ladder: every message starts with "conv:", whatever the entry
LADDER = [
    ({"x": NUL}, E_INVALID, "conv: null pointer"),
    ({"y": NUL}, E_INVALID, "conv: null pointer"),
    ({"precision": 2}, E_INVALID, "conv: precision must be"),
    ({"wlo": NUL}, E_INVALID, "conv: the split-bf16 mode needs the lo weight plane"),
    ({"Cin": 0}, E_INVALID, "conv: bad channel counts"),
    ({"Cout": 0}, E_INVALID, "conv: bad channel counts"),
    ({"Cin": 6}, E_ALIGN, "conv: Cin and ldx must be multiples of 4, ldx >= Cin"),
    ({"ldx": 60}, E_ALIGN, "conv: Cin and ldx"),
    ({"ldy": 60}, E_INVALID, "conv: ldy/ldres smaller than Cout"),
    ({"ldy": 66}, E_ALIGN, "conv: Cout, ldy, ldres must be multiples of 4 and y, res 16-byte aligned"),
    ({"y": Q + 4}, E_ALIGN, "conv: Cout, ldy, ldres"),
    ({"scale1": P + 4}, E_ALIGN, "conv: scale/shift vectors must be 16-byte aligned"),
    ({"x": P + 4}, E_ALIGN, "conv: x and the weight planes must be 16-byte aligned"),
    ({"whi": P + 8}, E_ALIGN, "conv: x and the weight planes"),
    # precedence: the first failing step speaks
    ({"x": NUL, "precision": 2, "Cin": 6}, E_INVALID, "conv: null pointer"),
    ({"Cin": 6, "ldy": 60, "H": 0}, E_ALIGN, "conv: Cin and ldx"),
    ({"y": Q + 4, "scale1": P + 4, "x": P + 4}, E_ALIGN, "conv: Cout, ldy, ldres"),
]
AFFINE2 = [
    ({"scale2": P}, E_INVALID, "conv: scale2/shift2 must come together"),
    ({"res": P, "ldres": 60}, E_INVALID, "conv: ldy/ldres smaller than Cout"),
    ({"res": P + 4}, E_ALIGN, "conv: Cout, ldy, ldres"),
    ({"scale2": P, "shift2": P + 4}, E_ALIGN, "conv: scale/shift vectors"),
    ({"res": P, "scale2": P, "shift2": P}, OK, ""),
]
SHAPE = lambda who: [({"H": 0}, E_INVALID, who + ": bad shape"), ({"B": -1}, E_INVALID, who + ": bad shape"),
                     ({"W": 0, "x": P + 4}, E_ALIGN, "conv: x and the weight planes")]
STRIDE = lambda who: [({"stride": 3}, E_UNSUPPORTED, who + ": stride must be 1 or 2"), ({"stride": 0, "H": 0}, E_INVALID, who + ": bad shape")]
PLANE = lambda i, v: tuple(v if j == i else P for j in range(4))
PHASES = [({"whi": NUL}, E_INVALID, ": null weight table"),
          ({"whi": PLANE(2, NUL)}, E_INVALID, "conv: null pointer"),
          ({"wlo": PLANE(3, NUL)}, E_INVALID, "conv: the split-bf16 mode needs the lo weight plane"),
          ({"wlo": NUL}, E_INVALID, "conv: the split-bf16 mode needs the lo weight plane"),
          ({"wlo": PLANE(1, P + 8)}, E_ALIGN, "conv: x and the weight planes"),
          ({"whi": PLANE(3, NUL), "ldy": 60}, E_INVALID, "conv: ldy/ldres smaller than Cout")]       # phase 0's whole ladder comes first
STATS_F32 = lambda who, stats_who, img, img_fail: [c for c in LADDER if c[0] != {"wlo": NUL}] + [
    ({}, E_INVALID, stats_who + ": mean, var and an 8-byte aligned workspace are required"),          # (the passing values carry no workspace)
    ({"workspace": Q + 4}, E_INVALID, stats_who + ": mean, var and"),
    ({"workspace": Q, "mean": NUL}, E_INVALID, stats_who + ": mean, var and"),
    ({"B": 0}, E_INVALID, who + ": bad shape"),
    ({"B": 65536}, E_INVALID, who + ": bad shape"),
    ({"W": 0, "workspace": Q}, E_INVALID, who + ": bad shape"),
    ({"workspace": Q, "images": 1, **img_fail}, E_UNSUPPORTED, stats_who + ": per-image statistics need " + img + " % 128 == 0 (a 128-row tile"),
    ({"images": 1, **img_fail}, E_INVALID, stats_who + ": mean, var and"),
]
GENERIC = "emd_conv*_stats_f32"
FOLD = lambda who: [({}, E_INVALID, who + ": null fold block"), ({"x": NUL}, E_INVALID, who + ": null fold block")]
# the split32 ladder: "split32 conv" for the 3x3 and the transposed convs
SC = "split32 conv"
SPLIT_LADDER = lambda who: [
    ({"xs": NUL}, E_INVALID, who + ": null pointer"),
    ({"wlo": NUL}, E_INVALID, who + ": null pointer"),
    ({"ldx": 48}, E_ALIGN, who + ": xs 128-byte aligned, ldx a multiple of 32, >= ceil32(Cin)"),
    ({"xs": P + 64}, E_ALIGN, who + ": xs 128-byte aligned"),
    ({"scale1": P + 4}, E_ALIGN, who + ": weight planes and scale/shift vectors must be 16-byte aligned"),
    ({"whi": P + 8}, E_ALIGN, who + ": weight planes"),
    ({}, OK, ""),
]
SPLIT_AFFINE2 = lambda who: [
    ({"scale2": P}, E_INVALID, who + ": scale2/shift2 must come together"),
    ({"scale2": P, "shift2": P + 4}, E_ALIGN, who + ": weight planes"),
    ({"res": P, "scale2": P, "shift2": P}, OK, ""),
]
CONV_Y = [
    ({"Cin": 0}, E_INVALID, SC + ": 1 <= Cin <= 2048, Cout a multiple of 4"),
    ({"Cin": 2049, "ldx": 4096}, E_INVALID, SC + ": 1 <= Cin"),
    ({"Cout": 6}, E_INVALID, SC + ": 1 <= Cin"),
    ({"ldy": 60}, E_ALIGN, SC + ": ldy a multiple of 4, >= Cout; y 16-byte aligned"),
    ({"y": Q + 4}, E_ALIGN, SC + ": ldy a multiple of 4"),
    ({"out_split": 1, "ldy": 68}, E_ALIGN, SC + ": split32 output needs y 128-byte aligned, ldy a multiple of 32, >= ceil32(Cout)"),
    ({"out_split": 1, "y": Q + 64}, E_ALIGN, SC + ": split32 output needs"),
    ({"out_split": 1}, OK, ""),
    ({"xs": P + 64, "ldy": 60, "scale1": P + 4}, E_ALIGN, SC + ": xs 128-byte aligned"),
]
DECONV_SPLIT = lambda who: [c for c in SPLIT_LADDER(SC) if c[0] not in ({"wlo": NUL}, {"whi": P + 8})] + CONV_Y + [
    ({"whi": NUL}, E_INVALID, who + ": null weight table"),
    ({"wlo": NUL}, E_INVALID, who + ": null weight table"),
    ({"wlo": PLANE(2, NUL)}, E_INVALID, SC + ": null pointer"),
    ({"whi": PLANE(3, P + 8)}, E_ALIGN, SC + ": weight planes"),
    ({"H": 0}, E_INVALID, who + ": bad shape"),
    ({"B": -1, "whi": PLANE(1, NUL)}, E_INVALID, SC + ": null pointer"),
]
UPN, F3, BWDN, S3 = "emd_conv1x1_up_f32", "emd_conv3x3_f32", "emd_conv1x1_s2_bwd_data_f32", "emd_conv3x3_split32_f32"
FUSEDN = "emd_deconv3x3s2_fused_split32_f32"
PROBES = {
    "emd_conv1x1_f32": LADDER + AFFINE2 + SHAPE("emd_conv1x1_f32") + STRIDE("emd_conv1x1_f32") + [({}, OK, ""), ({"stride": 2}, OK, ""),
                                                                                                ({"wlo": NUL, "precision": 1}, OK, "")],
    F3: LADDER + AFFINE2 + SHAPE(F3) + STRIDE(F3) + [
        ({"rate": 0}, E_UNSUPPORTED, F3 + ": rate must be 1..31, and 1 when stride is 2"),
        ({"rate": 32}, E_UNSUPPORTED, F3 + ": rate must be"),
        ({"rate": 2, "stride": 2}, E_UNSUPPORTED, F3 + ": rate must be"),
        ({"rate": 2, "stride": 3}, E_UNSUPPORTED, F3 + ": stride must be 1 or 2"),
        ({"rate": 31}, OK, "")],
    UPN: [c for c in LADDER if "shift1" not in c[0]] + SHAPE(UPN) + [
        ({"scale2": P}, E_UNSUPPORTED, UPN + ": no second affine and no residual with an upsampled shift"),
        ({"res": P, "x": NUL}, E_UNSUPPORTED, UPN + ": no second affine"),
        ({"up": NUL}, E_INVALID, "conv: null pointer"),
        ({"up": P + 4}, E_ALIGN, "conv: scale/shift vectors must be 16-byte aligned"),     # `up` stands in shift1's place
        ({"Hu": 0}, E_INVALID, UPN + ": bad shape"),
        ({"ldup": 60}, E_ALIGN, UPN + ": ldup must be a multiple of 4, >= Cout"),
        ({"ldup": 66}, E_ALIGN, UPN + ": ldup must be"),
        ({"H": (1 << 20) + 1}, E_UNSUPPORTED, UPN + ": H, W <= 2^20, B < 2^23"),
        ({"Wu": 0, "ldup": 60, "H": 1 << 21}, E_INVALID, UPN + ": bad shape"),
        ({}, OK, "")],
    "emd_deconv3x3s2_f32": [c for c in LADDER if c[0] != {"wlo": NUL}] + SHAPE("emd_deconv3x3s2_f32") + [
        (ch, code, ("emd_deconv3x3s2_f32" if text.startswith(":") else "") + text) for ch, code, text in PHASES] + [({}, OK, "")],
    BWDN: [({"dy": NUL}, E_INVALID, "conv: null pointer"), ({"Cout": 6}, E_ALIGN, "conv: Cin and ldx"), ({"Cin": 6}, E_ALIGN, "conv: Cout, ldy, ldres"),
           ({"ldd": 60}, E_ALIGN, "conv: Cin and ldx"), ({"ldx": 60}, E_INVALID, "conv: ldy/ldres smaller than Cout"),
           ({"res": P, "ldres": 60}, E_INVALID, "conv: ldy/ldres"), ({"dx": Q + 4}, E_ALIGN, "conv: Cout, ldy, ldres"),
           ({"H": 0}, E_INVALID, BWDN + ": bad shape"), ({"res": Q}, OK, ""), ({}, OK, "")],
    "emd_conv1x1_stats_f32": STATS_F32("emd_conv1x1_stats_f32", GENERIC, "Ho * Wo", {"H": 9}) + [
        ({"stride": 3}, E_UNSUPPORTED, "emd_conv1x1_stats_f32: stride must be 1 or 2"),
        ({"workspace": Q, "images": 1, "H": 32, "W": 8, "stride": 2}, E_UNSUPPORTED, GENERIC + ": per-image statistics need Ho * Wo")],
    "emd_conv1x1_stats_fold_f32": FOLD("emd_conv1x1_stats_fold_f32"),
    "emd_conv3x3_stats_f32": STATS_F32("emd_conv3x3_stats_f32", GENERIC, "Ho * Wo", {"H": 9}) + [
        ({"rate": 32}, E_UNSUPPORTED, "emd_conv3x3_stats_f32: rate must be 1..31 (stride 1)"),
        ({"rate": 0, "workspace": Q + 4}, E_UNSUPPORTED, "emd_conv3x3_stats_f32: rate must be")],
    "emd_conv3x3_stats_fold_f32": FOLD("emd_conv3x3_stats_fold_f32"),
    "emd_deconv3x3s2_stats_f32": STATS_F32("emd_deconv3x3s2_stats_f32", "emd_deconv3x3s2_stats_f32", "H * W", {"H": 9}) + [
        (ch, code, ("emd_deconv3x3s2_stats_f32" if text.startswith(":") else "") + text) for ch, code, text in PHASES],
    "emd_deconv3x3s2_stats_fold_f32": FOLD("emd_deconv3x3s2_stats_fold_f32"),
    S3: SPLIT_LADDER(SC) + SPLIT_AFFINE2(SC) + CONV_Y + [
        ({"res": P + 4}, E_ALIGN, SC + ": res alignment"),
        ({"res": P, "ldres": 60}, E_ALIGN, SC + ": res alignment"),
        ({"H": 0}, E_INVALID, S3 + ": bad shape"),
        ({"stride": 3}, E_UNSUPPORTED, S3 + ": stride must be 1 or 2"),
        ({"rate": 32}, E_UNSUPPORTED, S3 + ": rate must be 1..31, and 1 when stride is 2"),
        ({"rate": 2, "stride": 2}, E_UNSUPPORTED, S3 + ": rate must be"),
        ({"B": -1, "stride": 3}, E_INVALID, S3 + ": bad shape")],
    "emd_deconv3x3s2_split32_f32": DECONV_SPLIT("emd_deconv3x3s2_split32_f32"),
    FUSEDN: DECONV_SPLIT(FUSEDN) + [
        # the one refusal behind the checks: the layer is deconv_pipe's, the pitch is beyond its 32-bit offsets -- before any launch
        ({"B": 1, "ldx": 4194304}, E_UNSUPPORTED, FUSEDN + ": this layer runs on the patch-resident kernel, whose in-image offsets are 32-bit"),
        ({"B": 1, "ldy": 1864136}, E_UNSUPPORTED, FUSEDN + ": this layer runs on the patch-resident kernel")],
}


def test_every_entry_has_probes():
    family = {n for n in _lib.SIGNATURES if n.startswith(("emd_conv1x1_", "emd_conv3x3_", "emd_deconv3x3s2_")) and n.endswith("_f32")}
    family -= {n for n in family if "cout1" in n or "cin1" in n or "wgrad" in n or n.startswith("emd_conv1x1_split32")}
    assert set(PROBES) == set(SIGS) == family


def call(h, keep, entry, change):
    sig = SIGS[entry]
    assert set(change) <= {a[0] for a in sig}, (entry, change)
    args = []
    for n, kind, v in sig:
        v = change.get(n, v)
        if kind == "t" and v:      # (one value: the same plane four times)
            keep.append((C.c_void_p * 4)(*(v if isinstance(v, tuple) else (v,) * 4)))
            v = C.cast(keep[-1], C.c_void_p)
        args.append(v if kind in "if" else v if isinstance(v, C.c_void_p) else C.c_void_p(v))
    fn = getattr(h, entry)
    args = [C.cast(a, t) if isinstance(a, C.c_void_p) and t is not C.c_void_p else a for a, t in zip(args, fn.argtypes)]
    return fn(*args)


@pytest.mark.parametrize("entry", sorted(SIGS))
def test_argument_checks(lib, entry):
    keep = []
    for change, code, text in PROBES[entry]:
        rc = call(lib, keep, entry, change)
        assert rc == code, (entry, change, rc, lib.emd_last_error())
        if code != OK:
            assert lib.emd_last_error().decode().startswith(text), (entry, change, lib.emd_last_error())


def test_fold_block_is_converted_before_or_after_the_ladder(lib):
    """A fold block with a null pointer inside: the transposed conv reports it before the common checks, the 1x1 and 3x3 entries after."""
    fold = _lib.BnTrainFold()
    keep = []
    bad = {"fold": C.addressof(fold), "x": NUL}
    assert call(lib, keep, "emd_deconv3x3s2_stats_fold_f32", bad) != OK and not lib.emd_last_error().decode().startswith("conv:")
    for entry in ("emd_conv1x1_stats_fold_f32", "emd_conv3x3_stats_fold_f32"):
        assert call(lib, keep, entry, bad) == E_INVALID and lib.emd_last_error().decode().startswith("conv: null pointer")
        assert call(lib, keep, entry, {"fold": C.addressof(fold)}) != OK and not lib.emd_last_error().decode().startswith("conv:")


def test_workspace_sizes(lib):
    assert lib.emd_conv_stats_workspace_bytes(1, 4) == (1 + 3) * 2 * 4 * 8           # three rows more: the transposed conv's four phases
    assert lib.emd_conv_stats_workspace_bytes(4 * 130, 8) == (5 + 3) * 2 * 8 * 8
    assert lib.emd_conv_stats_workspace_bytes(0, 8) == 0 and lib.emd_conv_stats_workspace_bytes(8, 0) == 0
