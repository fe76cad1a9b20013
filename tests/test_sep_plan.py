"""The host side of the fused separable convolution (csrc/sep_entry.hip), without a GPU: which kernel a layer gets and with which grid
(emd_debug_sep_plan against a table written out by hand from the routing rules), that the *_supported / *_preferred predicates say what
the plan says, and every step of the entry points' argument checks with its return code and message.

Table rows: (B, H, W, Cin, Cout, Cout2, stride, precision, flags) -> (route, waves, tpw, grid x, y, z, schedule, epilogue width, xcd, nt),
or 0 where no kernel takes the shape.  Tiles: sep_fused 8 x 16 pixels (4 x 16 on its 256-column tile), sep_pipe 8 x 32 with 8 waves,
8 x 16 with 4, 4 x 16 output pixels at stride 2, sep_pipe2 8 x 32.  tpw = the largest of 8, 4, 2 that divides the tiles of a row and
leaves 2048 workgroups (sep_fused and sep_pipe's 4-wave form) or 1024 (8 waves).  xcd = the grid's size is a multiple of 8.
"""
import ctypes as C

import pytest

from emdenoise import _lib

FUSED, WRES, WIDE, DUAL, GEN9, PIPE, PIPE2, CHUNK = range(1, 9)
REFLECT, RES, AFF2, OSPLIT, GEN, G9, GENRES, FOLD = (1 << i for i in range(8))
OK, E_INVALID, E_UNSUPPORTED, E_ALIGN = 0, -1, -2, -3

KNOB_DEFAULTS = {"sep_pipe": 1, "sep_pipe2": 0, "sep_pipe2_chunk": -1, "sep_gen_pipe": 0, "sep_mode": -1, "sep_nw": 0, "sep_ablate": 0,
                 "sep_tpw": 0, "sep_xcd": 1, "sep_wide": 1, "sep_wres": 1, "epi_width": 0, "nt_mask": 7}


@pytest.fixture
def lib():
    h = _lib.load()
    yield h
    for k, v in KNOB_DEFAULTS.items():
        _lib.knob(k, v)


def plan(h, row):
    out = (C.c_int * 10)(*[-1] * 10)
    route = h.emd_debug_sep_plan(*row, out)
    if route == 0:
        assert list(out) == [-1] * 10
        return 0
    assert route == out[0]
    return tuple(out)


# ---- graph D at [32, 512, 512, 1] (machine_learning/denoiser.py), in the order of the graph
GRAPH_D = [
    ((32, 512, 512, 64, 64, 0, 1, 3, G9), (GEN9, 4, 8, 4, 64, 32, 0, 0, 1, 1)),                # cnn0 -> cnn0_last from the image
    ((32, 512, 512, 64, 64, 0, 1, 3, GEN), (WRES, 4, 8, 4, 64, 32, 0, 0, 1, 1)),               #   the same from d
    ((32, 512, 512, 64, 128, 0, 2, 3, GENRES | AFF2), (PIPE, 8, 8, 2, 64, 32, 1, 1, 1, 0)),    # cnn0_strided + generated residual0
    ((32, 512, 512, 64, 128, 0, 2, 3, RES | AFF2), (PIPE, 8, 8, 2, 64, 32, 1, 1, 1, 0)),       #   with the residual tensor
    ((32, 256, 256, 128, 128, 0, 1, 3, 0), (PIPE, 4, 8, 2, 32, 32, 1, 1, 1, 0)),               # cnn1, cnn1_last
    ((32, 256, 256, 128, 128, 0, 2, 3, RES | AFF2), (PIPE, 8, 8, 1, 32, 32, 1, 1, 1, 0)),      # cnn1_strided + residual1
    ((32, 128, 128, 128, 256, 0, 1, 3, 0), (PIPE, 8, 2, 2, 16, 32, 0, 1, 1, 0)),               # cnn2
    ((32, 128, 128, 256, 256, 0, 1, 3, 0), (PIPE, 8, 2, 2, 16, 32, 0, 1, 1, 0)),               # cnn2_last
    ((32, 128, 128, 256, 256, 0, 1, 3, RES), (PIPE, 8, 2, 2, 16, 32, 1, 4, 1, 0)),             #   with a residual: 16-byte epilogue
    ((32, 128, 128, 256, 256, 0, 2, 3, RES | AFF2), (PIPE, 8, 2, 2, 16, 32, 1, 4, 1, 0)),      # cnn2_strided + residual2
    ((32, 64, 64, 256, 728, 0, 1, 3, 0), 0),                                                   # cnn3 and the 728-channel flow: split32 GEMMs
    ((32, 128, 128, 384, 256, 0, 1, 3, 0), 0),                                                 # deconv2_a: 256 columns stop at Cin = 256
    ((32, 128, 128, 256, 256, 0, 1, 3, RES | AFF2), (PIPE, 8, 2, 2, 16, 32, 1, 4, 1, 0)),      # deconv2_b + residual2_d
    ((32, 256, 256, 384, 128, 128, 1, 3, 0), (CHUNK, 8, 8, 1, 32, 32, 0, 1, 1, 0)),            # deconv1_a | residual1_d
    ((32, 256, 256, 128, 128, 0, 1, 3, RES | AFF2 | OSPLIT), (PIPE, 4, 8, 2, 32, 32, 1, 1, 1, 0)),   # deconv1_b -> split32
    ((32, 512, 512, 128, 64, 64, 1, 3, 0), (PIPE, 4, 8, 4, 64, 32, 1, 1, 1, 0)),               # deconv0_a | residual0_d
    ((32, 512, 512, 64, 64, 0, 1, 3, 0), (PIPE, 4, 8, 4, 64, 32, 1, 1, 1, 0)),                 # deconv0_b
    ((32, 512, 512, 64, 64, 0, 1, 3, FOLD | RES | AFF2), (PIPE, 4, 8, 4, 64, 32, 1, 1, 1, 0)),  #   with deconv_final folded in
]
# ---- graph G's generator at [4, 512, 512, 1] (misc_py/gan-infilling-100.py)
GRAPH_G = [
    ((4, 512, 512, 32, 64, 0, 1, 3, GEN | REFLECT), (WRES, 4, 4, 8, 64, 4, 0, 0, 1, 1)),       # a generated first layer
    ((4, 512, 512, 32, 64, 0, 2, 3, REFLECT), (PIPE, 8, 4, 4, 64, 4, 0, 1, 1, 0)),             # enc1
    ((4, 256, 256, 64, 128, 0, 2, 3, REFLECT), (PIPE, 8, 1, 8, 32, 4, 0, 1, 1, 0)),            # nin_down0
    ((4, 128, 128, 128, 256, 0, 2, 3, REFLECT), (PIPE, 8, 1, 4, 16, 4, 0, 1, 1, 0)),           # nin_down1
    ((4, 64, 64, 256, 768, 0, 2, 3, REFLECT), 0),                                              # nin_down2, nin_mid*, nin_up0: GEMMs
    ((4, 64, 64, 768, 256, 0, 1, 3, 0), 0),
    ((4, 128, 128, 256, 128, 0, 1, 3, 0), (PIPE, 4, 1, 8, 16, 4, 1, 1, 1, 0)),                 # nin_up1
    ((4, 256, 256, 128, 64, 0, 1, 3, 0), (PIPE, 4, 1, 16, 32, 4, 1, 1, 1, 0)),                 # nin_up2
    ((4, 256, 256, 64, 64, 0, 1, 3, REFLECT | RES), (PIPE, 4, 1, 16, 32, 4, 1, 1, 1, 0)),      # local*
    ((4, 512, 512, 64, 32, 0, 1, 3, 0), (PIPE, 4, 4, 8, 64, 4, 1, 1, 1, 0)),                   # up
    ((4, 512, 512, 32, 32, 0, 1, 3, REFLECT), (PIPE, 4, 4, 8, 64, 4, 1, 1, 1, 0)),             # last_sep
]
# ---- graph X's entry flow at [8, 512, 512, 1] (misc_py/modified_Xception.py); from 728 channels on it runs on the split32 GEMMs
GRAPH_X = [
    ((8, 256, 256, 64, 128, 0, 1, 3, 0), (PIPE, 4, 2, 8, 32, 8, 1, 1, 1, 0)),
    ((8, 256, 256, 128, 128, 0, 1, 3, 0), (PIPE, 4, 2, 8, 32, 8, 1, 1, 1, 0)),
    ((8, 256, 256, 128, 128, 0, 2, 3, RES), (PIPE, 8, 2, 4, 32, 8, 1, 1, 1, 0)),
    ((8, 128, 128, 128, 256, 0, 1, 3, 0), (PIPE, 8, 1, 4, 16, 8, 0, 1, 1, 0)),
    ((8, 128, 128, 256, 256, 0, 1, 3, 0), (PIPE, 8, 1, 4, 16, 8, 0, 1, 1, 0)),
    ((8, 128, 128, 256, 256, 0, 2, 3, RES), (PIPE, 8, 1, 4, 16, 8, 1, 4, 1, 0)),
    ((8, 64, 64, 256, 728, 0, 1, 3, 0), 0),
]
S1 = (2, 16, 64, 64, 64, 0, 1, 3, 0)          # the shape most knobs are shown on
D2 = (2, 16, 64, 128, 128, 128, 1, 3, 0)      # two outputs on the 256-column tile
EDGES = [
    ((1, 8, 32, 32, 128, 128, 1, 3, 0), (CHUNK, 8, 1, 1, 1, 1, 0, 1, 0, 0)),
    ((1, 8, 48, 32, 192, 0, 1, 3, 0), (WIDE, 4, 1, 3, 2, 1, 0, 0, 0, 1)),
    # W % 32 != 0: with a 4-wave instance sep_pipe, without one sep_fused
    ((2, 16, 48, 64, 64, 0, 1, 3, 0), (PIPE, 4, 1, 3, 2, 2, 1, 1, 0, 0)),
    ((2, 16, 48, 64, 128, 128, 1, 3, 0), (DUAL, 4, 1, 3, 4, 2, 0, 0, 1, 1)),
    ((2, 16, 48, 64, 256, 0, 1, 3, 0), (WIDE, 4, 1, 3, 4, 2, 0, 0, 1, 1)),
    ((2, 16, 40, 64, 64, 0, 1, 3, 0), 0),
    # Cout 64 / 68 / 128: 4 waves; 132 / 256: 8 waves on 8 x 32; 260: none; 132 from more than 256 channels: none
    (S1, (PIPE, 4, 1, 4, 2, 2, 1, 1, 1, 0)),
    ((2, 16, 64, 64, 68, 0, 1, 3, 0), (PIPE, 4, 1, 4, 2, 2, 1, 1, 1, 0)),
    ((2, 16, 64, 64, 128, 0, 1, 3, 0), (PIPE, 4, 1, 4, 2, 2, 1, 1, 1, 0)),
    ((2, 16, 64, 64, 132, 0, 1, 3, 0), (PIPE, 8, 1, 2, 2, 2, 0, 1, 1, 0)),
    ((2, 16, 64, 64, 256, 0, 1, 3, 0), (PIPE, 8, 1, 2, 2, 2, 0, 1, 1, 0)),
    ((2, 16, 64, 64, 256, 0, 1, 3, RES), (PIPE, 8, 1, 2, 2, 2, 1, 4, 1, 0)),
    ((2, 16, 64, 64, 260, 0, 1, 3, 0), 0),
    ((2, 16, 64, 288, 132, 0, 1, 3, 0), 0),
    ((2, 16, 64, 64, 66, 0, 1, 3, 0), 0),
    # precision 1: sep_fused only, and no resident weights
    ((2, 16, 64, 64, 64, 0, 1, 1, 0), (FUSED, 4, 1, 4, 2, 2, 0, 0, 1, 1)),
    ((2, 16, 64, 64, 128, 0, 1, 1, 0), (FUSED, 4, 1, 4, 2, 2, 0, 0, 1, 1)),
    ((2, 16, 64, 64, 192, 0, 1, 1, 0), (WIDE, 4, 1, 4, 4, 2, 0, 0, 1, 1)),
    # two outputs: 64 | 64 on 4 waves, 128 | 128 whole-chunk; H % 8 != 0: sep_fused's 4 x 16 tiles
    ((2, 16, 64, 128, 64, 64, 1, 3, 0), (PIPE, 4, 1, 4, 2, 2, 1, 1, 1, 0)),
    (D2, (CHUNK, 8, 1, 2, 2, 2, 0, 1, 1, 0)),
    ((2, 12, 64, 128, 128, 128, 1, 3, 0), (DUAL, 4, 1, 4, 3, 2, 0, 0, 1, 1)),
    ((2, 12, 64, 128, 64, 64, 1, 3, 0), 0),
    ((2, 16, 64, 128, 132, 64, 1, 3, 0), 0),
    # split32 output: 64 columns have no sep_pipe instance
    ((2, 16, 64, 64, 64, 0, 1, 3, OSPLIT), (WRES, 4, 1, 4, 2, 2, 0, 0, 1, 1)),
    ((2, 16, 64, 128, 64, 0, 1, 3, OSPLIT), (FUSED, 4, 1, 4, 2, 2, 0, 0, 1, 1)),
    ((2, 16, 64, 64, 128, 0, 1, 3, OSPLIT), (PIPE, 4, 1, 4, 2, 2, 1, 1, 1, 0)),
    # stride 2, generated residual
    ((2, 16, 64, 64, 128, 0, 2, 3, 0), (PIPE, 8, 1, 2, 2, 2, 0, 1, 1, 0)),
    ((2, 16, 64, 64, 256, 0, 2, 3, RES), (PIPE, 8, 1, 2, 2, 2, 1, 4, 1, 0)),
    ((2, 16, 48, 64, 128, 0, 2, 3, 0), 0),
    ((2, 16, 64, 64, 128, 0, 2, 3, GENRES), (PIPE, 8, 1, 2, 2, 2, 1, 1, 1, 0)),
    ((2, 16, 64, 64, 256, 0, 2, 3, GENRES), 0),
    ((2, 16, 64, 64, 36, 0, 2, 3, GENRES), 0),
    # fold, gen9, generated input
    ((2, 16, 48, 64, 64, 0, 1, 3, FOLD), (PIPE, 4, 1, 3, 2, 2, 1, 1, 0, 0)),
    ((2, 16, 48, 64, 128, 0, 1, 3, FOLD), 0),
    ((2, 16, 48, 32, 64, 0, 1, 3, G9), (GEN9, 4, 1, 3, 2, 2, 0, 0, 0, 1)),
    ((2, 16, 48, 128, 64, 0, 1, 3, G9), 0),
    ((2, 16, 48, 32, 64, 0, 1, 1, G9), 0),
    ((2, 16, 64, 64, 192, 0, 1, 3, GEN), 0),
]
# knob, value, row, plan
KNOBS = [
    ("sep_pipe", 0, S1, (WRES, 4, 1, 4, 2, 2, 0, 0, 1, 1)),
    ("sep_pipe", 0, D2, (DUAL, 4, 1, 4, 4, 2, 0, 0, 1, 1)),
    ("sep_pipe", 0, (2, 16, 64, 64, 128, 0, 2, 3, 0), 0),
    ("sep_pipe", 0, (2, 16, 48, 64, 64, 0, 1, 3, FOLD), 0),
    ("sep_pipe2", 1, D2, (PIPE2, 8, 1, 2, 2, 2, 0, 1, 1, 0)),
    ("sep_pipe2", 1, S1, (PIPE, 4, 1, 4, 2, 2, 1, 1, 1, 0)),
    ("sep_pipe2", 2, S1, (PIPE2, 8, 1, 2, 2, 2, 0, 1, 1, 0)),
    ("sep_pipe2", 2, (2, 16, 48, 64, 64, 0, 1, 3, 0), (PIPE, 4, 1, 3, 2, 2, 1, 1, 0, 0)),
    ("sep_pipe2_chunk", 0, D2, (PIPE, 8, 1, 2, 2, 2, 1, 1, 1, 0)),
    ("sep_pipe2_chunk", 1, D2, (CHUNK, 8, 1, 2, 2, 2, 0, 1, 1, 0)),
    ("sep_gen_pipe", 1, (2, 16, 64, 64, 64, 0, 1, 3, GEN), (PIPE, 4, 1, 4, 2, 2, 1, 1, 1, 0)),
    ("sep_mode", 0, S1, (PIPE, 4, 1, 4, 2, 2, 0, 1, 1, 0)),
    ("sep_mode", 1, (2, 16, 64, 64, 256, 0, 1, 3, 0), (PIPE, 8, 1, 2, 2, 2, 1, 1, 1, 0)),
    ("sep_mode", 0, D2[:4] + (64, 64) + D2[6:], (PIPE, 4, 1, 4, 2, 2, 1, 1, 1, 0)),     # two outputs have the one schedule
    ("sep_nw", 8, S1, (PIPE, 8, 1, 2, 2, 2, 0, 1, 1, 0)),
    ("sep_nw", 8, (2, 16, 48, 64, 64, 0, 1, 3, 0), (WRES, 4, 1, 3, 2, 2, 0, 0, 0, 1)),
    ("sep_nw", 8, (2, 16, 48, 64, 64, 0, 1, 3, FOLD), 0),
    ("sep_nw", 4, S1, (PIPE, 4, 1, 4, 2, 2, 1, 1, 1, 0)),
    ("sep_nw", 4, D2, (PIPE, 8, 1, 2, 2, 2, 1, 1, 1, 0)),
    ("sep_ablate", 1, D2, (PIPE, 8, 1, 2, 2, 2, 1, 1, 1, 0)),
    ("sep_tpw", 2, S1, (PIPE, 4, 2, 2, 2, 2, 1, 1, 1, 0)),
    ("sep_tpw", 4, S1, (PIPE, 4, 4, 1, 2, 2, 1, 1, 0, 0)),
    ("sep_tpw", 3, S1, (PIPE, 4, 1, 4, 2, 2, 1, 1, 1, 0)),
    ("sep_tpw", 2, D2, (CHUNK, 8, 2, 1, 2, 2, 0, 1, 0, 0)),
    ("sep_tpw", 2, (2, 16, 64, 64, 64, 0, 1, 1, 0), (FUSED, 4, 2, 2, 2, 2, 0, 0, 1, 1)),
    ("sep_xcd", 0, S1, (PIPE, 4, 1, 4, 2, 2, 1, 1, 0, 0)),
    ("sep_xcd", 0, (2, 16, 64, 64, 64, 0, 1, 1, 0), (FUSED, 4, 1, 4, 2, 2, 0, 0, 0, 1)),
    ("sep_wide", 0, (2, 16, 64, 64, 192, 0, 1, 3, 0), 0),
    ("sep_wide", 2, (2, 16, 64, 288, 132, 0, 1, 3, 0), (PIPE, 8, 1, 2, 2, 2, 0, 1, 1, 0)),
    ("sep_wide", 2, (2, 16, 48, 288, 132, 0, 1, 3, 0), (WIDE, 4, 1, 3, 4, 2, 0, 0, 1, 1)),
    ("sep_wres", 0, (2, 16, 64, 64, 64, 0, 1, 3, OSPLIT), (FUSED, 4, 1, 4, 2, 2, 0, 0, 1, 1)),
    ("epi_width", 4, S1, (PIPE, 4, 1, 4, 2, 2, 1, 4, 1, 0)),
    ("epi_width", 4, D2, (CHUNK, 8, 1, 2, 2, 2, 0, 4, 1, 0)),
    ("epi_width", 4, (2, 16, 48, 64, 64, 0, 1, 3, FOLD), (PIPE, 4, 1, 3, 2, 2, 1, 1, 0, 0)),   # one form
    ("epi_width", 4, (2, 16, 64, 64, 128, 0, 2, 3, GENRES), (PIPE, 8, 1, 2, 2, 2, 1, 1, 1, 0)),
    ("epi_width", 1, (2, 16, 64, 64, 256, 0, 1, 3, RES), (PIPE, 8, 1, 2, 2, 2, 1, 1, 1, 0)),
    ("nt_mask", 5, (2, 16, 64, 64, 64, 0, 1, 1, 0), (FUSED, 4, 1, 4, 2, 2, 0, 0, 1, 0)),
]
# two knobs: sep_pipe2's instances come in both epilogue widths only on the 256-column one-output tile
KNOB_PAIRS = [
    ({"sep_pipe2": 2, "epi_width": 4}, S1, (PIPE2, 8, 1, 2, 2, 2, 0, 1, 1, 0)),
    ({"sep_pipe2": 2, "epi_width": 4}, (2, 16, 64, 64, 256, 0, 1, 3, 0), (PIPE2, 8, 1, 2, 2, 2, 0, 4, 1, 0)),
    ({"sep_pipe2": 2}, (2, 16, 64, 64, 256, 0, 1, 3, RES), (PIPE2, 8, 1, 2, 2, 2, 0, 4, 1, 0)),
    ({"sep_gen_pipe": 1, "epi_width": 4}, (2, 16, 64, 64, 64, 0, 1, 3, GEN), (PIPE, 4, 1, 4, 2, 2, 1, 4, 1, 0)),
]
TABLE = GRAPH_D + GRAPH_G + GRAPH_X + EDGES


def test_plan_table(lib):
    for row, want in TABLE:
        assert plan(lib, row) == want, row


def test_plan_under_each_knob(lib):
    for name, value, row, want in KNOBS:
        _lib.knob(name, value)
        assert plan(lib, row) == want, (name, value, row)
        _lib.knob(name, KNOB_DEFAULTS[name])
    for knobs, row, want in KNOB_PAIRS:
        for k, v in knobs.items():
            _lib.knob(k, v)
        assert plan(lib, row) == want, (knobs, row)
        for k in knobs:
            _lib.knob(k, KNOB_DEFAULTS[k])
    for row, want in TABLE:   # and the defaults are back
        assert plan(lib, row) == want, row


def test_predicates_agree_with_the_plan(lib):
    for (B, H, W, ci, co, co2, stride, prec, flags), _ in TABLE:
        took = lambda fl, c2=0, s=stride: plan(lib, (B, H, W, ci, co, c2, s, 3, fl))
        if co2:
            p = took(0, co2)
            assert bool(lib.emd_sep3x3_dual_supported(H, W, ci, co, co2)) == (p != 0)
            # the one launch is preferred wherever sep_pipe (or its sep_pipe2 forms) takes it, and always for 64 | 64
            assert bool(lib.emd_sep3x3_dual_preferred(H, W, ci, co, co2)) == (p != 0 and (p[0] >= PIPE or max(co, co2) <= 64))
            assert bool(lib.emd_debug_sep_pipe2_chunk_covers(H, W, ci, co, co2)) == (p != 0 and p[0] == CHUNK)
            continue
        # the shape predicate does not know the form: a plain layer of the shape
        assert bool(lib.emd_sep3x3_fused_supported(H, W, ci, co, stride, 1)) == (took(0) != 0)
        assert not lib.emd_sep3x3_fused_supported(H, W, ci, co, stride, 2)
        if stride == 1:
            assert bool(lib.emd_sep3x3_fused_fold_supported(H, W, ci, co)) == (took(FOLD) != 0)
            assert bool(lib.emd_sep3x3_fused_gen9_supported(H, W, ci, co)) == (took(G9) != 0)
        else:
            assert bool(lib.emd_sep3x3_fused_s2_genres_supported(H, W, ci, co)) == (took(GENRES) != 0)


# ---- argument checks: (parameter name, kind, a value that passes) in the order of the C signature; B = 0, so that a call that
# passes every check returns EMD_OK without a launch.  P, Q: two pointers that are never dereferenced.
P, Q, NUL = 4096, 8192, 0
_FUSED = [("x", "p", P), ("ldx", "i", 64), ("dw", "p", P), ("whi", "p", P), ("wlo", "p", P), ("scale1", "p", P), ("shift1", "p", P),
          ("scale2", "p", NUL), ("shift2", "p", NUL), ("res", "p", NUL), ("ldres", "i", 64), ("y", "p", Q), ("ldy", "i", 64), ("B", "i", 0),
          ("H", "i", 16), ("W", "i", 32), ("Cin", "i", 64), ("Cout", "i", 64), ("act", "i", 1)]
_GEN = [("x", "p", P), ("ldx", "i", 1), ("gen_a", "p", P), ("gen_t", "p", P), ("gen_act", "i", 1)] + _FUSED[2:] + \
       [("precision", "i", 3), ("reflect", "i", 0), ("stream", "p", NUL)]
_S2_HEAD = [a if a[0] not in ("ldy", "ldres", "Cout") else (a[0], "i", 128) for a in _FUSED]
SIGS = {
    "emd_sep3x3_fused_f32": _FUSED + [("precision", "i", 3), ("stream", "p", NUL)],
    "emd_sep3x3_fused_reflect_f32": _FUSED + [("precision", "i", 3), ("stream", "p", NUL)],
    "emd_sep3x3_fused_out_f32": [a if a[0] not in ("ldx", "ldy", "ldres", "Cin", "Cout") else (a[0], "i", 128) for a in _FUSED] + [("stream", "p", NUL)],
    "emd_sep3x3_fused_gen_f32": _GEN,
    "emd_sep3x3_fused_gen9_f32": [("img", "p", P + 4), ("w9", "p", P + 4)] + _GEN[2:],     # img and w9 need no alignment
    "emd_sep3x3_fused_fold_f32": _FUSED[:11] + [("wfin", "p", P), ("z", "p", Q)] + _FUSED[13:] + [("stream", "p", NUL)],
    "emd_sep3x3_fused_s2_f32": _S2_HEAD + [("stream", "p", NUL)],
    "emd_sep3x3_fused_s2_reflect_f32": _S2_HEAD + [("stream", "p", NUL)],
    "emd_sep3x3_fused_s2_genres_f32": _S2_HEAD[:9] + [("img", "p", P), ("ldimg", "i", 1), ("img_stride", "i", 2), ("res_a", "p", P), ("res_t", "p", P),
                                                      ("res_act", "i", 1)] + _S2_HEAD[11:] + [("stream", "p", NUL)],
    "emd_sep3x3_dual_f32": [("x", "p", P), ("ldx", "i", 128), ("dw", "p", P), ("whi", "p", P), ("wlo", "p", P), ("scale1", "p", P), ("shift1", "p", P),
                            ("y", "p", Q), ("ldy", "i", 64), ("w2hi", "p", P), ("w2lo", "p", P), ("scale_b", "p", P), ("shift_b", "p", P),
                            ("y2", "p", Q + 4096), ("ldy2", "i", 64), ("B", "i", 0), ("H", "i", 16), ("W", "i", 32), ("Cin", "i", 128), ("Cout", "i", 64),
                            ("Cout2", "i", 64), ("act", "i", 1), ("stream", "p", NUL)],
}
F, S2N = "emd_sep3x3_fused_f32", "emd_sep3x3_fused_s2_f32"
SPAN = {"W": 1 << 22, "H": 8}   # 9 rows of 2^22 pixels of 64 floats reach 2^31
# one probe per step of the ladder: the arguments changed, the code, what the message must contain (the reporting name first)
COMMON = lambda who, out="ldy": [
    ({"dw": NUL}, E_INVALID, who + ": null pointer"),
    ({"scale2": P}, E_INVALID, who + ": scale2/shift2 pair"),
    ({"W": 0}, E_INVALID, who + ": bad shape"),
    ({"B": -1}, E_INVALID, who + ": bad shape"),
    ({"H": 12}, E_UNSUPPORTED, who + ": needs "),
    ({"B": 65536}, E_UNSUPPORTED, who + ": B > 65535"),
    (SPAN, E_UNSUPPORTED, who + ": 9 image rows of "),
    ({out: 62}, E_ALIGN, who + ": pixel strides"),
    ({"res": P, "ldres": 8}, E_ALIGN, who + ": pixel strides"),
    ({"scale1": P + 4}, E_ALIGN, who + ": pointers"),
    ({"res": P + 8}, E_ALIGN, who + ": pointers"),
    ({"scale2": P, "shift2": P + 4}, E_ALIGN, who + ": pointers"),
    ({"res": P, "scale2": P, "shift2": P}, OK, ""),
    ({}, OK, ""),
]
FUSED_ONLY = [
    ({"precision": 2}, E_INVALID, F + ": bad precision"),
    ({"wlo": NUL}, E_INVALID, F + ": the split-bf16 mode needs the lo plane"),
    ({"wlo": NUL, "precision": 1}, OK, ""),
    ({"Cout": 260, "ldy": 260}, E_UNSUPPORTED, F + ": needs H%8==0"),
    ({"ldx": 32}, E_ALIGN, F + ": pixel strides"),
    # precedence: the first failing step speaks
    ({"dw": NUL, "precision": 2, "H": 12}, E_INVALID, F + ": null pointer"),
    ({"precision": 2, "scale2": P, "H": 12}, E_INVALID, F + ": bad precision"),
    ({"H": 12, "B": 65536, "ldy": 62}, E_UNSUPPORTED, F + ": needs"),
    ({**SPAN, "ldy": 66, "y": Q + 4}, E_UNSUPPORTED, F + ": 9 image rows of the output"),
    ({"ldy": 62, "y": Q + 4}, E_ALIGN, F + ": pixel strides"),
]
PROBES = {
    F: COMMON(F) + FUSED_ONLY,
    "emd_sep3x3_fused_reflect_f32": COMMON(F) + FUSED_ONLY,     # reports as emd_sep3x3_fused_f32
    "emd_sep3x3_fused_out_f32": [c for c in COMMON(F) if c[0] != {"ldy": 62}] + [                  # so does this one, but for its own step
        ({"ldy": 132}, E_ALIGN, "emd_sep3x3_fused_out_f32: a split32 output needs"),
        ({"ldy": 62}, E_ALIGN, "emd_sep3x3_fused_out_f32: a split32 output needs"),     # its step comes before the pixel strides
        ({"ldy": 96}, E_ALIGN, F + ": pixel strides"),
        ({"y": Q + 64}, E_ALIGN, "emd_sep3x3_fused_out_f32: a split32 output needs"),
        ({"Cout": 68, "ldy": 96}, E_ALIGN, "emd_sep3x3_fused_out_f32: a split32 output needs"),
        ({"wlo": NUL}, E_INVALID, F + ": the split-bf16 mode needs the lo plane"),
        ({**SPAN, "y": Q + 64}, E_UNSUPPORTED, F + ": 9 image rows of the output"),
    ],
    "emd_sep3x3_fused_gen_f32": COMMON(F) + [
        ({"gen_a": NUL}, E_INVALID, "emd_sep3x3_fused_gen_f32: null gen_a / gen_t"),
        ({"gen_t": NUL, "dw": NUL}, E_INVALID, "emd_sep3x3_fused_gen_f32: null gen_a / gen_t"),
        ({"gen_a": P + 4}, E_INVALID, "emd_sep3x3_fused_gen_f32: gen_a / gen_t must be 16-byte aligned"),
        ({"gen_act": 3}, E_INVALID, "emd_sep3x3_fused_gen_f32: gen_a / gen_t must be 16-byte aligned"),
        ({"gen_act": 5, "ldy": 62}, E_ALIGN, F + ": pixel strides"),
        ({"ldx": 0}, E_ALIGN, F + ": pixel strides"),
        ({"ldx": 3}, OK, ""),                                   # a generated input's pitch is any number of floats
        ({"precision": 2}, E_INVALID, F + ": bad precision"),
        ({"Cout": 192, "ldy": 192, "ldres": 192}, OK, ""),      # (B == 0; with B > 0 there is no generated-input form above 128 columns)
        ({"Cout": 192, "ldy": 192, "ldres": 192, "B": 1}, E_UNSUPPORTED, "emd_sep3x3_fused_gen_f32: Cout > 128 has no generated-input form"),
    ],
    "emd_sep3x3_fused_gen9_f32": COMMON("emd_sep3x3_fused_gen9_f32") + [
        ({"img": NUL}, E_INVALID, "emd_sep3x3_fused_gen9_f32: null pointer"),
        ({"wlo": NUL}, E_INVALID, "emd_sep3x3_fused_gen9_f32: null pointer"),
        ({"gen_act": 2}, E_UNSUPPORTED, "emd_sep3x3_fused_gen9_f32: needs relu6 generation"),
        ({"reflect": 1}, E_UNSUPPORTED, "emd_sep3x3_fused_gen9_f32: needs relu6 generation"),
        ({"precision": 1}, E_UNSUPPORTED, "emd_sep3x3_fused_gen9_f32: needs relu6 generation"),
        ({"Cin": 128}, E_UNSUPPORTED, "emd_sep3x3_fused_gen9_f32: needs relu6 generation"),
        ({"gen_a": P + 4}, E_ALIGN, "emd_sep3x3_fused_gen9_f32: pointers (but img, w9) must be 16-byte aligned"),
        ({"img": P + 2, "w9": P + 6}, OK, ""),
    ],
    "emd_sep3x3_fused_fold_f32": COMMON("emd_sep3x3_fused_fold_f32", "ldx") + [
        ({"wfin": NUL}, E_INVALID, "emd_sep3x3_fused_fold_f32: null pointer"),
        ({"Cout": 128}, E_UNSUPPORTED, "emd_sep3x3_fused_fold_f32: needs H%8==0, W%16==0, Cin%32==0, Cout==64"),
        (SPAN, E_UNSUPPORTED, "emd_sep3x3_fused_fold_f32: 9 image rows of the input"),
        ({"W": 1 << 22, "H": 8, "ldx": 32, "Cin": 32, "ldres": 32}, OK, ""),   # the span is the input's and the residual's pitch, 2^31 / 2 here
        ({"W": 1 << 22, "H": 8, "ldx": 32, "Cin": 32, "ldres": 64}, E_UNSUPPORTED, "emd_sep3x3_fused_fold_f32: 9 image rows of the input"),
        ({"z": Q + 4}, E_ALIGN, "emd_sep3x3_fused_fold_f32: pointers must be 16-byte aligned"),
        ({"wfin": P + 4}, E_ALIGN, "emd_sep3x3_fused_fold_f32: pointers must be 16-byte aligned"),
    ],
    S2N: COMMON(S2N) + [
        ({"H": 1}, E_INVALID, S2N + ": bad shape"),
        ({"W": 48}, E_UNSUPPORTED, S2N + ": needs H%8==0, W%32==0"),
        ({"Cout": 260, "ldy": 260}, E_UNSUPPORTED, S2N + ": needs"),
        ({**SPAN, "ldy": 130}, E_ALIGN, S2N + ": pixel strides"),       # here the strides are looked at before the span
    ],
    "emd_sep3x3_fused_s2_reflect_f32": COMMON(S2N),                      # reports as emd_sep3x3_fused_s2_f32
    "emd_sep3x3_fused_s2_genres_f32": [c for c in COMMON(S2N) if "res" not in c[0] and c[0] not in ({"W": 0}, {"H": 12})] + [   # so does this one after its own steps
        ({"img": NUL}, E_INVALID, "emd_sep3x3_fused_s2_genres_f32: null pointer"),
        ({"res_t": NUL, "ldimg": 0}, E_INVALID, "emd_sep3x3_fused_s2_genres_f32: null pointer"),
        ({"ldimg": 0}, E_INVALID, "emd_sep3x3_fused_s2_genres_f32: image pitch and sampling stride must be >= 1"),
        ({"img_stride": 3}, E_UNSUPPORTED, "emd_sep3x3_fused_s2_genres_f32: sampling stride 1 or 2, image pitch <= 64"),
        ({"ldimg": 65}, E_UNSUPPORTED, "emd_sep3x3_fused_s2_genres_f32: sampling stride 1 or 2, image pitch <= 64"),
        ({"Cout": 256, "ldy": 256}, E_UNSUPPORTED, "emd_sep3x3_fused_s2_genres_f32: needs H%8==0, W%32==0, Cin%32==0, Cout%4==0, Cout<=128"),
        ({"Cout": 36}, E_UNSUPPORTED, "emd_sep3x3_fused_s2_genres_f32: needs"),
        ({"H": 12, "dw": NUL}, E_UNSUPPORTED, "emd_sep3x3_fused_s2_genres_f32: needs"),
        ({"img_stride": 1, "img": P + 4}, OK, ""),
    ],
    "emd_sep3x3_dual_f32": [c for c in COMMON("emd_sep3x3_dual_f32") if not {"res", "scale2"} & set(c[0])] + [
        ({"shift_b": NUL}, E_INVALID, "emd_sep3x3_dual_f32: null pointer"),
        ({"Cout2": 132, "ldy2": 132}, E_UNSUPPORTED, "emd_sep3x3_dual_f32: needs H%8==0 (H%4==0 above 64 output channels)"),
        ({"H": 12, "Cout2": 128, "ldy2": 128}, OK, ""),
        ({"W": 1 << 22, "H": 8, "ldy2": 64, "ldy": 32, "Cout": 32}, E_UNSUPPORTED, "emd_sep3x3_dual_f32: 9 image rows of an output"),
        ({"ldy2": 60}, E_ALIGN, "emd_sep3x3_dual_f32: pixel strides"),
        ({"w2lo": P + 8}, E_ALIGN, "emd_sep3x3_dual_f32: pointers must be 16-byte aligned"),
        ({"y2": Q}, E_INVALID, "emd_sep3x3_dual_f32: the two outputs alias"),
        ({"y2": Q, "y": Q + 4}, E_ALIGN, "emd_sep3x3_dual_f32: pointers"),
    ],
}


def test_every_entry_has_probes():
    assert set(PROBES) == set(SIGS) == {n for n in _lib.SIGNATURES if n.startswith("emd_sep3x3_") and n.endswith("_f32")} - {"emd_sep3x3_gemm_f32"}


@pytest.mark.parametrize("entry", sorted(SIGS))
def test_argument_checks(lib, entry):
    sig = SIGS[entry]
    names = [a[0] for a in sig]
    for change, code, text in PROBES[entry]:
        assert set(change) <= set(names), (entry, change)
        args = [C.c_void_p(change.get(n, v)) if kind == "p" else change.get(n, v) for n, kind, v in sig]
        rc = getattr(lib, entry)(*args)
        assert rc == code, (entry, change, rc, lib.emd_last_error())
        if code != OK:
            assert lib.emd_last_error().decode().startswith(text), (entry, change, lib.emd_last_error())


def test_stride_2_without_its_kernel(lib):
    """sep_pipe = 0 takes the only stride-2 form away: the predicate says so and the entry refuses, B == 0 or not."""
    _lib.knob("sep_pipe", 0)
    assert not lib.emd_sep3x3_fused_supported(16, 32, 64, 128, 2, 1)
    sig = SIGS[S2N]
    for B in (0, 1):
        rc = lib.emd_sep3x3_fused_s2_f32(*[C.c_void_p(v) if kind == "p" else (B if n == "B" else v) for n, kind, v in sig])
        assert rc == E_UNSUPPORTED and lib.emd_last_error().decode().startswith(S2N + ": needs H%8==0, W%32==0")
