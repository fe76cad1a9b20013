"""csrc/exitwave.hip has one workspace layout for one stack and for C candidates: every size query still answers what it answered
when there were three.  No GPU here."""
import ctypes as C
import json
import os

from emdenoise import _lib, exitwave

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "exitwave_workspace_bytes.json")
LAM, PX = 2.51e-12, 1e-10


def test_every_size_query_answers_what_it_answered_before_the_layouts_were_merged():
    """tests/golden/exitwave_workspace_bytes.json was written by this script from a build of the commit before the merge (8d5a00b),
    run in the repository's root:

        import itertools, json, sys
        sys.path.insert(0, ".")
        from emdenoise import _lib, exitwave

        lib = _lib.load()
        N, Cs, S, PAD = (1, 3, 64, 65), (1, 3, 64, 1024), (8, 12, 32, 256, 4096), (0, 1, 3)
        grids = {"emd_exitwave_workspace_bytes": (N, S, PAD),
                 "emd_exitwave_candidates_workspace_bytes": (Cs, N, S, PAD),
                 "emd_exitwave_search_workspace_bytes": ((0, 1), Cs, N, S, PAD),
                 "emd_propagate_workspace_bytes": (N, S, PAD),
                 "emd_cfft2_workspace_bytes": (N, S)}
        out = {}
        for knob in (0, 1):
            _lib.knob(exitwave.COMPOSED_KNOB, knob)
            for fn, grid in grids.items():
                out[f"{fn}, composed knob {knob}"] = [[*args, getattr(lib, fn)(*args)] for args in itertools.product(*grid)]
        _lib.knob(exitwave.COMPOSED_KNOB, 0)
        with open("tests/golden/exitwave_workspace_bytes.json", "w") as f:
            f.write("{\\n" + ",\\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in out.items()) + "\\n}\\n")

    Every record is the arguments (the search's: method, C, N, s, pad_periods) and the answer; 0 is a refusal: 65 images, 1024
    candidates (x 64 images > 65535), a side of 12, a side of 4096 with padding, a search method with a candidate count it does not
    take."""
    lib = _lib.load()
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert len(golden) == 10 and sum(len(v) for v in golden.values()) == 1720
    seen = set()
    try:
        for key, records in golden.items():
            fn, knob = key.split(", composed knob ")
            _lib.knob(exitwave.COMPOSED_KNOB, int(knob))
            wrong = [(r[:-1], r[-1], got) for r in records if (got := getattr(lib, fn)(*r[:-1])) != r[-1]]
            assert not wrong, (key, wrong[:5])
            seen.add((fn, bool(records) and any(r[-1] for r in records), any(r[-1] == 0 for r in records)))
    finally:
        _lib.knob(exitwave.COMPOSED_KNOB, 0)
    assert len(seen) == 5 and all(granted and refused for _, granted, refused in seen)
    # the cases the merge could have moved: one stack is the one-candidate layout, without the composed path's extra exit wave
    q = {k: {tuple(r[:-1]): r[-1] for r in v} for k, v in golden.items()}
    for args in ((1, 8, 0), (3, 32, 0), (64, 256, 0), (1, 4096, 0)):
        assert q["emd_exitwave_workspace_bytes, composed knob 0"][args] == q["emd_exitwave_candidates_workspace_bytes, composed knob 0"][(1, *args)]
    for args in ((3, 32, 0), (3, 32, 1)):
        for C_ in (1, 3):
            assert q["emd_exitwave_candidates_workspace_bytes, composed knob 1"][(C_, *args)] \
                == q["emd_exitwave_workspace_bytes, composed knob 1"][args] + 32 * 32 * 16


def test_images_that_overlap_the_defocuses_are_still_refused():
    """Two inputs: the shared check would let them share bytes if they were marked as inputs.  This file refuses every overlap."""
    lib = _lib.load()
    a, c, d, e, f, g = (C.c_void_p(v) for v in (1 << 20, 3 << 20, 4 << 20, 5 << 20, 6 << 20, 1 << 30))
    inside = C.c_void_p((1 << 20) + 64)   # 3 x 32 x 32 floats start at a
    null, big, err = C.c_void_p(0), 1 << 28, lib.emd_last_error
    assert lib.emd_exitwave_reconstruct_f64(a, 3, 32, 0, inside, LAM, PX, 0.0, 1, 0, c, d, e, g, big, null) == -1 and b"overlap" in err()
    assert lib.emd_exitwave_reconstruct_f64(a, 3, 32, 0, a, LAM, PX, 0.0, 1, 0, c, null, null, g, big, null) == -1 and b"overlap" in err()
    assert lib.emd_exitwave_candidates_f64(a, 2, 3, 32, 0, inside, LAM, PX, 0.0, 1, 0, c, d, e, f, g, big, null) == -1 and b"overlap" in err()
    assert lib.emd_exitwave_candidates_f64(a, 2, 3, 32, 0, a, LAM, PX, 0.0, 1, 0, c, d, null, null, g, big, null) == -1 and b"overlap" in err()
