"""GPU tests of emdenoise.resample (csrc/resample.hip) through the C ABI, against the float64 restatement of
tests/resample_ref.py.

Inputs: ``raw = float32(900) * synthetic_lq(B, H, W, seed=700 + H + W)[..., 0] - 40``.  Inputs and outputs are views of
tests/guarded.py; the guards are checked after every call, an output must be written completely and be finite (an over-read of a
segment into a neighbouring buffer would feed the sum a pattern NaN).

The bars are not derived from the device's output.  NEAREST is bit for bit a source pixel, equal sizes are bit for bit the source in
every mode.  Everything else: relative L2 against the float64 restatement <= FACTOR = 4 times the LARGEST relative L2 distance of the
float32 restatement (cv2's order: float32 weights, a horizontal pass into float32 rows, a vertical pass in float32) from the float64
one over CASES in that mode, computed once on the CPU by ``python -m tests.test_resample_gpu`` (it prints them; no GPU) and written
below as YARD_*: the kernel sums in double and rounds once, so it owes the reference less than cv2's own arithmetic does.

Every figure is printed before it is asserted."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from emdenoise import _lib, exitwave, resample
from tests import resample_ref as R
from tests.guarded import assert_written, guarded
from tests.synth_inputs import synthetic_lq

pytestmark = pytest.mark.gpu

FACTOR = 4.0
# the float32 restatement's largest relative L2 distance from the float64 one over CASES (python -m tests.test_resample_gpu)
YARD_LINEAR = 4.114e-08
YARD_CUBIC = 6.517e-08
YARD_AREA = 5.559e-07
YARD = {"linear": YARD_LINEAR, "cubic": YARD_CUBIC, "area": YARD_AREA}

MODES = ["nearest", "linear", "cubic", "area"]
# ((B, H, W), (h, w)): the smallest shapes at which each part can go wrong
CASES = [
    ((2, 37, 53), (16, 20)),        # true area with unequal runs and both edge weights; a downscale for the others
    ((2, 48, 64), (16, 16)),        # whole ratios 3 x 4: the block form
    ((1, 40, 40), (20, 20)),        # exactly 2
    ((3, 17, 23), (40, 31)),        # enlarging: area takes the emulated form
    ((2, 33, 65), (50, 20)),        # mixed axes: area emulated on both
    ((1, 1, 7), (3, 3)),            # extents of 1: every cubic tap clamped
    ((1, 5, 1), (2, 4)),
    ((1, 130, 70), (129, 69)),      # near identity: tiny second weights
    ((2, 64, 64), (64, 64)),        # bitwise
    ((1, 300, 520), (96, 200)),     # several tiles, several LDS segments both ways, non-square
    ((1, 2100, 9), (5, 9)),         # runs of 420 rows, many row segments; x is an identity axis inside true area
    ((1, 80, 1100), (20, 70)),      # two tiles of columns, each over several column segments (ratio 15.7) and two row segments
]
BIG = ((1, 2048, 2048), (512, 512))  # the load_image shape, once: AREA and CUBIC only
PARAMS = [(c, m) for c in CASES for m in MODES] + [(BIG, "area"), (BIG, "cubic")]


@functools.lru_cache(maxsize=None)
def raw(shape):
    B, H, W = shape
    r = np.float32(900) * synthetic_lq(B, H, W, seed=700 + H + W)[..., 0] - np.float32(40)
    return r                                                               # shared: nobody writes it


@functools.lru_cache(maxsize=None)
def ref64(case, mode):
    (shape, (h, w)) = case
    y = R.resize(raw(shape), (w, h), mode)
    return y


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def yardsticks():
    """Per mode, the float32 restatement's largest distance from the float64 one over PARAMS (CPU only)."""
    out = {}
    for case, mode in PARAMS:
        if mode != "nearest":
            (shape, (h, w)) = case
            out[mode] = max(out.get(mode, 0.0), rel_l2(R.resize(raw(shape), (w, h), mode, np.float32), ref64(case, mode)))
    return out


def dev():
    return torch.device("cuda", 0)


def call_c(x, boxes, hw, mode):
    """emd_resize_f32 on guarded copies of x [B,H,W] (and of the boxes: a tensor, an array or None) -> the output [B,h,w] as numpy,
    after the guards of every buffer have been checked and the output found written and finite."""
    B, H, W = x.shape
    h, w = hw
    xin, gx = guarded(x.size, torch.float32, dev(), fill=np.array(x), name="x")
    out, gy = guarded(B * h * w, torch.float32, dev(), name="y")
    bptr = C.c_void_p(0)
    if boxes is not None:
        bt = torch.as_tensor(np.asarray(boxes), dtype=torch.int32).to(dev()).contiguous()
        assert tuple(bt.shape) == (B, 4)
        bptr = C.c_void_p(bt.data_ptr())
    rc = _lib.load().emd_resize_f32(C.c_void_p(xin.data_ptr()), H * W, W, B, H, W, bptr, C.c_void_p(out.data_ptr()), h, w,
                                    resample.INTERPOLATIONS[mode], _lib.stream_ptr())
    _lib.check(rc, "emd_resize_f32")
    torch.cuda.synchronize()
    gx()
    gy()
    assert np.array_equal(xin.cpu().numpy().view(np.int32), np.ascontiguousarray(x).ravel().view(np.int32)), "the input was written"
    y = out.view(B, h, w)
    assert_written(y)
    assert bool(torch.isfinite(y).all()), "a non-finite output: something outside the image was read"
    return y.cpu().numpy()


def check(got, want, x, mode, what):
    """The bars of this file, on one result."""
    if mode == "nearest":
        assert np.isin(got, x).all() and np.array_equal(got, want.astype(np.float32)), f"{what}: not bit for bit a source pixel"
        print(f"{what}: bit for bit")
        return
    if got.shape == x.shape:
        assert np.array_equal(got.view(np.int32), x.view(np.int32)), f"{what}: equal sizes must return the source bit for bit"
        print(f"{what}: equal sizes, bit for bit")
        return
    e, yard = rel_l2(got, want), YARD[mode]
    print(f"{what}: rel L2 {e:.3e}; bar {FACTOR * yard:.3e} (float32 restatement's largest {yard:.3e})")
    assert e <= FACTOR * yard, what


# ---- resize ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case,mode", PARAMS, ids=lambda p: p if isinstance(p, str) else "x".join(map(str, p[0])) + "-" + "x".join(map(str, p[1])))
def test_resize(case, mode):
    (shape, hw) = case
    x = raw(shape)
    got = call_c(x, None, hw, mode)
    check(got, ref64(case, mode), x, mode, f"{mode} {shape} -> {hw}")


# ---- crop_resize ----------------------------------------------------------------------------------------------------------------

CROP_SHAPE = (3, 70, 131)
WHOLE, CORNER, PIXEL = (0, 0, 131, 70), (100, 40, 31, 30), (5, 7, 1, 1)
CROP_HW = (16, 24)


@pytest.mark.parametrize("mode", MODES)
def test_crop_resize(mode):
    x = raw(CROP_SHAPE)
    for box in (WHOLE, CORNER, PIXEL):
        boxes = [box] * 3
        got = call_c(x, boxes, CROP_HW, mode)
        want = R.crop_resize(x, boxes, CROP_HW[::-1], mode)
        x0, y0, bw, bh = box
        check(got, want, x[:, y0:y0 + bh, x0:x0 + bw], mode, f"crop_resize {mode} box {box} -> {CROP_HW}")
        if box == WHOLE:
            assert np.array_equal(got.view(np.int32), call_c(x, None, CROP_HW, mode).view(np.int32)), "the whole image as a box is resize"
    boxes = [CORNER, (3, 2, 64, 48), (17, 5, 40, 16)]                      # three sizes in one batch; the last is 16 rows: an identity axis
    got = call_c(x, boxes, (16, 16), mode)
    want = R.crop_resize(x, boxes, (16, 16), mode)
    for b, (x0, y0, bw, bh) in enumerate(boxes):
        check(got[b], want[b], x[b, y0:y0 + bh, x0:x0 + bw], mode, f"crop_resize {mode} box {boxes[b]} of a mixed batch -> (16, 16)")
    # the same boxes from the host and from the device, through the Python interface
    xd = torch.from_numpy(x).to(dev())
    host = resample.crop_resize(xd, np.array(boxes), 16, mode)
    device = resample.crop_resize(xd, torch.tensor(boxes, dtype=torch.int32, device=dev()), 16, mode)
    assert host.is_cuda and tuple(host.shape) == (3, 16, 16) and torch.equal(host, device)
    assert np.array_equal(host.cpu().numpy().view(np.int32), got.view(np.int32))


@pytest.mark.parametrize("mode", MODES)
def test_a_device_box_reaching_outside_the_image_is_clamped(mode):
    x = raw(CROP_SHAPE)
    wild = [(120, 60, 50, 50), (-5, -5, 20, 20), (500, 500, 0, -3)]
    clamped = [(120, 60, 11, 10), (0, 0, 20, 20), (130, 69, 1, 1)]         # x0 into 0..W-1, then bw into 1..W-x0; likewise y
    got = call_c(x, wild, (16, 16), mode)                                  # call_c checks the guards around x and y
    assert np.array_equal(got.view(np.int32), call_c(x, clamped, (16, 16), mode).view(np.int32))
    want = R.crop_resize(x, clamped, (16, 16), mode)
    for b, (x0, y0, bw, bh) in enumerate(clamped):
        check(got[b], want[b], x[b, y0:y0 + bh, x0:x0 + bw], mode, f"crop_resize {mode} box {wild[b]} clamped to {clamped[b]}")


# ---- conventions, bits and capture ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_an_image_does_not_depend_on_its_batch(mode):
    x = raw((3, 17, 23))
    for hw in ((40, 31), (8, 10)):
        batch = call_c(x, None, hw, mode)
        alone = call_c(x[1:2], None, hw, mode)
        assert np.array_equal(batch[1].view(np.int32), alone[0].view(np.int32)), (mode, hw)
        assert np.array_equal(batch.view(np.int32), call_c(x, None, hw, mode).view(np.int32)), "not reproducible"


def test_the_generic_instance_gives_the_same_bits():
    """The development knob resize_generic selects the instance with one inner loop for every form (tools/resample_bench.py's A/B)."""
    cases = [(CASES[0], m) for m in MODES] + [(CASES[3], "area"), (CASES[1], "area"), (CASES[10], "area"), (CASES[9], "cubic")]
    for (shape, hw), mode in cases:
        kept = call_c(raw(shape), None, hw, mode)
        _lib.knob("resize_generic", 1)
        try:
            generic = call_c(raw(shape), None, hw, mode)
        finally:
            _lib.knob("resize_generic", 0)
        assert np.array_equal(kept.view(np.int32), generic.view(np.int32)), (shape, hw, mode)


def test_numpy_and_tensor_conventions():
    x = raw((2, 37, 53))
    want = call_c(x, None, (16, 20), "area")
    y, yt = resample.resize(x, (20, 16), "area"), resample.resize(torch.from_numpy(x).to(dev()), (20, 16), 3)
    assert isinstance(y, np.ndarray) and y.dtype == np.float32 and y.shape == (2, 16, 20) and np.array_equal(y, want)
    assert isinstance(yt, torch.Tensor) and yt.is_cuda and yt.dtype == torch.float32 and np.array_equal(yt.cpu().numpy(), want)
    one = resample.resize(x[0], (20, 16), "area")
    assert one.shape == (16, 20) and np.array_equal(one, want[0])
    sq = resample.resize(x, 8)                                             # an int is a square; the default is cv2's: linear
    assert sq.shape == (2, 8, 8) and np.array_equal(sq, call_c(x, None, (8, 8), "linear"))
    c = resample.crop_resize(x[0], [(3, 2, 30, 20)], (10, 5))              # the default is area
    assert c.shape == (5, 10) and np.array_equal(c, call_c(x[:1], [(3, 2, 30, 20)], (5, 10), "area")[0])
    empty = resample.resize(torch.empty((0, 8, 8), device=dev()), 4)
    assert tuple(empty.shape) == (0, 4, 4)


def test_resize_stack_is_linear_resize():
    x = torch.from_numpy(raw((3, 48, 48))).to(dev())
    y = exitwave.resize_stack(x, 32)
    assert y.is_cuda and tuple(y.shape) == (3, 32, 32) and torch.equal(y, resample.resize(x, 32, "linear"))
    e = rel_l2(y.cpu().numpy(), R.resize(raw((3, 48, 48)), 32, "linear"))
    print(f"resize_stack [3,48,48] -> 32: rel L2 {e:.3e}; bar {FACTOR * YARD_LINEAR:.3e}")
    assert e <= FACTOR * YARD_LINEAR
    assert isinstance(exitwave.resize_stack(raw((3, 48, 48)), 32), np.ndarray)


def test_captured_in_one_graph_and_replayed_on_new_boxes():
    x = torch.from_numpy(raw(CROP_SHAPE)).to(dev())
    first = torch.tensor([CORNER, (3, 2, 64, 48), (17, 5, 40, 16)], dtype=torch.int32, device=dev())
    second = torch.tensor([(0, 0, 131, 70), (60, 30, 48, 40), (9, 9, 24, 24)], dtype=torch.int32, device=dev())
    run = lambda b: (lambda c: (c, exitwave.resize_stack(c, 32)))(resample.crop_resize(x, b, 24, "area"))
    want1, want2 = run(first), run(second)                                 # eager
    boxes = first.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = run(boxes)
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs, want1))
    boxes.copy_(second)
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs, want2))
    assert not torch.equal(want1[0], want2[0])


if __name__ == "__main__":
    for mode, y in sorted(yardsticks().items()):
        print(f"YARD_{mode.upper()} = {y:.3e}     # bar {FACTOR * y:.3e}")
