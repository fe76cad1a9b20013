"""tests/guarded.py itself, on the CPU: an untouched buffer passes, one overwritten element of the front guard, the rear guard or a pad
column fails -- also when what was written is a NaN (the guards are compared as integers) -- and the failure names the buffer and
the offset."""
import pytest
import torch

from tests import guarded as G

CPU = torch.device("cpu")
DTYPES = [torch.float32, torch.float64, torch.int16]


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("numel", [1, 37, 40000])
def test_layout(dtype, numel):
    view, check = G.guarded(numel, dtype, CPU, name="v")
    size = view.element_size()
    assert view.dtype == dtype and view.numel() == numel and view.is_contiguous() and view.data_ptr() % 256 == 0
    front, rear = check.start, check.parent.numel() - check.start - numel
    for g in (front, rear):
        assert g * size >= 64 * 1024 and g >= numel
    assert view.data_ptr() == check.parent.data_ptr() + check.start * size      # the rear guard starts at the view's last byte + 1
    assert bool(G.holds_pattern(view).all())                                    # fill=None: the pattern is visible
    if dtype != torch.int16:
        assert bool(torch.isnan(view).all())
    check()


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_fill(dtype):
    view, check = G.guarded(5, dtype, CPU, fill=0)
    assert view.tolist() == [0] * 5
    view, check = G.guarded(5, dtype, CPU, fill=torch.arange(5))
    assert view.tolist() == [0, 1, 2, 3, 4]
    view.fill_(3)      # writing the view is what a kernel is allowed to do
    check()
    with pytest.raises(AssertionError, match="never written"):
        G.assert_written(G.guarded(5, dtype, CPU)[0])
    G.assert_written(view)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("where", ["front", "rear", "front_far", "rear_far"])
@pytest.mark.parametrize("nan", [False, True])
def test_one_overwritten_guard_element_is_caught(dtype, where, nan):
    view, check = G.guarded(37, dtype, CPU, fill=1, name="victim")
    check()
    i = {"front": check.start - 1, "rear": check.start + 37, "front_far": 0, "rear_far": check.parent.numel() - 1}[where]
    if nan and dtype != torch.int16:
        check.parent.view(dtype)[i] = float("nan")          # torch's own NaN: another payload
        assert bool(torch.isnan(check.parent.view(dtype)[i]))
    elif nan:
        check.parent[i] = 0x7FC0                            # bf16's default NaN
    else:
        check.parent[i] = 0
    with pytest.raises(AssertionError, match=rf"victim: {where.split('_')[0]} guard changed at element {i - check.start} ") as e:
        check()
    assert "victim" in str(e.value)


def test_the_first_changed_offset_is_reported():
    view, check = G.guarded(8, torch.float32, CPU, name="w")
    check.parent[check.start + 8 + 5] = 0
    check.parent[check.start + 8 + 2] = 0
    with pytest.raises(AssertionError, match=r"w: rear guard changed at element 10 of a view of 8 \(40 bytes"):
        check()


def test_act_with_row_padding():
    a, check = G.guarded_act(2, 3, 5, 8, ld=16, c0=4, fill=0.0, device=CPU, name="dx")
    assert (a.B, a.H, a.W, a.C, a.ld, a.c0) == (2, 3, 5, 8, 16, 4) and a.buf.shape == (2, 3, 5, 16)
    assert a.buf.data_ptr() % 256 == 0
    assert float(a.torch().abs().sum()) == 0.0 and bool(torch.isnan(a.buf[..., :4]).all()) and bool(torch.isnan(a.buf[..., 12:]).all())
    check()
    a.torch().fill_(2.0)
    check()
    for c, val in ((3, 0.0), (12, 0.0), (15, float("nan")), (0, float("nan"))):
        a, check = G.guarded_act(2, 3, 5, 8, ld=16, c0=4, fill=0.0, device=CPU, name="dx")
        check.view_words.view(torch.float32).view(2, 3, 5, 16)[1, 2, 4, c] = val      # through the parent tensor
        with pytest.raises(AssertionError, match=rf"dx: pad column {c} of pixel 29 "):
            check()
    for i, what in ((-1, "front"), (2 * 3 * 5 * 16, "rear")):
        a, check = G.guarded_act(2, 3, 5, 8, ld=16, c0=4, device=CPU, name="dx")
        check.parent.view(torch.float32)[check.start + i] = float("nan")
        with pytest.raises(AssertionError, match=rf"dx: {what} guard changed at element {i} "):
            check()


def test_act_fill_with_an_array_and_dense_rows():
    import numpy as np

    x = np.arange(2 * 2 * 3 * 4, dtype=np.float32).reshape(2, 2, 3, 4)
    a, check = G.guarded_act(2, 2, 3, 4, fill=x, device=CPU)
    assert a.ld == 4 and torch.equal(a.torch(), torch.from_numpy(x))
    check()
    b, check = G.guarded_act(2, 2, 3, 4, ld=12, c0=4, device=CPU)     # fill=None: the visible part holds the pattern too
    with pytest.raises(AssertionError, match="never written"):
        G.assert_written(b.torch())


def test_workspace_substitute_hands_out_the_advertised_size():
    ws = G.Workspaces()
    v = ws(9 * 2 * 32 * 8, CPU)
    assert v.dtype == torch.float64 and v.numel() == 9 * 2 * 32 and ws(0, CPU).numel() == 1
    ws.check(at_least=2)
    v[-1] = 1.0
    ws.check()
    short = G.Workspaces(shrink_bytes=1536)
    u = short(12 * 2 * 32 * 8, CPU)
    assert u.numel() == 12 * 2 * 32 - 192
    short.guards[0].parent.view(torch.float64)[short.guards[0].start + u.numel()] = 0.5      # the first double past the short size
    with pytest.raises(AssertionError, match=r"workspace 0 \(6144 bytes\): rear guard changed at element 576 "):
        short.check()
    with pytest.raises(AssertionError, match="expected at least 1"):
        G.Workspaces().check()


def test_the_library_allocator_returns_the_advertised_size():
    from emdenoise import ops

    for nbytes in (0, 8, 4608, 6144):
        w = ops.workspace(nbytes, CPU)
        assert w.dtype == torch.float64 and w.numel() == max(nbytes // 8, 1)
