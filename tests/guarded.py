"""Guard-banded buffers for the tests of entry points that take a pointer and no size.

``guarded(numel, dtype, device)`` places a view inside a larger allocation, with a guard region before and behind it (each at least
64 KiB and at least as large as the view; the view starts 256-byte aligned, its rear guard starts at its last byte + 1).  Guards and
row padding hold a NaN with a distinctive payload (float32, float64) or a fixed word (int16: the packed bf16 planes), and ``check()``
compares them AS INTEGERS against that word: a kernel that writes a NaN of its own into a guard is caught like any other write.  A
guard only ever observes writes inside the test's own allocation; nothing here makes an over-run fault.

``guarded_act`` wraps such a view as an ``ops.Act`` whose in-row columns outside [c0, c0 + C) are guarded too; ``Workspaces`` is the
substitute for ``ops.workspace`` (pytest's monkeypatch), ``Vectors`` the one for the float32 vectors the wrappers allocate themselves.
No GPU is needed to import or to use this module (tests/test_guarded.py runs it on the CPU)."""
import contextlib

import numpy as np
import torch

GUARD_BYTES = 64 * 1024
ALIGN = 256

# dtype -> (integer dtype of the same width, the word the guards hold)
PATTERN = {
    torch.float32: (torch.int32, 0x7FC5A5C3),                 # a quiet NaN, mantissa 0x45A5C3
    torch.float64: (torch.int64, 0x7FF8A5C3A5C3A5C3),         # a quiet NaN, mantissa 0x8A5C3A5C3A5C3
    torch.int16: (torch.int16, 0x7FC5),                       # read as bf16: a NaN too
}

_empty, _empty_like, _full = torch.empty, torch.empty_like, torch.full    # the originals (Vectors substitutes torch.empty)


class Guard:
    """check() of one guarded buffer: raises AssertionError naming the buffer and the first changed offset (in elements, relative to
    the view's first element: negative in the front guard, >= numel in the rear guard)."""

    def __init__(self, name, parent, start, numel, dtype):
        self.name, self.parent, self.start, self.numel, self.dtype = name, parent, start, numel, dtype
        self.word = PATTERN[dtype][1]

    def _first_changed(self, lo, hi):
        bad = (self.parent[lo:hi] != self.word).nonzero()
        return None if bad.numel() == 0 else lo + int(bad[0, 0])

    def __call__(self):
        for lo, hi, what in ((0, self.start, "front guard"), (self.start + self.numel, self.parent.numel(), "rear guard")):
            i = self._first_changed(lo, hi)
            if i is not None:
                raise AssertionError(f"{self.name}: {what} changed at element {i - self.start} of a view of {self.numel} "
                                     f"({(i - self.start) * self.parent.element_size()} bytes from its start): "
                                     f"0x{int(self.parent[i]) & ((1 << (8 * self.parent.element_size())) - 1):x}")

    @property
    def view_words(self):
        """The view's elements as integers (the same memory)."""
        return self.parent[self.start:self.start + self.numel]


def guarded(numel, dtype, device, fill=None, name="buffer"):
    """-> (view, check): ``view`` a contiguous 1-D tensor of ``numel`` elements of ``dtype`` between two guards, ``check`` its Guard.
    fill: None leaves the pattern in the view (an output that must be written completely), a number or a tensor / array of ``numel``
    elements pre-loads it (a base for an accumulating output, an input)."""
    idt, word = PATTERN[dtype]
    size = _empty((), dtype=dtype).element_size()
    numel = int(numel)
    guard = -(-max(GUARD_BYTES, numel * size) // ALIGN) * ALIGN // size
    slack = ALIGN // size
    parent = _full((slack + guard + numel + guard,), word, dtype=idt, device=device)
    start = guard + (-(parent.data_ptr() + guard * size) % ALIGN) // size
    parent = parent[: start + numel + guard]
    view = parent[start:start + numel].view(dtype)
    assert numel == 0 or view.data_ptr() % ALIGN == 0
    if fill is not None:
        if isinstance(fill, (int, float)):
            view.fill_(fill)
        else:
            view.copy_(torch.as_tensor(fill).reshape(-1).to(device=device, dtype=dtype))
    return view, Guard(name, parent, start, numel, dtype)


def holds_pattern(t):
    """Boolean tensor: where ``t`` (a float32 / float64 / int16 tensor) still holds the guard word."""
    idt, word = PATTERN[t.dtype]
    return t.contiguous().view(idt) == word


def assert_written(t, name="output"):
    """An output that must be written completely holds the pattern nowhere."""
    left = holds_pattern(t)
    if bool(left.any()):
        first = tuple(int(i) for i in left.nonzero()[0])
        raise AssertionError(f"{name}: {int(left.sum())} of {left.numel()} elements were never written, the first at {first}")


class ActGuard(Guard):
    """check() of a guarded_act: the two guards and every in-row column outside [c0, c0 + C)."""

    def __init__(self, g, shape, C, c0):
        super().__init__(g.name, g.parent, g.start, g.numel, g.dtype)
        self.shape, self.C, self.c0 = shape, C, c0

    def __call__(self):
        super().__call__()
        rows = self.view_words.view(-1, self.shape[3])
        for lo, hi in ((0, self.c0), (self.c0 + self.C, self.shape[3])):
            bad = (rows[:, lo:hi] != self.word).nonzero()
            if bad.numel():
                p, c = int(bad[0, 0]), lo + int(bad[0, 1])
                raise AssertionError(f"{self.name}: pad column {c} of pixel {p} changed (channels [{self.c0}, {self.c0 + self.C}) of "
                                     f"{self.shape[3]}; element {p * self.shape[3] + c} of the view)")


def guarded_act(B, H, W, C, ld=None, c0=0, fill=None, device=None, name="act"):
    """-> (act, check): an ops.Act [B,H,W,C] = channels [c0, c0 + C) of a guarded [B,H,W,ld] buffer whose other columns hold the pattern.
    fill as for guarded(), for the visible channels only: None, a number, or an array [B,H,W,C]."""
    from emdenoise import ops

    ld = C if ld is None else ld
    device = torch.device("cuda", 0) if device is None else device
    view, g = guarded(B * H * W * ld, torch.float32, device, name=name)
    buf = view.view(B, H, W, ld)
    if fill is not None:
        vis = buf[..., c0:c0 + C]
        if isinstance(fill, (int, float)):
            vis.fill_(fill)
        else:
            vis.copy_(torch.as_tensor(np.asarray(fill, dtype=np.float32) if not torch.is_tensor(fill) else fill).to(device))
    if buf.is_cuda:
        act = ops.Act(buf, C, c0)
    else:   # ops.Act takes device memory only; the CPU tests of this module need the view, not the kernels
        act = object.__new__(ops.Act)
        act.buf, act.B, act.H, act.W, act.ld, act.C, act.c0 = buf, B, H, W, ld, C, c0
    return act, ActGuard(g, (B, H, W, ld), C, c0)


class Workspaces:
    """The substitute for ops.workspace: ``monkeypatch.setattr(ops, "workspace", Workspaces())``.  Hands out guarded views of exactly the
    advertised size (``shrink_bytes``: that much less -- the negative control) and keeps their checks."""

    def __init__(self, shrink_bytes=0):
        self.guards, self.shrink = [], int(shrink_bytes)

    def __call__(self, nbytes, device):
        nbytes = int(nbytes)
        assert nbytes >= 0 and nbytes % 8 == 0 and self.shrink % 8 == 0, nbytes
        view, g = guarded(max((nbytes - self.shrink) // 8, 1), torch.float64, device, name=f"workspace {len(self.guards)} ({nbytes} bytes)")
        self.guards.append(g)
        return view

    def check(self, at_least=1):
        assert len(self.guards) >= at_least, f"{len(self.guards)} workspaces were handed out, expected at least {at_least}"
        for g in self.guards:
            g()


class Vectors:
    """Guards for the float32 vectors the wrappers allocate themselves (mean, var, s1, s2, K, m1, m2, the folded scale / shift ...):
    inside ``with vectors.installed(monkeypatch):`` every 1-D float32 device torch.empty / torch.empty_like comes from guarded()."""

    def __init__(self):
        self.guards = []

    def _one(self, n, device):
        view, g = guarded(n, torch.float32, device, name=f"vector {len(self.guards)} ({n} floats)")
        self.guards.append(g)
        return view

    def empty(self, *size, **kw):
        shape = size[0] if len(size) == 1 and isinstance(size[0], (tuple, list)) else size
        device = kw.get("device")
        if (len(shape) == 1 and kw.get("dtype") == torch.float32 and device is not None and torch.device(device).type == "cuda"
                and set(kw) <= {"dtype", "device"}):
            return self._one(int(shape[0]), device)
        return _empty(*size, **kw)

    def empty_like(self, t, **kw):
        if t.dim() == 1 and t.dtype == torch.float32 and t.is_cuda and not kw:
            return self._one(t.numel(), t.device)
        return _empty_like(t, **kw)

    @contextlib.contextmanager
    def installed(self, monkeypatch):
        with monkeypatch.context() as m:
            m.setattr(torch, "empty", self.empty)
            m.setattr(torch, "empty_like", self.empty_like)
            yield self

    def check(self):
        for g in self.guards:
            g()
