"""Poisoned buffers for the suites that check: no native entry point reads bytes it did not write.

A fresh process gets zeroed pages from the driver, so a `torch.empty` workspace looks clean; in a long-lived process the
caching allocator hands back blocks full of old data.  Three states per case:

    zero      byte 0x00 -- what a fresh process sees;
    ff        byte 0xFF -- fp32 / fp64 NaN, int -1, unsigned max (tests/test_poisoned_workspace_gpu.py's convention);
    leftover  an object that keeps a buffer between calls runs its family's largest case first, then the case under test on
              the same buffers: in-range, plausible old values.

fill(t, byte)                   byte-fills a tensor the caller supplies (workspace=, stats=, out=, a host view as numpy).
poisoned_empty(monkeypatch, b)  every device tensor that torch.empty / torch.empty_like return while the test runs is
                                byte-filled; this reaches the workspaces and output buffers the wrappers allocate themselves.
                                (The package has no Tensor.new_empty call.)  CPU tensors stay as they are: the package draws
                                host dropout masks with torch.empty(...).bernoulli_().
same_bits(a, b)                 bit-for-bit equality of two results (tensors, numpy arrays, scalars, nested lists / tuples / dicts);
                                NaN equals NaN of the same bits.  first_difference(a, b) says where they differ.
"""
import numpy as np
import torch

ZERO, FF = 0x00, 0xFF


def fill(t, byte):
    """Byte-fill a tensor (any dtype, contiguous) or a numpy array in place."""
    if isinstance(t, np.ndarray):
        t.view(np.uint8)[...] = byte
        return t
    if t.numel():
        if not t.is_contiguous():
            raise ValueError("poison.fill: contiguous tensors only")
        t.reshape(-1).view(torch.uint8).fill_(byte)
    return t


class Poisoner:
    """What poisoned_empty returns: `byte` may be changed between calls of one test; `filled` counts the tensors reached."""

    def __init__(self, byte, match):
        self.byte, self.match, self.filled, self.nbytes = byte, match, 0, 0

    def __call__(self, t):
        if isinstance(t, torch.Tensor) and self.byte is not None and self.match(t) and t.numel():
            if t.is_contiguous():
                fill(t, self.byte)
            else:                           # (empty_like of a strided tensor keeps its strides: fill what it owns)
                torch.empty(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage()).fill_(self.byte)
            self.filled += 1
            self.nbytes += t.numel() * t.element_size()
        return t


def poisoned_empty(monkeypatch, byte, match=None):
    """Patch torch.empty and torch.empty_like until the test ends (monkeypatch undoes it).  `match(t)` says which tensors count
    as device memory: CUDA tensors, unless a CPU test names a stand-in."""
    p = Poisoner(byte, match if match is not None else (lambda t: t.is_cuda))
    real_empty, real_like = torch.empty, torch.empty_like

    def empty(*a, **kw):
        return p(real_empty(*a, **kw))

    def empty_like(*a, **kw):
        return p(real_like(*a, **kw))

    monkeypatch.setattr(torch, "empty", empty)
    monkeypatch.setattr(torch, "empty_like", empty_like)
    return p


def _bits(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().contiguous()
        return (str(x.dtype), tuple(x.shape), x.reshape(-1).view(torch.uint8).numpy().tobytes() if x.numel() else b"")
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, np.ascontiguousarray(x).tobytes())
    if isinstance(x, float):
        return ("float", np.float64(x).tobytes())
    if isinstance(x, dict):
        return tuple((k, _bits(v)) for k, v in sorted(x.items()))
    if isinstance(x, (list, tuple)):
        return tuple(_bits(v) for v in x)
    return x


def same_bits(a, b):
    return _bits(a) == _bits(b)


def first_difference(a, b, path="result"):
    """Where two nested results first differ, as text for an assertion message ('' when they are bit-identical)."""
    if type(a) is not type(b):
        return f"{path}: {type(a).__name__} vs {type(b).__name__}"
    if isinstance(a, dict):
        if sorted(a) != sorted(b):
            return f"{path}: keys {sorted(a)} vs {sorted(b)}"
        return next((d for d in (first_difference(a[k], b[k], f"{path}[{k!r}]") for k in sorted(a)) if d), "")
    if isinstance(a, (list, tuple)):
        if len(a) != len(b):
            return f"{path}: {len(a)} vs {len(b)} entries"
        return next((d for d in (first_difference(x, y, f"{path}[{i}]") for i, (x, y) in enumerate(zip(a, b))) if d), "")
    if _bits(a) == _bits(b):
        return ""
    if isinstance(a, (torch.Tensor, np.ndarray)):
        x, y = (np.asarray(t.detach().cpu() if isinstance(t, torch.Tensor) else t) for t in (a, b))
        if x.shape != y.shape or x.dtype != y.dtype:
            return f"{path}: {x.dtype}{list(x.shape)} vs {y.dtype}{list(y.shape)}"
        bad = np.nonzero((x.reshape(-1).view(np.uint8).reshape(x.size, -1) != y.reshape(-1).view(np.uint8).reshape(y.size, -1)).any(axis=1))[0]
        i = int(bad[0])
        return f"{path}: {bad.size} of {x.size} elements differ, first at flat index {i}: {x.reshape(-1)[i]!r} vs {y.reshape(-1)[i]!r}"
    return f"{path}: {a!r} vs {b!r}"


def all_finite(x):
    """Every float in a nested result is finite (ints, strings and None pass)."""
    if isinstance(x, torch.Tensor):
        return bool(torch.isfinite(x).all()) if x.is_floating_point() else True
    if isinstance(x, np.ndarray):
        return bool(np.isfinite(x).all()) if x.dtype.kind == "f" else True
    if isinstance(x, float):
        return bool(np.isfinite(x))
    if isinstance(x, dict):
        return all(all_finite(v) for v in x.values())
    if isinstance(x, (list, tuple)):
        return all(all_finite(v) for v in x)
    return True
