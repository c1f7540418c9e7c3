"""Guarded allocations for tests/test_gpu_bounds.py (a helper module like bf16_replica.py: no fixtures, no settings).

While a `Guard` is active, `torch.empty`, `torch.zeros`, `torch.full`, `torch.empty_like` and `torch.zeros_like` hand
out, for the guarded device type, tensors that lie inside a larger uint8 allocation:

    [ leading band >= 64 KiB | payload (dtype, shape as asked) | trailing band >= 1 MiB ]

Both bands and the payload are filled with ONE byte value per run (0x00: zeros; 0xFF: fp32 / bf16 NaN, int32 -1);
`zeros` / `full` tensors keep their content, only their bands take the fill.  The package allocates every output and
workspace through these five module attributes, so none of its code changes.  `verify()` checks, after a device
synchronise, that every band still holds the fill: a kernel that writes a row, a tile or a few bytes outside what it
was given fails an assertion that names the allocation instead of landing in the caching allocator's slack.  A read
of memory nothing wrote shows as a result that differs between the two fills (or is NaN under 0xFF).

Band widths are a design choice, not a measurement: wider than any single tile a kernel writes (the largest is a
256 x 256 fp32 GEMM tile = 256 KiB; rows of W_e are 16 KiB), so that a whole mis-addressed tile still lands in memory
the test owns.

The guard also wraps the bound functions of the loaded library for its duration: it records which `mdno_*` entry
points ran, and can pass ONE of them a workspace size one byte below what its `*_workspace_bytes` function returned
(`undersize=`), to exercise the refusal the header documents."""
from __future__ import annotations

import re
import sys
from pathlib import Path

import torch

FRONT = 64 * 1024
BACK = 1024 * 1024
FILLS = (0x00, 0xFF)
PATCHED = ("empty", "zeros", "full", "empty_like", "zeros_like")
HEADER = Path(__file__).resolve().parents[1] / "include" / "mdno.h"
_THIS = __file__


class GuardError(AssertionError):
    pass


def header_functions(header: Path = HEADER):
    """include/mdno.h parsed the way tests/cabi.py does, keeping the parameters: name -> [(type, parameter name), ...]."""
    text = re.sub(r"/\*.*?\*/", "", header.read_text(), flags=re.S)
    out = {}
    for m in re.finditer(r"^(?:int|size_t|const char\*)\s+(mdno_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S | re.M):
        args = m.group(2).strip()
        params = []
        if args not in ("", "void"):
            for a in args.split(","):
                a = " ".join(a.split())
                pm = re.match(r"^(.*?)(\w+)(\[\d*\])?$", a)
                typ = pm.group(1).strip() + ("*" if pm.group(3) else "")
                params.append((typ, pm.group(2)))
        out[m.group(1)] = params
    return out


def writes_memory(params) -> bool:
    """An entry point that can write caller memory: a non-const pointer other than the stream, or a host table of
    device pointers (mdno_adam_tensor / mdno_flat_tensor)."""
    for typ, name in params:
        if name == "stream" or "*" not in typ:
            continue
        if not typ.startswith("const ") or "mdno_adam_tensor" in typ or "mdno_flat_tensor" in typ:
            return True
    return False


class Record:
    __slots__ = ("base", "offset", "nbytes", "site", "kind")

    def __init__(self, base, offset, nbytes, site, kind):
        self.base, self.offset, self.nbytes, self.site, self.kind = base, offset, nbytes, site, kind

    def leading(self):
        return self.base[:self.offset]

    def payload(self):
        return self.base[self.offset:self.offset + self.nbytes]

    def trailing(self):
        return self.base[self.offset + self.nbytes:]


def _call_site() -> str:
    f = sys._getframe(1)
    while f is not None and f.f_code.co_filename == _THIS:
        f = f.f_back
    if f is None:
        return "?"
    return f"{Path(f.f_code.co_filename).name}:{f.f_lineno} in {f.f_code.co_name}"


def _default_device() -> torch.device:
    return torch.get_default_device() if hasattr(torch, "get_default_device") else torch.device("cpu")


class Guard:
    """Context manager: `with Guard(0xFF) as G: ...; G.verify()`.  `device_type="cpu"` guards host allocations instead
    (the helper's own self-test)."""

    def __init__(self, fill: int, device_type: str = "cuda", front: int = FRONT, back: int = BACK,
                 record_calls: bool = True, undersize=None):
        assert 0 <= fill <= 255 and front % 256 == 0 and back % 256 == 0
        self.fill, self.device_type, self.front, self.back = int(fill), device_type, int(front), int(back)
        self.records = []
        self.calls = []                 # mdno_* entry points in call order (with repeats)
        self.record_calls = record_calls
        self.undersize = dict(undersize or {})      # entry point -> its *_workspace_bytes function
        self.undersized = []            # (entry point, bytes passed) for every call that was given one byte less
        self.sizes = {}                 # *_workspace_bytes function -> its last result
        self._real = {}
        self._lib_real = {}

    # ------------------------------------------------------------------ allocation
    def _guarded(self, device) -> bool:
        return torch.device(device).type == self.device_type

    def alloc(self, shape, dtype, device, kind: str, site: str = None) -> torch.Tensor:
        device = torch.device(device)
        shape = tuple(int(s) for s in shape)
        numel = 1
        for s in shape:
            numel *= s
        item = self._real["empty"]((), dtype=dtype, device="meta").element_size()
        nbytes = numel * item
        total = self.front + nbytes + self.back
        total += -total % 256
        base = self._real["empty"](total, dtype=torch.uint8, device=device)
        base.fill_(self.fill)
        strides, acc = [], 1
        for s in reversed(shape):
            strides.append(acc)
            acc *= max(s, 1)
        t = self._real["empty"](0, dtype=dtype, device=device)
        t.set_(base.untyped_storage(), self.front // item, shape, tuple(reversed(strides)))
        assert (nbytes == 0 or t.data_ptr() == base.data_ptr() + self.front) and t.is_contiguous()      # (empty: null)
        self.records.append(Record(base, self.front, nbytes, site or _call_site(), kind))
        return t

    @staticmethod
    def _size(args, kwargs):
        if "size" in kwargs:
            return tuple(kwargs["size"])
        if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
            return tuple(args[0])
        return tuple(args)

    @staticmethod
    def _plain(kwargs) -> bool:
        """Only what a strided, contiguous, unpinned allocation means is emulated; anything else passes through."""
        if kwargs.get("out") is not None or kwargs.get("pin_memory") or kwargs.get("names") is not None:
            return False
        if kwargs.get("layout", torch.strided) is not torch.strided:
            return False
        return kwargs.get("memory_format", torch.contiguous_format) in (torch.contiguous_format, torch.preserve_format)

    def _finish(self, t, kwargs):
        return t.requires_grad_() if kwargs.get("requires_grad") else t

    def _empty(self, *args, **kwargs):
        dev = kwargs.get("device")
        dev = _default_device() if dev is None else torch.device(dev)
        if not self._guarded(dev) or not self._plain(kwargs):
            return self._real["empty"](*args, **kwargs)
        return self._finish(self.alloc(self._size(args, kwargs), kwargs.get("dtype") or torch.get_default_dtype(), dev,
                                       "empty"), kwargs)

    def _zeros(self, *args, **kwargs):
        dev = kwargs.get("device")
        dev = _default_device() if dev is None else torch.device(dev)
        if not self._guarded(dev) or not self._plain(kwargs):
            return self._real["zeros"](*args, **kwargs)
        t = self.alloc(self._size(args, kwargs), kwargs.get("dtype") or torch.get_default_dtype(), dev, "zeros")
        return self._finish(t.zero_(), kwargs)

    def _full(self, size, fill_value, **kwargs):
        dev = kwargs.get("device")
        dev = _default_device() if dev is None else torch.device(dev)
        if not self._guarded(dev) or not self._plain(kwargs):
            return self._real["full"](size, fill_value, **kwargs)
        dtype = kwargs.get("dtype") or self._real["full"]((), fill_value, device="meta").dtype
        return self._finish(self.alloc(tuple(size), dtype, dev, "full").fill_(fill_value), kwargs)

    def _like(self, name, t, **kwargs):
        dev = torch.device(kwargs["device"]) if kwargs.get("device") is not None else t.device
        if not self._guarded(dev) or not self._plain(kwargs) or t.layout is not torch.strided:
            return self._real[name](t, **kwargs)
        out = self.alloc(t.shape, kwargs.get("dtype") or t.dtype, dev, "empty" if name == "empty_like" else "zeros")
        return self._finish(out.zero_() if name == "zeros_like" else out, kwargs)

    def place(self, t: torch.Tensor, device=None) -> torch.Tensor:
        """A copy of an input tensor inside an arena of its own (a read past its end reads the fill)."""
        device = torch.device(device) if device is not None else t.device
        out = self.alloc(t.shape, t.dtype, device, "input")
        out.copy_(t)
        return out

    # ------------------------------------------------------------------ checks
    def _sync(self):
        if self.device_type == "cuda":
            torch.cuda.synchronize()

    def verify(self) -> None:
        """Every band of every record still holds the fill; otherwise GuardError naming the allocation's call site, its
        size, the side, the first bad offset within that band and the number of bad bytes."""
        self._sync()
        if not self.records:
            return
        counts = []
        for r in self.records:
            counts.append(r.leading().ne(self.fill).sum())
            counts.append(r.trailing().ne(self.fill).sum())
        counts = torch.stack(counts).cpu().tolist()
        bad = []
        for i, r in enumerate(self.records):
            for side, n, band in (("leading", counts[2 * i], r.leading()), ("trailing", counts[2 * i + 1], r.trailing())):
                if n:
                    first = int(band.ne(self.fill).nonzero()[0])
                    bad.append(f"{r.kind} allocation of {r.nbytes} bytes at {r.site}: {side} band overwritten, first bad "
                               f"offset {first} of {band.numel()}, {int(n)} bad byte(s) (fill {self.fill:#04x})")
        if bad:
            raise GuardError(f"{len(bad)} guard band(s) overwritten:\n  " + "\n  ".join(bad[:8]))

    def untouched(self, since: int = 0) -> None:
        """Every `empty` payload allocated from record `since` on still holds the fill and every `zeros` payload is
        still zero (a refused call wrote nothing)."""
        self._sync()
        for r in self.records[since:]:
            if r.kind in ("empty", "zeros") and r.nbytes:
                n = int(r.payload().ne(self.fill if r.kind == "empty" else 0).sum())
                assert n == 0, f"allocation of {r.nbytes} bytes at {r.site}: {n} byte(s) written by a refused call"

    # ------------------------------------------------------------------ context
    def __enter__(self):
        if self.record_calls:           # (first: if the library does not load, torch is still untouched)
            self._wrap_library()
        for name in PATCHED:
            self._real[name] = getattr(torch, name)
        torch.empty, torch.zeros, torch.full = self._empty, self._zeros, self._full
        torch.empty_like = lambda t, **kw: self._like("empty_like", t, **kw)
        torch.zeros_like = lambda t, **kw: self._like("zeros_like", t, **kw)
        return self

    def __exit__(self, *exc):
        for name, fn in self._real.items():
            setattr(torch, name, fn)
        for name, fn in self._lib_real.items():
            setattr(self._lib, name, fn)
        self._lib_real = {}
        self.records = []               # (drops the arenas)
        return False

    def _wrap_library(self):
        from molecular_dynamics_neural_operator_amd import _lib
        self._lib = lib = _lib.load()
        decls = header_functions()
        for name in _lib.SIGNATURES:
            fn = getattr(lib, name)
            self._lib_real[name] = fn
            ws_at = [i for i, (_, p) in enumerate(decls.get(name, [])) if p == "workspace_bytes"]
            setattr(lib, name, self._wrapper(name, fn, ws_at[0] if ws_at else None))

    def _wrapper(self, name, fn, ws_at):
        is_size = name.endswith("_workspace_bytes")

        def call(*args):
            self.calls.append(name)
            if ws_at is not None and name in self.undersize:
                stated = self.sizes.get(self.undersize[name], 0)
                if stated > 0:
                    args = list(args)
                    args[ws_at] = stated - 1
                    self.undersized.append((name, stated - 1))
            res = fn(*args)
            if is_size:
                self.sizes[name] = int(res)
            return res
        return call
