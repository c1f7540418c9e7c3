"""The host-side argument checks of the wrappers in ops.py and forecast.py, one definition each.  Every function returns the
normalised value or raises MdnoError; none loads the library or touches a device beyond converting the tensor it was
given.  A wrapper validates with these, in the order of its arguments, before `_lib.load()`."""
from __future__ import annotations

import math

import torch

from ._lib import MdnoError

INT_MAX = 2 ** 31 - 1


def to_list(v):
    """A tensor as the flat list of its Python values; anything else as it is."""
    return v.detach().cpu().reshape(-1).tolist() if torch.is_tensor(v) else v


def check_dims(what: str, shape, dims=None) -> None:
    """The kernels index with int32: no dimension of `shape` (of `dims`, where only some are limited) may pass 2^31 - 1."""
    if max(shape if dims is None else dims, default=0) > INT_MAX:
        raise MdnoError(f"{what} has shape {tuple(shape)}: a dimension exceeds 2^31 - 1")


def tensor(t, what: str) -> torch.Tensor:
    """`t` itself, a torch tensor."""
    if not torch.is_tensor(t):
        raise MdnoError(f"{what} must be a torch tensor, got {type(t).__name__}")
    return t


def on_device(t: torch.Tensor, what: str) -> torch.Tensor:
    """`t` itself, a tensor on the GPU: the one wording of the refusal of a CPU tensor."""
    if not t.is_cuda:
        raise MdnoError(f"{what} is a CPU tensor: the kernels run on the GPU only (no CPU fallback exists)")
    return t


def device_tensor(t, what: str, ranks, last=None, dtype=torch.float32) -> torch.Tensor:
    """`t` as a contiguous device tensor whose rank is one of `ranks` (None: any) and, with `last`, whose last dimension is
    `last`, converted to `dtype`: a torch dtype, "float" (f64 stays, everything else becomes f32) or None (as it is)."""
    on_device(tensor(t, what), what)
    if (ranks is not None and t.dim() not in ranks) or (last is not None and t.shape[-1:] != (last,)):
        raise MdnoError(f"{what} has shape {tuple(t.shape)}, expected rank {' or '.join(str(r) for r in ranks or ['any'])}"
                        + ("" if last is None else f" and a last dimension of {last}"))
    if dtype == "float":
        dtype = torch.float64 if t.dtype == torch.float64 else torch.float32
    return (t if dtype is None or t.dtype == dtype else t.to(dtype)).contiguous()


def operand(t, what: str, dtypes, shape, dev, optional: bool = False):
    """`t` contiguous: a tensor of one of `dtypes` and exactly `shape` (None: any length) on `dev`; `optional`: or None."""
    if t is None and optional:
        return None
    dtypes = dtypes if isinstance(dtypes, tuple) else (dtypes,)
    if not torch.is_tensor(t) or t.dtype not in dtypes or t.device != dev or t.dim() != len(shape) or \
            any(w is not None and w != d for w, d in zip(shape, t.shape)):
        got = f"{t.dtype} {tuple(t.shape)} on {t.device}" if torch.is_tensor(t) else type(t).__name__
        want = " or ".join(str(d).split(".")[-1] for d in dtypes) + " [" + ", ".join("n" if w is None else str(w) for w in shape) + "]"
        raise MdnoError(f"{what} is {got}: expected {want} on {dev}{' or None' if optional else ''}")
    return t.contiguous()


def int_list(v, what: str, item: str, count, lo: int, hi: int):
    """`v` (a tensor or a sequence) as a list of Python ints: `count` = (fewest, most) entries, each in lo .. hi."""
    v = to_list(v)
    try:
        v = list(v)
        vals = [int(e) for e in v]
        same = all(a == b for a, b in zip(vals, v))
    except (TypeError, ValueError):
        raise MdnoError(f"{what}: {item}s={v!r}: expected a sequence of integers") from None
    if not same:
        raise MdnoError(f"{what}: {item}s={v!r}: expected integers")
    if not count[0] <= len(vals) <= count[1]:
        raise MdnoError(f"{what}: {len(vals)} {item}s, expected {count[0]} .. {count[1]}")
    for e in vals:
        if not lo <= e <= hi:
            raise MdnoError(f"{what}: {item} {e} is outside {lo} .. {hi}")
    return vals


def integer(v, what: str, lo: int, hi: int = INT_MAX, exact: bool = False) -> int:
    """`v` as an int in lo .. hi (None: no upper bound).  The strict rule takes an int and nothing else (no bool, no float,
    no numpy scalar); `exact` takes anything with int(v) == v."""
    ok = isinstance(v, int) and not isinstance(v, bool)
    if exact:
        try:
            ok = int(v) == v
        except (TypeError, ValueError):
            ok = False
    if not ok or not (lo <= int(v) and (hi is None or int(v) <= hi)):
        bound = f">= {lo}" if hi is None or hi == INT_MAX else f"in {lo} .. {hi}"
        raise MdnoError(f"{what} = {v!r}: expected an integer {bound}")
    return int(v)


def real(v, what: str, positive: bool = True, finite: bool = True) -> float:
    """`v` as a float that is > 0 (`positive`) or >= 0, and finite unless `finite` is False (+inf passes, NaN never)."""
    try:
        x = float(v)
    except (TypeError, ValueError):
        raise MdnoError(f"{what} = {v!r}: expected a number") from None
    if not (x > 0.0 if positive else x >= 0.0) or (finite and math.isinf(x)):
        raise MdnoError(f"{what} = {x}: expected a {'finite ' if finite else ''}number {'> 0' if positive else '>= 0'}")
    return x


def form_code(form, table) -> int:
    """The code of the kernel form `form` in `table`."""
    if form not in table:
        raise MdnoError(f"form {form!r}: expected one of {sorted(table)}")
    return table[form]
