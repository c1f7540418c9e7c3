"""Golden fixtures under ``tests/golden/`` as files of at most 1 MiB each — TEST INFRASTRUCTURE.

``save_golden(path, **arrays)`` writes ``<stem>.npz`` (``np.savez_compressed``) when that stays under
``MAX_FILE_BYTES``; otherwise the same arrays as ``<stem>.part0.npz``, ``<stem>.part1.npz``, ... each under the
limit, an array too large for one part split along axis 0 into pieces named ``<key>@0``, ``<key>@1``, ...
``load_golden(path)`` reads either form and returns the same arrays, in the same order, bit for bit.
"""
from __future__ import annotations

import io
import re
from pathlib import Path

import numpy as np

MAX_FILE_BYTES = 1 << 20          # the repository's limit for a committed file
PART_RAW_BYTES = 768 << 10        # uncompressed bytes packed into one part (deflate never grows arrays past this)
_PART = re.compile(r"\.part(\d+)\.npz$")


def _parts(path: Path):
    found = [(int(m.group(1)), p) for p in path.parent.glob(f"{path.stem}.part*.npz") if (m := _PART.search(p.name))]
    return [p for _, p in sorted(found)]


def _npz_bytes(arrays: dict) -> bytes:
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    return buf.getvalue()


def save_golden(path, **arrays) -> list:
    """Write `arrays` as the fixture `path` (a `.npz` name); returns the files written."""
    path = Path(path)
    arrays = {k: np.asanyarray(v) for k, v in arrays.items()}
    if any("@" in k for k in arrays):
        raise ValueError("fixture keys may not contain '@'")
    for old in [path] + _parts(path):
        old.unlink(missing_ok=True)
    whole = _npz_bytes(arrays)
    if len(whole) <= MAX_FILE_BYTES:
        path.write_bytes(whole)
        return [path]
    pieces = []
    for k, a in arrays.items():
        if a.dtype != object and a.ndim >= 1 and a.nbytes > PART_RAW_BYTES and a.shape[0] > 1:
            n = min(a.shape[0], -(-a.nbytes // PART_RAW_BYTES))
            pieces += [(f"{k}@{j}", c) for j, c in enumerate(np.array_split(a, n, axis=0))]
        else:
            pieces.append((k, a))
    groups, cur, size = [], {}, 0
    for k, a in pieces:
        if cur and size + a.nbytes > PART_RAW_BYTES:
            groups.append(cur)
            cur, size = {}, 0
        cur[k] = a
        size += a.nbytes
    groups.append(cur)
    written = []
    for i, g in enumerate(groups):
        data = _npz_bytes(g)
        if len(data) > MAX_FILE_BYTES:
            raise ValueError(f"{path.stem}.part{i}.npz would be {len(data)} bytes")
        p = path.with_name(f"{path.stem}.part{i}.npz")
        p.write_bytes(data)
        written.append(p)
    return written


class GoldenArrays(dict):
    """The arrays of a fixture stored in parts; `files` lists the keys as `np.load`'s NpzFile does."""

    @property
    def files(self):
        return list(self.keys())


def load_golden(path):
    """The fixture `path` (`<stem>.npz`, or its `<stem>.partN.npz` files)."""
    path = Path(path)
    if path.exists():
        return np.load(path, allow_pickle=True)
    parts = _parts(path)
    if not parts:
        raise FileNotFoundError(path)
    order, whole, split = [], {}, {}
    for p in parts:
        with np.load(p, allow_pickle=True) as z:
            for k in z.files:
                base, _, j = k.rpartition("@") if "@" in k else (k, "", "")
                if base not in whole and base not in split:
                    order.append(base)
                if j:
                    split.setdefault(base, []).append((int(j), z[k]))
                else:
                    whole[base] = z[k]
    for base, chunks in split.items():
        whole[base] = np.concatenate([c for _, c in sorted(chunks, key=lambda t: t[0])], axis=0)
    return GoldenArrays((k, whole[k]) for k in order)
