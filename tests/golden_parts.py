"""A golden fixture too large for one committed file, stored as several.

``save_parts(stem, arrays)`` writes ``<stem>.part<k>.npz`` files of at most
``PART_BYTES`` of array data each (an array larger than that is cut along its
first axis into ``<key>#<i>`` pieces); ``load_parts(stem)`` returns the arrays
as they were given, bit for bit.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np

PART_BYTES = 768 * 1024  # raw array bytes per part: every file stays below 1 MiB


def save_parts(stem: Path, arrays: dict) -> list:
    pieces = []
    for key, a in arrays.items():
        a = np.asarray(a)
        n = -(-a.nbytes // PART_BYTES)
        if n <= 1:
            pieces.append((key, a))
        else:
            pieces += [(f"{key}#{i}", c) for i, c in enumerate(np.array_split(a, n, axis=0))]
    parts, size = [{}], 0
    for key, a in pieces:
        if parts[-1] and size + a.nbytes > PART_BYTES:
            parts.append({})
            size = 0
        parts[-1][key] = a
        size += a.nbytes
    stem = Path(stem)
    for old in stem.parent.glob(stem.name + ".part*.npz"):
        old.unlink()
    out = []
    for k, part in enumerate(parts):
        out.append(stem.parent / f"{stem.name}.part{k}.npz")
        np.savez_compressed(out[-1], **part)
    return out


def load_parts(stem: Path) -> dict:
    stem = Path(stem)
    files = sorted(stem.parent.glob(stem.name + ".part*.npz"),
                   key=lambda p: int(p.name[len(stem.name) + 5:-4]))
    if not files:
        raise FileNotFoundError(f"no {stem.name}.part*.npz under {stem.parent}")
    whole, cut = {}, {}
    for f in files:
        with np.load(f) as d:  # allow_pickle=False (default)
            for key in d.files:
                if "#" in key:
                    name, i = key.rsplit("#", 1)
                    cut.setdefault(name, {})[int(i)] = d[key]
                else:
                    whole[key] = d[key]
    for name, chunks in cut.items():
        whole[name] = np.concatenate([chunks[i] for i in range(len(chunks))], axis=0)
    return whole
