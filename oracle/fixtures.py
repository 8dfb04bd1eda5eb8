"""Reading and writing the golden fixtures (tests/golden/*.npz) -- TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).

A fixture is one compressed ``<name>.npz``.  No committed file may exceed 1 MiB, so an array that would push the
file over it (the HIP log-mel of the config-4 clips: 1.5 MB per clip before compression) is stored as row blocks in
``<name>.part<k>.npz`` beside it, each under the limit; ``load_fixture`` joins them along axis 0, bit for bit.
"""
from __future__ import annotations

import glob
import io
import os
import re

import numpy as np

PART_LIMIT = 1000 * 1000  # bytes per committed file, with headroom under 1 MiB


def _parts(path: str) -> list:
    stem = path[: -len(".npz")]
    found = [(int(m.group(1)), p) for p in glob.glob(glob.escape(stem) + ".part*.npz")
             if (m := re.fullmatch(r"\.part(\d+)\.npz", p[len(stem):]))]
    return [p for _, p in sorted(found)]


def load_fixture(path: str) -> dict:
    """``dict(np.load(path))`` plus the arrays stored as row blocks in ``<stem>.part<k>.npz``, concatenated in
    part order."""
    out = dict(np.load(path, allow_pickle=False))
    blocks = {}
    for p in _parts(path):
        for k, v in np.load(p, allow_pickle=False).items():
            blocks.setdefault(k, []).append(v)
    for k, vs in blocks.items():
        assert k not in out, f"{path}: {k} is both in the fixture and in its parts"
        out[k] = np.concatenate(vs, axis=0)
    return out


def save_fixture(path: str, arrays: dict, split=("features",)) -> list:
    """Write ``arrays`` as ``path`` (compressed).  If the file comes out above the limit, the ``split`` arrays
    (same number of rows each) move into ``<stem>.part<k>.npz`` blocks of consecutive rows, each file under it.
    Returns the files written; parts of an earlier split are removed."""
    stem = path[: -len(".npz")]
    for p in _parts(path):
        os.remove(p)
    np.savez_compressed(path, **arrays)
    if os.path.getsize(path) <= PART_LIMIT:
        return [path]
    keys = [k for k in split if k in arrays]
    assert keys, f"{path} is over {PART_LIMIT} bytes and has none of {split} to split"
    rows = len(arrays[keys[0]])
    assert all(len(arrays[k]) == rows for k in keys)
    np.savez_compressed(path, **{k: v for k, v in arrays.items() if k not in keys})
    assert os.path.getsize(path) <= PART_LIMIT, f"{path}: still over the limit without {keys}"

    def block(r0, r1):
        buf = io.BytesIO()
        np.savez_compressed(buf, **{k: np.asarray(arrays[k])[r0:r1] for k in keys})
        return buf.getvalue()

    files, r0 = [path], 0
    while r0 < rows:  # consecutive rows, as many as fit (rows compress very differently: noise vs zero padding)
        r1, data = r0 + 1, block(r0, r0 + 1)
        if len(data) > PART_LIMIT:
            raise ValueError(f"{path}: row {r0} of {keys} alone is over {PART_LIMIT} bytes")
        while r1 < rows and len(more := block(r0, r1 + 1)) <= PART_LIMIT:
            r1, data = r1 + 1, more
        files.append(f"{stem}.part{len(files) - 1}.npz")
        with open(files[-1], "wb") as f:
            f.write(data)
        r0 = r1
    return files
