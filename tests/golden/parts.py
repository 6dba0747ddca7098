"""A golden archive too large for one committed file (1 MiB) is stored as numbered parts
(<stem>.0.npz, <stem>.1.npz, ...): every array whole and unchanged in exactly one part."""
import glob
import io
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PART_LIMIT = 1000 * 1000       # bytes per part file, below the 1 MiB limit of a committed file


def part_paths(stem):
    paths = glob.glob(os.path.join(HERE, stem + ".[0-9]*.npz"))
    return sorted(paths, key=lambda p: int(p.rsplit(".", 2)[1]))


def load_parts(stem):
    """the arrays of every part of tests/golden/<stem>.N.npz as one dict"""
    paths = part_paths(stem)
    if not paths:
        raise FileNotFoundError(f"no golden parts {stem}.N.npz under {HERE}")
    out = {}
    for p in paths:
        with np.load(p, allow_pickle=False) as z:
            for k in z.files:
                assert k not in out, (k, p)
                out[k] = z[k]
    return out


def _packed_size(a):
    buf = io.BytesIO()
    np.savez_compressed(buf, a=a)
    return buf.tell()


def save_parts(stem, arrays):
    """write `arrays` as <stem>.N.npz parts of at most PART_LIMIT bytes each (first fit over
    the arrays by decreasing packed size); parts of an earlier run are replaced"""
    sizes = {k: _packed_size(np.asarray(v)) + len(k) + 64 for k, v in arrays.items()}
    bins = []
    for k in sorted(arrays, key=lambda k: -sizes[k]):
        if sizes[k] > PART_LIMIT:
            raise ValueError(f"{k}: {sizes[k]} bytes packed, more than one part holds")
        for b in bins:
            if b[0] + sizes[k] <= PART_LIMIT:
                b[0] += sizes[k]
                b[1].append(k)
                break
        else:
            bins.append([sizes[k], [k]])
    for p in part_paths(stem):
        os.remove(p)
    paths = []
    for i, (_, keys) in enumerate(bins):
        path = os.path.join(HERE, f"{stem}.{i}.npz")
        np.savez_compressed(path, **{k: arrays[k] for k in keys})
        paths.append(path)
    return paths
