"""Host-side helpers for the CSR neighbour list of ``Backend.neighbor_list`` (sphmi_neighbors_build, csrc/sphmi_neighbor_list.h):
row i lists ``neighbors[offsets[i]:offsets[i + 1]]``, 0-based rows of what ``download`` delivered at the same point, ascending.

A pair sum the library does not define is three lines with them::

    off, nbr = eng.neighbor_list()
    d = eng.download(("Position", "Density"))
    i, j = pairs(off, nbr)
    r = np.linalg.norm(d["Position"][i] - d["Position"][j], axis=1)
    S = pair_sum(off, (m0 / d["Density"][j]) * W(r))            # one value per entry -> one sum per row

No device, no library: numpy only."""
from __future__ import annotations

import numpy as np


def _offsets(offsets) -> np.ndarray:
    off = np.asarray(offsets, dtype=np.int64)
    if off.ndim != 1 or len(off) < 1 or off[0] != 0 or (np.diff(off) < 0).any():
        raise ValueError("offsets: a non-decreasing 1-D array that starts at 0")
    return off


def pairs(offsets, neighbors):
    """(i, j) of every entry, in list order: i[k] is the row whose list holds entry k, j[k] = neighbors[k]."""
    off = _offsets(offsets)
    j = np.asarray(neighbors)
    if j.ndim != 1 or len(j) != off[-1]:
        raise ValueError("neighbors: offsets[-1] entries")
    i = np.repeat(np.arange(len(off) - 1, dtype=np.int64), np.diff(off))
    return i, j.astype(np.int64)


def pair_sum(offsets, values_per_entry) -> np.ndarray:
    """Per-row sums of one value per entry ([total] or [total, …]): out[i] = sum(values[offsets[i]:offsets[i + 1]]), zero for a
    row without entries.  Summed in list order per row (ascending j), in the dtype numpy adds the values in."""
    off = _offsets(offsets)
    v = np.asarray(values_per_entry)
    if v.ndim < 1 or len(v) != off[-1]:
        raise ValueError("values_per_entry: offsets[-1] entries along the first axis")
    n = len(off) - 1
    out = np.zeros((n,) + v.shape[1:], dtype=np.result_type(v.dtype, np.float64) if v.dtype.kind == "f" else v.dtype)
    full = np.flatnonzero(off[1:] > off[:-1])                                      # np.add.reduceat misreads an empty segment: leave those out
    if len(full):
        out[full] = np.add.reduceat(v, off[:-1][full], axis=0)
    return out


def symmetric(offsets, neighbors) -> bool:
    """Whether j in list(i) implies i in list(j) for every entry — true of a FULL list, false of a HALF list with any pair."""
    i, j = pairs(offsets, neighbors)
    n = len(_offsets(offsets)) - 1
    if len(j) and (j.min() < 0 or j.max() >= n):
        return False
    a, b = np.sort(i * n + j), np.sort(j * n + i)
    return bool(np.array_equal(a, b))
