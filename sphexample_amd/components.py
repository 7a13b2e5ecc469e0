"""Host-side companion of ``Backend.components`` (sphmi_components_build, csrc/sphmi_components.h): the connected bodies of the
selected rows — main body, droplets — restated in numpy, and the statistics a splash study reads off them.

Two selected rows i != j are linked iff ``r^2 = ((dx^2 + dy^2) + dz^2) <= link * link``; a component is a connected set of selected
rows, its FIRST ROW its smallest row, and components are numbered in ascending first row.  `label` and `from_pairs` return what
the device returns, bit for bit: a dict of ``label`` int32 [n] (-1: not selected), ``first_row``, ``count`` int32 [C] and ``box``
float64 [C, 6] (min x, y, z, max x, y, z; exact zeros for z in 2-D)::

    c = eng.components()                                         # the fluid, linked within H
    d = eng.download(("Position", "Velocity"))
    bulk = main_body_mask(c["label"], c["count"])                # rows of the largest body
    x_front = front_position(d["Position"], c["label"], c["count"])      # … and ITS wave front: no droplet spoils it
    t = droplet_table(c["label"], c["count"], d["Position"], d["Velocity"], m0)

Mass, centroid and momentum per component are formed here and not on the device on purpose: they are floating-point sums, which
would need a fixed order there; ``np.bincount`` adds in row order.

No device, no library: numpy only."""
from __future__ import annotations

import numpy as np

_SIGN = np.uint64(1 << 63)


def _key(x: np.ndarray) -> np.ndarray:
    """The order-preserving uint64 image of float64 (-0 below +0), the one the device takes its minima and maxima on."""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) != 0, ~b, b ^ _SIGN)


def _unkey(k: np.ndarray) -> np.ndarray:
    k = np.ascontiguousarray(k, dtype=np.uint64)
    return np.where(k >> np.uint64(63) != 0, k ^ _SIGN, ~k).view(np.float64)


def _selected(n: int, selected) -> np.ndarray:
    sel = np.ones(n, bool) if selected is None else np.asarray(selected)
    if sel.shape != (n,):
        raise ValueError("selected: one flag per row")
    return sel.astype(bool)


def _roots(n: int, i: np.ndarray, j: np.ndarray) -> np.ndarray:
    """Min-label union–find over the links (i, j): root[x] is the smallest row x is connected to.  Every round hooks, for every
    link whose ends lie in different trees, the larger root under the smallest root offered to it, then flattens all trees."""
    root = np.arange(n, dtype=np.int64)
    while len(i):
        ri, rj = root[i], root[j]
        open_ = ri != rj
        if not open_.any():
            break
        i, j, ri, rj = i[open_], j[open_], ri[open_], rj[open_]                      # a closed link stays closed
        np.minimum.at(root, np.maximum(ri, rj), np.minimum(ri, rj))
        while True:
            up = root[root]
            if np.array_equal(up, root):
                break
            root = up
    return root


def _table(root: np.ndarray, sel: np.ndarray, position) -> dict:
    n = len(root)
    rows = np.arange(n, dtype=np.int64)
    is_root = sel & (root == rows)
    dense = np.cumsum(is_root) - 1
    label = np.where(sel, dense[root], -1).astype(np.int32)
    first_row = np.flatnonzero(is_root).astype(np.int32)
    C = len(first_row)
    count = np.bincount(label[sel], minlength=C).astype(np.int32)
    box = None
    if position is not None:
        X = np.asarray(position, dtype=np.float64)
        if X.ndim != 2 or len(X) != n or X.shape[1] not in (2, 3):
            raise ValueError("position: [n, 2] or [n, 3]")
        box = np.zeros((C, 6))
        if C:
            order = np.flatnonzero(sel)
            order = order[np.argsort(label[order], kind="stable")]
            starts = np.concatenate([[0], np.cumsum(count[:-1], dtype=np.int64)])
            for d in range(X.shape[1]):
                k = _key(X[order, d])
                box[:, d] = _unkey(np.minimum.reduceat(k, starts))
                box[:, 3 + d] = _unkey(np.maximum.reduceat(k, starts))
    return {"label": label, "first_row": first_row, "count": count, "box": box}


def from_pairs(n: int, i, j, selected=None, position=None) -> dict:
    """The components of `n` rows from a list of links (i[k], j[k]) — each once or both ways, e.g. ``neighbors.pairs`` of
    ``neighbor_list(half=True)`` cut to the link length.  Links with an end that is not selected are ignored.  `box` is None
    without `position`."""
    n = int(n)
    sel = _selected(n, selected)
    i, j = np.asarray(i, dtype=np.int64).reshape(-1), np.asarray(j, dtype=np.int64).reshape(-1)
    if i.shape != j.shape:
        raise ValueError("from_pairs: i and j hold one entry per link")
    if len(i) and (min(i.min(), j.min()) < 0 or max(i.max(), j.max()) >= n):
        raise ValueError("from_pairs: a link names a row outside 0 .. n - 1")
    keep = sel[i] & sel[j] & (i != j)
    return _table(_roots(n, i[keep], j[keep]), sel, position)


def links(position, selected, link: float, chunk: int = 512):
    """(i, j), i < j, of every pair of selected rows with ``((dx^2 + dy^2) + dz^2) <= link * link``: an enumeration in chunks of
    rows, every term rounded on its own, as the device forms it."""
    X = np.asarray(position, dtype=np.float64)
    if X.ndim != 2 or X.shape[1] not in (2, 3):
        raise ValueError("position: [n, 2] or [n, 3]")
    sel = _selected(len(X), selected)
    link = float(link)
    if not np.isfinite(link) or not link > 0.0:
        raise ValueError("link: finite and positive")
    cut = link * link
    rows = np.flatnonzero(sel)
    Y = X[rows]
    out_i, out_j = [], []
    for a in range(0, len(rows), chunk):
        A = Y[a:a + chunk]
        B = Y[a:]                                                                    # j > i only
        dx = A[:, None, 0] - B[None, :, 0]
        dy = A[:, None, 1] - B[None, :, 1]
        r2 = dx * dx + dy * dy
        if X.shape[1] == 3:
            dz = A[:, None, 2] - B[None, :, 2]
            r2 = r2 + dz * dz
        ii, jj = np.nonzero(r2 <= cut)
        jj = jj + a
        ii = ii + a
        keep = jj > ii
        out_i.append(rows[ii[keep]]); out_j.append(rows[jj[keep]])
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)      # noqa: E731
    return cat(out_i), cat(out_j)


def label(position, selected, link: float) -> dict:
    """The host restatement of ``Backend.components``: the same four arrays from a download's `position`, the flags of the selected
    rows (e.g. ``Type == 1``) and the link length.  O(n^2) pair tests: for checks and small sets."""
    X = np.asarray(position, dtype=np.float64)
    i, j = links(X, selected, link)
    return _table(_roots(len(X), i, j), _selected(len(X), selected), X)


def main_body(count) -> int:
    """The number of the component with the most rows (the lowest number among equals)."""
    count = np.asarray(count)
    if count.ndim != 1 or len(count) == 0:
        raise ValueError("main_body: no component")
    return int(np.argmax(count))


def main_body_mask(label, count) -> np.ndarray:
    """The rows of the main body [n] (bool)."""
    return np.asarray(label) == main_body(count)


def droplet_table(label, count, position, velocity, m0: float) -> dict:
    """Per component: ``count`` [C], ``mass`` [C] = m0 * count, ``centroid`` [C, dims] (the mean position), ``momentum`` [C, dims]
    = m0 * sum v, and ``main`` — the number of the main body; every other row of the table is a droplet."""
    lab, count = np.asarray(label), np.asarray(count, dtype=np.int64)
    X, V = np.asarray(position, dtype=np.float64), np.asarray(velocity, dtype=np.float64)
    if X.ndim != 2 or X.shape != V.shape or len(X) != len(lab):
        raise ValueError("droplet_table: position and velocity are [n, dims], one row per label")
    C = len(count)
    sel = lab >= 0
    if sel.any() and lab.max() >= C:
        raise ValueError("droplet_table: a label beyond the table")
    if not np.array_equal(np.bincount(lab[sel], minlength=C), count):
        raise ValueError("droplet_table: count does not belong to label")
    per = lambda a: np.stack([np.bincount(lab[sel], weights=a[sel, d], minlength=C) for d in range(a.shape[1])], 1)      # noqa: E731
    return {"count": count, "mass": float(m0) * count, "centroid": per(X) / np.maximum(count, 1)[:, None], "momentum": float(m0) * per(V),
            "main": main_body(count) if C else -1}


def front_position(position, label, count, axis: int = 0, side: str = "max") -> float:
    """The extent of the MAIN BODY along `axis`: ``side="max"`` its largest coordinate — along x the wave front of a dam break —
    ``"min"`` its smallest.  The companion of ``budgets.front_position``, whose box a single flying droplet sets."""
    X = np.asarray(position, dtype=np.float64)
    if X.ndim != 2 or not 0 <= axis < X.shape[1] or side not in ("min", "max"):
        raise ValueError("front_position: axis names a column of position and side is \"min\" or \"max\"")
    x = X[main_body_mask(label, count), axis]
    return float(x.max() if side == "max" else x.min())


__all__ = ["label", "from_pairs", "links", "main_body", "main_body_mask", "droplet_table", "front_position"]
