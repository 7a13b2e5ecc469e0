"""The free surface as a mesh (``Backend.isosurface``, sphmi_isosurface_build): the numpy restatement of the extraction the library
runs on the device, and what one asks of the result — its area, the volume it encloses, whether it is closed.

``extract`` takes the arrays ``Backend.sample_grid`` returns and forms the same mesh on the host, bit for bit.  The rules, stated
once here as the header states them:

* node (i, j, k) lies at ``origin[d] + float(i_d) * spacing[d]``; it is inside iff ``S >= level``;
* every cell, named by its lowest node (x fastest), is cut into D! Kuhn simplices: for an axis permutation p (lexicographic),
  ``w0`` = the lowest corner, ``w_k = w_(k-1) + e_p(k)``;
* a lattice with a count of 1 along an axis has no cells and an empty mesh;
* an edge joins node ``a`` to ``b = a + m``, ``m`` in 1 … 2**D - 1 a bitmask of unit steps; ``a`` owns it in slot ``m - 1``; it crosses
  iff exactly one end is inside; one vertex per crossing edge at ``x_a + t * (x_b - x_a)``, ``t = (level - S_a) / (S_b - S_a)``,
  ordered by owner, then slot;
* per simplex (positions 0 … D in w): 3-D, one corner ``a`` inside or one outside — the triangle of the edges (a, b), b ascending;
  two inside a < b, two outside c < d — [(a,c), (a,d), (b,d)] then [(a,c), (b,d), (b,c)]; the first vertex stays and the other two
  are swapped where needed for the normal to point out of the fluid; 2-D — the segment between the two crossing edges with the
  inside to its left;
* attributes: ``A_a + t * (A_b - A_a)`` of the lattice means; where exactly one end has ``count == 0`` the other end's mean unmixed.

No device, no library: numpy only."""
from __future__ import annotations

import itertools

import numpy as np


def _perms(D):
    return list(itertools.permutations(range(D)))                                   # lexicographic


def _corner_masks(perm):
    masks = [0]
    for axis in perm:
        masks.append(masks[-1] | (1 << axis))
    return masks


def _simplex_elements(D, perm, inside):
    """The elements of one simplex as tuples of edges (p, q) — positions in w, as the rule names them — after the swap, and the
    swap bits.  `inside`: the set of inside positions.  The swap is read off the geometry of the unit cell: every vertex at the
    middle of its edge, the normal against the direction from the inside corners to the outside ones."""
    pos = list(range(D + 1))
    ins, outs = [p for p in pos if p in inside], [p for p in pos if p not in inside]
    if not ins or not outs:
        return [], 0
    if D == 3:
        if len(ins) == 1 or len(outs) == 1:
            a = ins[0] if len(ins) == 1 else outs[0]
            elems = [[(a, b) for b in pos if b != a]]
        else:
            (a, b), (c, d) = ins, outs
            elems = [[(a, c), (a, d), (b, d)], [(a, c), (b, d), (b, c)]]
    else:
        elems = [[(p, q) for p in pos for q in pos if p < q and ((p in inside) != (q in inside))]]
    W = np.array([[(m >> d) & 1 for d in range(D)] for m in _corner_masks(perm)], dtype=np.float64)
    out_dir = W[outs].mean(0) - W[ins].mean(0)
    bits = 0
    for k, e in enumerate(elems):
        x = np.array([0.5 * (W[p] + W[q]) for p, q in e])
        if D == 3:
            side = float(np.dot(np.cross(x[1] - x[0], x[2] - x[0]), out_dir))
        else:
            u = x[1] - x[0]
            side = float(-(u[0] * out_dir[1] - u[1] * out_dir[0]))                  # the outside to the right: the inside to the left
        assert side != 0.0
        if side < 0:
            e[-2], e[-1] = e[-1], e[-2]
            bits |= 1 << k
    return [tuple(e) for e in elems], bits


def swap_table(D):
    """{(perm, inside-set bits): swap bits} for every simplex and inside set (bit k of the set: w_k is inside; bit e of the value:
    element e had its last two vertices swapped)."""
    return {(perm, s): _simplex_elements(D, perm, {k for k in range(D + 1) if (s >> k) & 1})[1] for perm in _perms(D) for s in range(1 << (D + 1))}


def extract(weight, origin, spacing, level=0.5, pressure=None, velocity=None, count=None):
    """The mesh of ``weight == level``: ``(vertices [nv, 3] float64, elements [ne, D] int32)``, and — when `pressure` or `velocity`
    is given — ``(vertices, elements, pressure [nv], velocity [nv, 3])`` with ``None`` for the one left out.  `weight`, `pressure`,
    `count` are shaped ``counts[::-1]`` and `velocity` ``counts[::-1] + (3,)``, as ``Backend.sample_grid`` returns them."""
    S3 = np.asarray(weight, dtype=np.float64)
    D = S3.ndim
    if D not in (2, 3):
        raise ValueError("extract: a 2-D or 3-D lattice")
    counts = S3.shape[::-1]
    o = np.asarray(origin, dtype=np.float64).reshape(-1)
    sp = np.asarray(spacing, dtype=np.float64).reshape(-1)
    if len(o) != D or len(sp) != D:
        raise ValueError(f"extract: origin and spacing hold {D} entries each")
    level = np.float64(level)
    S = S3.reshape(-1)
    nodes = S.size
    idx = np.unravel_index(np.arange(nodes), S3.shape)[::-1]                         # idx[d]: the index along axis d, x fastest
    stride = np.cumprod((1,) + counts[:-1])
    inside = S >= level
    nslots = (1 << D) - 1
    offset = [sum(int(stride[d]) for d in range(D) if (m >> d) & 1) for m in range(1 << D)]
    step = [idx[d] + 1 < counts[d] for d in range(D)]

    def exists(m):
        on = np.ones(nodes, dtype=bool)
        for d in range(D):
            if (m >> d) & 1:
                on &= step[d]
        return on

    cross = np.zeros((nodes, nslots), dtype=bool)
    for m in range(1, 1 << D if min(counts) >= 2 else 1):                           # (a count of 1: no cells, no edges, an empty mesh)
        a = np.flatnonzero(exists(m))
        cross[a, m - 1] = inside[a] != inside[a + offset[m]]
    vid = (np.cumsum(cross.reshape(-1)) - 1).reshape(nodes, nslots)                  # owner ascending, then slot ascending
    owner, slot = np.nonzero(cross)
    nv = len(owner)
    other = owner + np.asarray(offset, dtype=np.int64)[slot + 1]
    with np.errstate(all="ignore"):
        t = (level - S[owner]) / (S[other] - S[owner])
        vertices = np.zeros((nv, 3))
        for d in range(D):
            xa = o[d] + idx[d][owner].astype(np.float64) * sp[d]
            xb = o[d] + (idx[d][owner] + (((slot + 1) >> d) & 1)).astype(np.float64) * sp[d]
            vertices[:, d] = xa + t * (xb - xa)

        def attribute(A):
            mixed = A[owner] + t * (A[other] - A[owner])
            if count is None:
                return mixed
            n = np.asarray(count).reshape(-1)
            na, nb = n[owner] == 0, n[other] == 0
            return np.where(na & ~nb, A[other], np.where(nb & ~na, A[owner], mixed))
        p_out = attribute(np.asarray(pressure, dtype=np.float64).reshape(-1)) if pressure is not None else None
        v_out = None
        if velocity is not None:
            V = np.asarray(velocity, dtype=np.float64).reshape(nodes, 3)
            v_out = np.stack([attribute(V[:, d]) for d in range(3)], axis=1).reshape(nv, 3)

    # the elements: cell ascending, simplices in the order of the permutations, then the order within a simplex
    cell = np.ones(nodes, dtype=bool)
    for d in range(D):
        cell &= step[d]
    cells = np.flatnonzero(cell)
    rows, keys = [], []
    for s, perm in enumerate(_perms(D)):
        masks = _corner_masks(perm)
        code = np.zeros(len(cells), dtype=np.int64)
        for k, m in enumerate(masks):
            code |= inside[cells + offset[m]].astype(np.int64) << k
        for c in range(1, (1 << (D + 1)) - 1):
            hit = cells[code == c]
            if not len(hit):
                continue
            elems, _ = _simplex_elements(D, perm, {k for k in range(D + 1) if (c >> k) & 1})
            for e, edges in enumerate(elems):
                cols = []
                for p, q in edges:
                    lo, hi = min(p, q), max(p, q)
                    cols.append(vid[hit + offset[masks[lo]], (masks[hi] ^ masks[lo]) - 1])
                rows.append(np.stack(cols, axis=1))
                keys.append((hit * len(_perms(D)) + s) * 2 + e)
    if rows:
        order = np.argsort(np.concatenate(keys), kind="stable")
        elements = np.concatenate(rows)[order].astype(np.int32)
    else:
        elements = np.zeros((0, D), dtype=np.int32)
    if pressure is None and velocity is None:
        return vertices, elements
    return vertices, elements, p_out, v_out


def _mesh(vertices, elements):
    X, E = np.asarray(vertices, dtype=np.float64), np.asarray(elements, dtype=np.int64)
    if X.ndim != 2 or X.shape[1] != 3 or E.ndim != 2 or E.shape[1] not in (2, 3):
        raise ValueError("a mesh: vertices [nv, 3] and elements [ne, 2] (segments) or [ne, 3] (triangles)")
    if E.size and (E.min() < 0 or E.max() >= len(X)):
        raise ValueError("an element names a vertex that does not exist")
    return X, E


def surface_area(vertices, elements) -> float:
    """The area of a triangle mesh, or the length of a polyline."""
    X, E = _mesh(vertices, elements)
    if E.shape[1] == 2:
        return float(np.linalg.norm(X[E[:, 1]] - X[E[:, 0]], axis=1).sum())
    return float(0.5 * np.linalg.norm(np.cross(X[E[:, 1]] - X[E[:, 0]], X[E[:, 2]] - X[E[:, 0]]), axis=1).sum())


def enclosed_volume(vertices, elements) -> float:
    """The volume a closed triangle mesh encloses (the divergence-theorem sum: positive when the normals point outwards), or the
    area a closed polyline encloses (the shoelace sum: positive when it runs counter-clockwise, the inside to its left)."""
    X, E = _mesh(vertices, elements)
    if E.shape[1] == 2:
        a, b = X[E[:, 0]], X[E[:, 1]]
        return float(0.5 * (a[:, 0] * b[:, 1] - b[:, 0] * a[:, 1]).sum())
    a, b, c = X[E[:, 0]], X[E[:, 1]], X[E[:, 2]]
    return float((a * np.cross(b, c)).sum() / 6.0)


def is_closed(vertices, elements) -> bool:
    """3-D: every directed edge of a triangle occurs once and its reverse once.  2-D: every vertex is once the head and once the
    tail of a segment.  (By index: the coincident vertices of a degenerate element are different vertices.)"""
    X, E = _mesh(vertices, elements)
    n = len(X)
    if E.shape[1] == 2:
        return bool((np.bincount(E[:, 0], minlength=n) == 1).all() and (np.bincount(E[:, 1], minlength=n) == 1).all())
    a = np.concatenate([E[:, 0], E[:, 1], E[:, 2]])
    b = np.concatenate([E[:, 1], E[:, 2], E[:, 0]])
    fwd, rev = np.sort(a * n + b), np.sort(b * n + a)
    return bool(len(np.unique(fwd)) == len(fwd) and np.array_equal(fwd, rev))
