"""Control boxes and what one reads off the per-step flow through them (host only).

The device delivers, per executed step, the dict of ``Backend.flow_read``: ``count`` [n, boxes] Fluid rows inside a box after the
step, ``volume`` [n, boxes] ``m0 * sum(1 / rho)`` of those rows, ``momentum`` [n, boxes, 3], and ``entered`` / ``left`` [n, boxes],
the rows that crossed into / out of the box during the step.  A box is axis-aligned and half-open, ``lo <= x < hi`` on every axis;
``-inf`` and ``+inf`` are bounds like any other.  Here: boxes that tile an axis, the host restatement of one step from two
downloads, and the rates and running sums a paper plots.
"""
from __future__ import annotations

import numpy as np

from ._abi import Backend

FLUID = 1


def empty_flow(n_boxes: int) -> dict:
    """A series of no steps, shaped like ``Backend.flow_read``'s for `n_boxes` boxes."""
    return Backend.empty_series(Backend.FLOW_FIELDS, int(n_boxes))


def strips(axis: int, edges, dims: int):
    """Boxes that tile ALL space along `axis`: ``(-inf, e0), [e0, e1), …, [e_last, +inf)`` for the increasing `edges`, unbounded
    along every other axis — ``len(edges) + 1`` boxes.  Returns ``(lo, hi)``, each [boxes, dims].  Every point lies in exactly one
    of them, so their counts add up to the number of Fluid rows, and a row that leaves one enters another."""
    e = np.asarray(edges, dtype=np.float64).reshape(-1)
    if dims not in (2, 3) or not 0 <= axis < dims:
        raise ValueError("strips: dims is 2 or 3 and 0 <= axis < dims")
    if np.isnan(e).any() or np.isinf(e).any() or (np.diff(e) <= 0).any():
        raise ValueError("strips: the edges are finite and strictly increasing")
    cuts = np.concatenate([[-np.inf], e, [np.inf]])
    lo = np.full((len(cuts) - 1, dims), -np.inf)
    hi = np.full((len(cuts) - 1, dims), np.inf)
    lo[:, axis], hi[:, axis] = cuts[:-1], cuts[1:]
    return lo, hi


def inside(position, lo, hi) -> np.ndarray:
    """[rows, boxes] bool: ``lo[b] <= x < hi[b]`` on every axis, compared in float64 — the device's rule."""
    x = np.asarray(position, dtype=np.float64)
    lo = np.asarray(lo, dtype=np.float64).reshape(-1, x.shape[1])
    hi = np.asarray(hi, dtype=np.float64).reshape(-1, x.shape[1])
    return ((lo[None, :, :] <= x[:, None, :]) & (x[:, None, :] < hi[None, :, :])).all(axis=2)


def restate(before, after, lo, hi) -> dict:
    """What the device records for ONE step, from the download before it and the download after it (dicts with ``Position``,
    ``Type`` and ``ID``; the rows may be ordered differently — a rebuild permutes them — and are matched by ``ID``): ``count``
    [boxes] Fluid rows inside after the step, ``entered`` [boxes] Fluid rows not inside before and inside after, ``left`` [boxes]
    the other way round.  Rows of another Type are ignored."""
    rows = []
    for d in (before, after):
        fluid = np.asarray(d["Type"]) == FLUID
        ids = np.asarray(d["ID"])[fluid]
        order = np.argsort(ids, kind="stable")
        if len(ids) > 1 and (np.diff(ids[order]) == 0).any():
            raise ValueError("restate: the IDs of the Fluid rows are not unique")
        rows.append((ids[order], inside(np.asarray(d["Position"])[fluid][order], lo, hi)))
    (id0, in0), (id1, in1) = rows
    if not np.array_equal(id0, id1):
        raise ValueError("restate: the two downloads do not hold the same Fluid rows")
    return {"count": in1.sum(axis=0).astype(np.int64), "entered": (~in0 & in1).sum(axis=0).astype(np.int64),
            "left": (in0 & ~in1).sum(axis=0).astype(np.int64)}


def _net(series) -> np.ndarray:
    return np.asarray(series["entered"], dtype=np.int64) - np.asarray(series["left"], dtype=np.int64)


def net_mass_rate(series, m0: float) -> np.ndarray:
    """``m0 * (entered - left) / dt`` per step and box [n, boxes]: the net mass flow into each box, kg/s."""
    return m0 * _net(series) / np.asarray(series["dt"], dtype=np.float64)[:, None]


def discharge(series, m0: float, rho0: float) -> np.ndarray:
    """``net_mass_rate / rho0`` [n, boxes]: the net volume flow into each box in m^3/s (2-D: m^2/s).  For the box ``[c, +inf)``
    along x it is the discharge through the plane ``x = c`` in the +x direction."""
    return net_mass_rate(series, m0) / rho0


def cumulative(series) -> np.ndarray:
    """The running net count per box [n, boxes]: rows that entered minus rows that left since the first sample of `series`."""
    return np.cumsum(_net(series), axis=0)


__all__ = ["empty_flow", "strips", "inside", "restate", "net_mass_rate", "discharge", "cumulative"]
