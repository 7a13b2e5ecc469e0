"""Tracers on the host: the restatement of one drifter step, and what is read off the series (host only).

The device follows chosen particles and advects massless drifters at every step (``Backend.tracers_enable`` / ``tracers_read``,
csrc/sphmi_tracers.h).  A drifter at ``X`` takes, on the state after a step, the probes' raw sums over the Fluid rows j with
``|X - x_j|^2 <= H^2``::

    w_j = (m0 / rho_j) W(|X - x_j|)      n = rows   S = sum w_j   SP = sum w_j P_j   Srho = sum w_j rho_j   Sv = sum w_j v_j

and moves by ``X += (Sv / S) * dt`` where ``S >= min_weight``; otherwise it is dry and stays.  The scheme is first order in ``dt``.
`move` forms the doubles the device forms (one rounding per operation, nothing fused); `sums` adds the rows in numpy's order, not
the device's, so its sums agree with the device's to rounding, not to the bit.
"""
from __future__ import annotations

import numpy as np


def kernel_w(cfg, q) -> np.ndarray:
    """W(q) of the handle's kernel: Wendland C2 (``cfg.kernel == 0``) or the cubic spline (1), with its ``alphaD``."""
    q = np.asarray(q, dtype=np.float64)
    if cfg.kernel == 1:
        return cfg.alphaD * ((1 - 1.5 * q ** 2 + 0.75 * q ** 3) * ((0 <= q) & (q <= 1)) + 0.25 * (2 - q) ** 3 * ((1 < q) & (q <= 2)))
    return cfg.alphaD * (1 - q / 2) ** 4 * (2 * q + 1)


def sums(X, state: dict, cfg) -> dict:
    """Every point of `X` [m, dims] against every Fluid row of `state` (a download: ``Position``, ``Velocity``, ``Density``,
    ``Pressure``, ``Type``), O(m·N): ``n`` [m] (int64), ``S``, ``SP``, ``Srho`` [m], ``Sv`` [m, 3] and ``near`` [m] — a row of the point
    lies within 1e-6·H of the cut.  r² is ``(dx² + dy²) + dz²`` rounded term by term and the cut ``r² <= H²`` inclusive, as on the
    device: a row AT the cut counts for both."""
    X = np.asarray(X, dtype=np.float64)
    m, D = X.shape
    fluid = np.asarray(state["Type"]) == 1
    x = np.asarray(state["Position"], dtype=np.float64)[fluid]
    v = np.asarray(state["Velocity"], dtype=np.float64)[fluid]
    rho = np.asarray(state["Density"], dtype=np.float64)[fluid]
    press = np.asarray(state["Pressure"], dtype=np.float64)[fluid]
    out = {"n": np.zeros(m, np.int64), "S": np.zeros(m), "SP": np.zeros(m), "Srho": np.zeros(m), "Sv": np.zeros((m, 3)), "near": np.zeros(m, bool)}
    for k in range(m):
        d = X[k][None, :] - x[:, :D]
        r2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
        if D == 3:
            r2 = r2 + d[:, 2] * d[:, 2]
        dist = np.sqrt(r2)
        out["near"][k] = (np.abs(dist - cfg.H) <= 1e-6 * cfg.H).any()
        sel = r2 <= cfg.H2
        w = (cfg.m0 / rho[sel]) * kernel_w(cfg, dist[sel] * cfg.h_inv)
        out["n"][k] = sel.sum()
        out["S"][k] = w.sum()
        out["SP"][k] = (w * press[sel]).sum()
        out["Srho"][k] = (w * rho[sel]).sum()
        out["Sv"][k, :D] = (w[:, None] * v[sel][:, :D]).sum(0)
    return out


def move(X, S, Sv, dt: float, min_weight: float = 0.5) -> np.ndarray:
    """The device's update of the drifters `X` [m, dims or 3] from their raw sums `S` [m] and `Sv` [m, 3]: where ``S >= min_weight``,
    ``X[d] + (Sv[d] / S) * dt`` with one rounding per operation; elsewhere — dry, empty, NaN — X itself, bit for bit."""
    X = np.array(X, dtype=np.float64)
    S, Sv = np.asarray(S, dtype=np.float64), np.asarray(Sv, dtype=np.float64)
    wet = S >= min_weight
    D = min(X.shape[1], Sv.shape[1])
    with np.errstate(all="ignore"):
        for d in range(D):
            u = Sv[wet, d] / S[wet]
            X[wet, d] = X[wet, d] + u * np.float64(dt)
    return X


def step(X, state: dict, cfg, dt: float, min_weight: float = 0.5):
    """One drifter step from a download: the sums at `X` on `state` (brute force), then the move.  Returns ``(X_new, sums)``."""
    s = sums(X, state, cfg)
    return move(X, s["S"], s["Sv"], dt, min_weight), s


def _reads(series):
    return [series] if isinstance(series, dict) else [r for r in series if r is not None]


def pathlines(series) -> np.ndarray:
    """The drifters' positions over a run [K_total + 1, m, 3]: `series` is one dict of ``Backend.tracers_read`` or the dicts of
    consecutive intervals (``None`` entries are skipped); the recorded positions — each the position BEFORE that step's move — are
    joined in order and the current position of the newest read is appended, so row k is the position after k executed steps."""
    reads = _reads(series)
    if not reads:
        raise ValueError("pathlines: no read")
    return np.concatenate([r["drifters"]["position"] for r in reads] + [np.asarray(reads[-1]["drifter_position"])[None]])


def dry(series) -> np.ndarray:
    """The mask ``weight < min_weight`` [K_total, m]: the steps at which a drifter did not move."""
    reads = _reads(series)
    if not reads:
        raise ValueError("dry: no read")
    return np.concatenate([r["drifters"]["weight"] < r["min_weight"] for r in reads])


def by_id(series, idp) -> dict:
    """The tracked particles keyed by particle: `idp` [n] holds the ``ID`` of the tracked rows in the order they were named at the
    enable.  Returns ``id`` ascending, ``iteration``, ``time``, ``dt`` and ``values``, ``position``, ``velocity``, ``density``,
    ``pressure`` over all reads of `series`, the particle axis in that ID order."""
    reads = _reads(series)
    ids = np.asarray(idp)
    order = np.argsort(ids, kind="stable")
    if len(ids) > 1 and (np.diff(ids[order]) == 0).any():
        raise ValueError("by_id: the IDs are not unique")
    if not reads:
        raise ValueError("by_id: no read")
    if any(r["particles"]["values"].shape[1] != len(ids) for r in reads):
        raise ValueError("by_id: one ID per tracked particle")
    out = {k: np.concatenate([r[k] for r in reads]) for k in ("iteration", "time", "dt")}
    values = np.concatenate([r["particles"]["values"] for r in reads])[:, order]
    out.update({"id": ids[order], "values": values, "position": values[:, :, 0:3], "velocity": values[:, :, 3:6], "density": values[:, :, 6],
                "pressure": values[:, :, 7]})
    return out


__all__ = ["kernel_w", "sums", "move", "step", "pathlines", "dry", "by_id"]
