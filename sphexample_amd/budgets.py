"""Curves on top of the per-step budgets of the fluid (host only).

The device delivers, per executed step, the dict of ``Backend.budgets_read``: ``count`` [n] Fluid rows, ``energy`` [n, 3]
(kinetic, potential ``m0 * g * sum(x_last)``, compressive), ``momentum`` [n, 3], ``angular`` [n, 3], ``centre`` [n, 3],
``extremes`` [n, 3] (largest speed, smallest and largest density) and ``box`` [n, 6] (min x per axis, then max x per axis).
What a paper plots from them is a sum or a column.
"""
from __future__ import annotations

import numpy as np

from ._abi import Backend


def empty_budgets() -> dict:
    """A series of no steps, shaped like ``Backend.budgets_read``'s."""
    return Backend.empty_series(Backend.BUDGET_FIELDS)


def total_energy(samples) -> np.ndarray:
    """Kinetic + potential + compressive energy per step [n], added in that order."""
    e = np.asarray(samples["energy"], dtype=np.float64)
    if e.ndim != 2 or e.shape[1] != 3:
        raise ValueError("total_energy: energy is [steps, 3]")
    return (e[:, 0] + e[:, 1]) + e[:, 2]


def front_position(samples, axis: int = 0, side: str = "max") -> np.ndarray:
    """The extent of the fluid along `axis` per step [n], read off ``box``: ``side="max"`` is the largest coordinate — along x the
    wave front of a dam break that runs towards +x (Martin & Moyce's curve) — ``"min"`` the smallest.  Steps without Fluid rows
    give 0, as the box does."""
    box = np.asarray(samples["box"], dtype=np.float64)
    if box.ndim != 2 or box.shape[1] != 6:
        raise ValueError("front_position: box is [steps, 6]")
    if axis not in (0, 1, 2) or side not in ("min", "max"):
        raise ValueError("front_position: axis is 0, 1 or 2 and side \"min\" or \"max\"")
    return box[:, axis + (3 if side == "max" else 0)].copy()


__all__ = ["empty_budgets", "total_energy", "front_position"]
