"""Per-particle pressure and speed envelopes: the host restatement of what the device accumulates, and what one reads off them
(host only).

The device keeps, for every selected row and over every executed step since ``Backend.envelopes_enable``, the eight values of
``Backend.envelopes_read``: ``p_max`` and the time ``t_p_max`` of its FIRST attainment, ``p_min``, ``impulse`` = sum P dt,
``square`` = sum P^2 dt, ``loaded`` = sum dt over the steps with P > 0, ``speed_max`` and ``t_arrival``, the end of the first step
with P > 0 (+inf: never) — with P the Pressure and v the Velocity a download directly after the step delivers, t the TotalTime at
the end of the step and dt its time step.  `update` forms the same doubles from such downloads, operation for operation: numpy
rounds every float64 product and sum on its own, as the kernel does with contraction off.  A NaN never wins a comparison and
poisons the sums.
"""
from __future__ import annotations

import numpy as np

FIELDS = ("p_max", "t_p_max", "p_min", "impulse", "square", "loaded", "speed_max", "t_arrival")
_START = {"p_max": -np.inf, "t_p_max": 0.0, "p_min": np.inf, "impulse": 0.0, "square": 0.0, "loaded": 0.0, "speed2_max": 0.0,
          "t_arrival": np.inf}


def start(n: int, t_begin: float = 0.0) -> dict:
    """The state at enable for `n` rows: every row the start record, a window of no steps that begins at `t_begin`.  The state
    keeps ``speed2_max`` = max |v|^2, as the device does; `result` takes the root."""
    state = {k: np.full(int(n), v, dtype=np.float64) for k, v in _START.items()}
    state.update(steps=0, t_begin=float(t_begin), t_end=float(t_begin), duration=0.0)
    return state


def update(state: dict, selected, pressure, velocity, t: float, dt: float) -> dict:
    """One executed step, in place: `selected` [n] bool (the rows whose Type the mask holds; the others keep what they have),
    `pressure` [n] and `velocity` [n, 2 or 3] as downloaded directly after the step — entry i of every array belongs to the same
    particle as entry i of the state, so key the downloads by ``ID`` first — `t` the TotalTime at the end of the step, `dt` its
    time step.  Returns `state`."""
    sel = np.asarray(selected, dtype=bool)
    P = np.asarray(pressure, dtype=np.float64)
    v = np.asarray(velocity, dtype=np.float64)
    t, dt = np.float64(t), np.float64(dt)
    vz = v[:, 2] if v.shape[1] == 3 else np.zeros(len(v))
    s = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + vz * vz
    with np.errstate(invalid="ignore", over="ignore"):
        higher = sel & (P > state["p_max"])                          # strict: the first attainment keeps its time
        state["p_max"][higher] = P[higher]
        state["t_p_max"][higher] = t
        lower = sel & (P < state["p_min"])
        state["p_min"][lower] = P[lower]
        state["impulse"][sel] = (state["impulse"] + P * dt)[sel]
        state["square"][sel] = (state["square"] + (P * P) * dt)[sel]
        loaded = sel & (P > 0.0)
        state["loaded"][loaded] = (state["loaded"] + dt)[loaded]
        faster = sel & (s > state["speed2_max"])
        state["speed2_max"][faster] = s[faster]
        arrived = loaded & (state["t_arrival"] == np.inf)
        state["t_arrival"][arrived] = t
    state["steps"] += 1
    state["t_end"] = float(t)
    state["duration"] = float(np.float64(state["duration"]) + dt)
    return state


def result(state: dict) -> dict:
    """The state in the shape of ``Backend.envelopes_read``: ``speed_max`` = sqrt(``speed2_max``), the window as scalars."""
    out = {"steps": int(state["steps"]), "t_begin": float(state["t_begin"]), "t_end": float(state["t_end"]), "duration": float(state["duration"])}
    for k in FIELDS:
        out[k] = np.sqrt(state["speed2_max"]) if k == "speed_max" else state[k].copy()
    return out


def mean_pressure(env: dict) -> np.ndarray:
    """``impulse / duration`` [n]: the time-averaged pressure of every row over the window (NaN for a window of no steps)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.asarray(env["impulse"], dtype=np.float64) / np.float64(env["duration"])


def rms_pressure(env: dict) -> np.ndarray:
    """``sqrt(square / duration)`` [n]: the root-mean-square pressure of every row over the window."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.sqrt(np.asarray(env["square"], dtype=np.float64) / np.float64(env["duration"]))


def arrival_map(env: dict) -> np.ndarray:
    """``t_arrival - t_begin`` [n]: how long after the enable the first positive pressure reached every row; NaN where it never
    did (rows that are not selected included)."""
    t = np.asarray(env["t_arrival"], dtype=np.float64)
    out = np.full(len(t), np.nan)
    reached = np.isfinite(t)
    out[reached] = t[reached] - np.float64(env["t_begin"])
    return out


def by_id(env: dict, id) -> dict:
    """`env` keyed by particle: `id` [n] is the ``ID`` of the download the read belongs to; every per-row array comes back in
    ascending ID order, ``id`` with them, the window unchanged — two reads of different row orders become comparable."""
    ids = np.asarray(id)
    order = np.argsort(ids, kind="stable")
    if len(ids) > 1 and (np.diff(ids[order]) == 0).any():
        raise ValueError("by_id: the IDs are not unique")
    out = {k: (np.asarray(v)[order] if isinstance(v, np.ndarray) and v.shape[:1] == ids.shape[:1] else v) for k, v in env.items()}
    out["id"] = ids[order]
    return out


__all__ = ["FIELDS", "start", "update", "result", "mean_pressure", "rms_pressure", "arrival_map", "by_id"]
