"""Per-bin maps of crest, arrival and mean flow: the host restatement of what the device accumulates, and what one reads off them
(host only).

The device keeps, for every bin of a lattice and over every executed step since ``Backend.maps_enable``, the twelve values of
``Backend.maps_read``.  Per step and bin it forms ``n`` (the owned Fluid rows with a finite velocity inside), ``top`` / ``bottom``
(max / min of the ``up_axis`` coordinate, taken on the order-preserving integer image of the double: -0 < +0) and ``S`` = sum of
``rint(v * 2**32)`` as int64 — operations that do not depend on the order of the rows — and folds them into the record of every wet
bin (``n > 0``) with ``Sd = float64(S) * 2**-32``, ``u = Sd / n``, ``t`` the TotalTime at the end of the step and ``dt`` its time
step:

    top_max, t_top_max        -inf, 0   if top > top_max: top_max, t_top_max = top, t
    bottom_min                +inf      if bottom < bottom_min: bottom_min = bottom
    t_arrival                 +inf      if t_arrival == inf: t_arrival = t
    wet                       0         wet + dt
    fill                      0         fill + n * dt
    flux[3]                   0         flux + Sd * dt
    speed2_max, t_speed2_max  0, 0      s = (ux*ux + uy*uy) + uz*uz; if s > speed2_max: speed2_max, t_speed2_max = s, t
    n_max                     0         max(n_max, n)

`update` forms the same doubles from downloads taken directly after every step, operation for operation: numpy rounds every float64
product, quotient and sum on its own, as the kernels do with contraction off, and ``np.rint`` rounds half to even.
"""
from __future__ import annotations

import numpy as np

FIELDS = ("top_max", "t_top_max", "bottom_min", "t_arrival", "wet", "fill", "flux", "speed2_max", "t_speed2_max", "n_max")
LAST = ("last_n", "last_top", "last_bottom", "last_velocity_sum")
_START = {"top_max": -np.inf, "t_top_max": 0.0, "bottom_min": np.inf, "t_arrival": np.inf, "wet": 0.0, "fill": 0.0, "speed2_max": 0.0,
          "t_speed2_max": 0.0, "n_max": 0.0}
_SIGN = np.uint64(1 << 63)


def lattice(origin, spacing, counts, up_axis: int = None) -> dict:
    """The lattice of ``Backend.maps_enable`` as `update` takes it: `origin`, `spacing`, `counts` of 2 or 3 entries, `up_axis` the
    coordinate whose extremes are kept (default: the last axis).  ``counts[d] = 1`` with ``spacing[d] = inf`` collapses axis d."""
    o, s = np.asarray(origin, dtype=np.float64).reshape(-1), np.asarray(spacing, dtype=np.float64).reshape(-1)
    c = np.asarray(counts, dtype=np.int64).reshape(-1)
    if not (len(o) == len(s) == len(c) and len(o) in (2, 3)):
        raise ValueError("maps: origin, spacing and counts need 2 or 3 entries each")
    up = len(o) - 1 if up_axis is None else int(up_axis)
    if not 0 <= up < len(o):
        raise ValueError("maps: up_axis out of range")
    return {"origin": o, "spacing": s, "counts": c, "up_axis": up, "bins": int(np.prod(c))}


def image(x) -> np.ndarray:
    """The order-preserving uint64 image of float64 values: ``a < b`` iff ``image(a) < image(b)``, -0 below +0."""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) != 0, ~b, b | _SIGN)


def value(u) -> np.ndarray:
    """The inverse of `image`."""
    u = np.ascontiguousarray(u, dtype=np.uint64)
    return np.where(u >> np.uint64(63) != 0, u & ~_SIGN, ~u).astype(np.uint64).view(np.float64)


def fixed(v) -> np.ndarray:
    """``rint(v * 2**32)`` as int64: a velocity in units of 2**-32 m/s, half to even (the product by a power of two is exact)."""
    return np.rint(np.asarray(v, dtype=np.float64) * 4294967296.0).astype(np.int64)


def bin_index(lat: dict, position) -> np.ndarray:
    """The bin of every row of `position` [n, dims], -1 outside the lattice: ``k = floor((x - origin) / spacing)`` per axis, a row
    lies inside iff ``0 <= k < counts`` on every axis, compared as float64 (a NaN lies outside, and ``0 <= -0``); the index is
    ``k0 + counts[0] * (k1 + counts[1] * k2)``, the node order of ``Backend.sample_grid``."""
    x = np.asarray(position, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        k = np.floor((x[:, :len(lat["origin"])] - lat["origin"]) / lat["spacing"])
        inside = ((k >= 0.0) & (k < lat["counts"].astype(np.float64))).all(axis=1)
    out = np.full(len(x), -1, dtype=np.int64)
    stride = 1
    idx = np.zeros(int(inside.sum()), dtype=np.int64)
    for d in range(len(lat["origin"])):
        idx += stride * k[inside, d].astype(np.int64)
        stride *= int(lat["counts"][d])
    out[inside] = idx
    return out


def start(lat: dict, t_begin: float = 0.0) -> dict:
    """The state at enable: every bin the start record, a window of no steps that begins at `t_begin`, a dry last-step map."""
    B = lat["bins"]
    state = {k: np.full(B, v, dtype=np.float64) for k, v in _START.items()}
    state["flux"] = np.zeros((B, 3))
    state.update(steps=0, t_begin=float(t_begin), t_end=float(t_begin), duration=0.0)
    state.update(last_n=np.zeros(B, dtype=np.int64), last_top=np.full(B, -np.inf), last_bottom=np.full(B, np.inf), last_velocity_sum=np.zeros((B, 3)))
    return state


def update(state: dict, lat: dict, position, velocity, is_fluid, t: float, dt: float) -> dict:
    """One executed step, in place: `position` and `velocity` [n, dims] and `is_fluid` [n] bool (``Type == 1``) as downloaded
    directly after the step, in any row order; `t` the TotalTime at the end of the step, `dt` its time step.  Returns `state`."""
    x = np.asarray(position, dtype=np.float64)
    v = np.asarray(velocity, dtype=np.float64)
    t, dt = np.float64(t), np.float64(dt)
    B = lat["bins"]
    counts_row = np.asarray(is_fluid, dtype=bool) & np.isfinite(v).all(axis=1)
    b = bin_index(lat, x)
    rows = np.nonzero(counts_row & (b >= 0))[0]
    b = b[rows]
    n = np.bincount(b, minlength=B).astype(np.int64)
    up = image(x[rows, lat["up_axis"]])
    top, bottom = np.zeros(B, dtype=np.uint64), np.full(B, ~np.uint64(0), dtype=np.uint64)
    np.maximum.at(top, b, up)
    np.minimum.at(bottom, b, up)
    S = np.zeros((B, 3), dtype=np.int64)
    for d in range(v.shape[1]):
        np.add.at(S[:, d], b, fixed(v[rows, d]))
    Sd = S.astype(np.float64) * np.float64(2.0 ** -32)
    wet = n > 0
    nd = n.astype(np.float64)
    topv, bottomv = np.where(wet, value(top), -np.inf), np.where(wet, value(bottom), np.inf)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        higher = wet & (topv > state["top_max"])
        state["top_max"][higher] = topv[higher]
        state["t_top_max"][higher] = t
        lower = wet & (bottomv < state["bottom_min"])
        state["bottom_min"][lower] = bottomv[lower]
        arrived = wet & (state["t_arrival"] == np.inf)
        state["t_arrival"][arrived] = t
        state["wet"][wet] = (state["wet"] + dt)[wet]
        state["fill"][wet] = (state["fill"] + nd * dt)[wet]
        state["flux"][wet] = (state["flux"] + Sd * dt)[wet]
        u = Sd / nd[:, None]
        s = (u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2]
        faster = wet & (s > state["speed2_max"])
        state["speed2_max"][faster] = s[faster]
        state["t_speed2_max"][faster] = t
        fuller = wet & (nd > state["n_max"])
        state["n_max"][fuller] = nd[fuller]
    state["steps"] += 1
    state["t_end"] = float(t)
    state["duration"] = float(np.float64(state["duration"]) + dt)
    state.update(last_n=n, last_top=topv, last_bottom=bottomv, last_velocity_sum=Sd)
    return state


def result(state: dict) -> dict:
    """The state in the shape of ``Backend.maps_read``."""
    out = {"steps": int(state["steps"]), "t_begin": float(state["t_begin"]), "t_end": float(state["t_end"]), "duration": float(state["duration"])}
    for k in FIELDS + LAST:
        out[k] = state[k].copy()
    return out


def _grid(lat: dict, a) -> np.ndarray:
    """[bins] or [bins, 3] → indexed [k0, k1(, k2)(, 3)] (x fastest in memory: Fortran order over the lattice axes)"""
    a = np.asarray(a)
    shape = tuple(int(c) for c in lat["counts"])
    return a.reshape(shape + a.shape[1:], order="F") if a.ndim == 1 else np.stack([a[:, d].reshape(shape, order="F") for d in range(a.shape[1])], axis=-1)


def crest(lat: dict, maps: dict) -> np.ndarray:
    """``top_max`` indexed [k0, k1(, k2)]: the highest `up_axis` coordinate a particle ever had over each bin, NaN where none ever was."""
    a = np.asarray(maps["top_max"], dtype=np.float64).copy()
    a[~np.isfinite(a)] = np.nan
    return _grid(lat, a)


def depth(lat: dict, maps: dict, dp: float, last: bool = False) -> np.ndarray:
    """``top - bottom + dp`` indexed like `crest`: the largest extent of the fluid over each bin across the window
    (``top_max - bottom_min + dp``), or with `last` that of the last executed step; 0 in a bin that stayed dry."""
    top, bottom = (maps["last_top"], maps["last_bottom"]) if last else (maps["top_max"], maps["bottom_min"])
    top, bottom = np.asarray(top, dtype=np.float64), np.asarray(bottom, dtype=np.float64)
    out = np.zeros(len(top))
    wet = np.isfinite(top) & np.isfinite(bottom)
    out[wet] = top[wet] - bottom[wet] + np.float64(dp)
    return _grid(lat, out)


def mean_depth(lat: dict, maps: dict, m0: float, rho0: float) -> np.ndarray:
    """``fill * m0 / rho0 / (area * duration)`` indexed like `crest`: the time-mean volume of fluid over each bin per unit of its
    base — the base is the product of the spacings of the axes other than `up_axis` (collapsed axes: the whole volume per unit of
    the finite ones).  NaN for a window of no steps."""
    s = np.delete(lat["spacing"], lat["up_axis"])
    area = np.prod(s[np.isfinite(s)])
    with np.errstate(invalid="ignore", divide="ignore"):
        return _grid(lat, np.asarray(maps["fill"], dtype=np.float64) * np.float64(m0) / np.float64(rho0) / (area * np.float64(maps["duration"])))


def mean_velocity(lat: dict, maps: dict) -> np.ndarray:
    """``flux / fill`` indexed [k0, k1(, k2), 3]: the mean velocity of the fluid that was in each bin, weighted by particle count and
    time; 0 in a bin that stayed dry."""
    fill = np.asarray(maps["fill"], dtype=np.float64)
    out = np.zeros((len(fill), 3))
    wet = fill > 0
    out[wet] = np.asarray(maps["flux"], dtype=np.float64)[wet] / fill[wet, None]
    return _grid(lat, out)


def max_speed(lat: dict, maps: dict) -> np.ndarray:
    """``sqrt(speed2_max)`` indexed like `crest`: the largest bin-mean speed; the one sqrt, taken here."""
    return _grid(lat, np.sqrt(np.asarray(maps["speed2_max"], dtype=np.float64)))


def arrival_map(lat: dict, maps: dict) -> np.ndarray:
    """``t_arrival - t_begin`` indexed like `crest`: how long after the enable the fluid first reached each bin; NaN where it never did."""
    t = np.asarray(maps["t_arrival"], dtype=np.float64)
    out = np.full(len(t), np.nan)
    reached = np.isfinite(t)
    out[reached] = t[reached] - np.float64(maps["t_begin"])
    return _grid(lat, out)


__all__ = ["FIELDS", "LAST", "lattice", "image", "value", "fixed", "bin_index", "start", "update", "result", "crest", "depth", "mean_depth",
           "mean_velocity", "max_speed", "arrival_map"]
