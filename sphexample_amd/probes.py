"""Gauges on top of the probe sums (host only).

The device delivers, per step and probe, the Shepard sum ``S = sum_j (m0 / rho_j) W(|x_p - x_j|)`` over the Fluid rows
within H (``Backend.probes_enable`` / ``probes_read``): about 1 inside the fluid, about 1/2 at a free surface, 0 in empty
space.  A water-height gauge is a vertical column of probes plus a threshold crossing of S along it — a discontinuous
functional of the state, which is why it lives here and not in a kernel.
"""
from __future__ import annotations

import numpy as np


def gauge_column(base, top, spacing: float) -> np.ndarray:
    """The probe points of a gauge: from `base` to `top` (points of the same dimension, usually differing in the vertical
    coordinate only), `spacing` apart or a little closer so that both ends are probes.  Returns [n, dims], base first."""
    base, top = np.asarray(base, dtype=np.float64), np.asarray(top, dtype=np.float64)
    if base.shape != top.shape or base.ndim != 1:
        raise ValueError("gauge_column: base and top are points of the same dimension")
    length = float(np.linalg.norm(top - base))
    if not (spacing > 0) or not (length > 0):
        raise ValueError("gauge_column: spacing and the distance from base to top must be positive")
    n = int(np.ceil(length / spacing - 1e-12)) + 1
    t = np.linspace(0.0, 1.0, max(n, 2))
    return base[None, :] + t[:, None] * (top - base)[None, :]


def water_level(z, S, threshold: float = 0.5):
    """The level along one gauge: `z` [n] the heights of its probes, ascending (z[0] = base, z[-1] = top), `S` [n] their
    Shepard sums — or [steps, n], giving one level per step.  Scanning from the top, the first adjacent pair with
    S[k] >= threshold > S[k + 1] is the surface; the level is interpolated linearly between the two probes.  A column
    that is dry (no probe reaches the threshold) returns z[0], one that is submerged (the top probe reaches it) z[-1];
    spray above the surface does not count unless it reaches the threshold, and then the topmost crossing is taken."""
    z = np.asarray(z, dtype=np.float64)
    S = np.asarray(S, dtype=np.float64)
    if z.ndim != 1 or len(z) < 2 or not (np.diff(z) > 0).all():
        raise ValueError("water_level: z holds at least two ascending heights")
    if S.shape[-1] != len(z):
        raise ValueError("water_level: S holds one value per probe of the column")
    if S.ndim == 2:
        return np.array([water_level(z, row, threshold) for row in S])
    if S.ndim != 1:
        raise ValueError("water_level: S is [n] or [steps, n]")
    if S[-1] >= threshold:
        return float(z[-1])
    for k in range(len(z) - 2, -1, -1):
        if S[k] >= threshold > S[k + 1]:
            f = (S[k] - threshold) / (S[k] - S[k + 1])
            return float(z[k] + f * (z[k + 1] - z[k]))
    return float(z[0])


# the sums `linear_fit` reads, by the trailing shape of one probe's entry
_MOMENT_SHAPES = {"weight": (), "count": (), "sum_pressure": (), "sum_density": (), "sum_velocity": (3,), "moment1": (3,), "moment2": (3, 3),
                  "moment_pressure": (3,), "moment_density": (3,), "moment_velocity": (3, 3)}


def empty_probe_moments(n_probes: int, dims: int, h: float) -> dict:
    """A record of no steps, shaped like ``Backend.probe_moments_read``'s for `n_probes` probes."""
    out = {"iteration": np.zeros(0, dtype=np.int64), "time": np.zeros(0), "dt": np.zeros(0)}
    out.update({key: np.zeros((0, int(n_probes), *shape), dtype=np.int64 if key == "count" else np.float64) for key, shape in _MOMENT_SHAPES.items()})
    out.update({"h": float(h), "dims": int(dims), "probe_moments_dropped": 0})
    return out


def fit_series(record, **kw) -> dict:
    """The fitted signal of every probe at every step: `record` is the dict of ``Backend.probe_moments_read`` — the raw moment
    sums shaped [steps, probes, …], with the handle's `h` and `dims` — and ``sphexample_amd.fields.linear_fit`` is run ONCE over
    all steps × probes (keywords go to it: `min_count`, `min_rcond`, `h`, `dims`).  Returns its dict reshaped to
    [steps, probes, …]: `pressure`, `density`, `velocity`, their gradients, `linear` (the entries that were fitted) and `rcond`,
    with the fallback to the Shepard mean as `linear_fit` defines it, plus the record's `iteration`, `time` and `dt` where it has
    them.  A probe on a wall or on the bed reads the field AT the sensor, not a fraction of h inside the fluid."""
    from .fields import linear_fit                        # (fields imports this module)
    S = np.asarray(record["weight"])
    if S.ndim != 2:
        raise ValueError("fit_series: the record of probe_moments_read is needed: weight [steps, probes]")
    steps, probes = S.shape
    flat = {k: v for k, v in record.items() if k not in _MOMENT_SHAPES}
    for key, shape in _MOMENT_SHAPES.items():
        a = np.asarray(record[key])
        if a.shape != (steps, probes, *shape):
            raise ValueError(f"fit_series: {key} is shaped [steps, probes{''.join(', %d' % s for s in shape)}]")
        flat[key] = a.reshape(steps * probes, *shape)
    fit = linear_fit(flat, **kw)
    out = {k: np.asarray(v).reshape(steps, probes, *np.asarray(v).shape[1:]) for k, v in fit.items()}
    out.update({k: record[k] for k in ("iteration", "time", "dt") if k in record})
    return out


__all__ = ["gauge_column", "water_level", "empty_probe_moments", "fit_series"]
