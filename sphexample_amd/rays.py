"""Rays through the fluid (``Backend.cast_rays``, sphmi_cast_rays, csrc/sphmi_rays.h): the search restated in numpy, and what is
built on it — the water level at gauges, depth images, the hit points handed on for normals.

The search, per ray ``x(t) = o + t·d`` (one multiply, one add), with ``inside(t) = S(x(t)) >= level``:
    march       K = ceil((t_end − t_begin) / step);  t_k = t_begin + k·step for k < K, t_K = t_end;  the crossing is the smallest k in
                1 … K whose ends disagree the way `mode` asks ("enter": out → in, "leave": in → out, "any": either)
    refinement  from (a, b) = (t_{k−1}, t_k), four rounds: δ = (b − a)·2⁻⁶, u_m = a + m·δ (u_0 = a, u_64 = b), the new bracket is
                (u_{m−1}, u_m) for the smallest m in 1 … 64 whose side differs from the side of a; δ == 0 leaves the bracket
    record      the point and the raw sums at the INSIDE end of the final bracket
`restate` performs exactly these operations in this order with `evaluate` as its only access to the fluid: with
``Backend.sample_point_gradients`` as evaluator it must reproduce the device bit for bit (tests/test_rays_gpu.py)."""
from __future__ import annotations

import numpy as np

MODES = ("enter", "leave", "any")
REFINE_ROUNDS = 4
FOUND, STARTS_INSIDE = 1, 2
SUMS = ("weight", "count", "sum_pressure", "sum_density", "sum_velocity")


def normalize(directions) -> np.ndarray:
    """Unit vectors along `directions` ([n, dims] or [dims]): with them t and `step` are lengths."""
    d = np.asarray(directions, dtype=np.float64)
    norm = np.sqrt((d * d).sum(axis=-1, keepdims=True))
    if not (norm > 0).all():
        raise ValueError("normalize: a zero direction")
    return d / norm


def intervals(t_begin, t_end, step) -> np.ndarray:
    """K of every ray."""
    return np.ceil((np.asarray(t_end, np.float64) - np.asarray(t_begin, np.float64)) / float(step)).astype(np.int64)


def march_t(t_begin, t_end, step, k, K) -> np.ndarray:
    """t_k: ``t_begin + float(k) * step`` for k < K and t_end itself for k = K (arrays broadcast)."""
    k = np.asarray(k, dtype=np.int64)
    return np.where(k >= K, t_end, t_begin + k.astype(np.float64) * float(step))


def refine_u(a, b, delta, m) -> np.ndarray:
    """u_m of a refinement round: a for m = 0, b for m = 64, ``a + float(m) * delta`` between."""
    m = np.asarray(m, dtype=np.int64)
    return np.where(m <= 0, a, np.where(m >= 64, b, a + m.astype(np.float64) * delta))


def ray_points(origins, directions, t) -> np.ndarray:
    """``o + t·d``: the product rounded, then the sum."""
    return origins + t[..., None] * directions


def crosses(before, after, mode: str) -> np.ndarray:
    differ = before != after
    return differ if mode == "any" else differ & (after if mode == "enter" else before)


def restate(evaluate, origins, directions, t_begin, t_end, step, level, mode) -> dict:
    """The complete search in numpy.  ``evaluate(points [m, dims])`` returns the raw sums at the points — a dict with `weight`
    [m] and, for the record, `count`, `sum_pressure`, `sum_density` [m], `sum_velocity` [m, 3] (missing ones stay zero).
    Returns the dict of ``Backend.cast_rays`` and two more keys: `margin` [n], the smallest |S − level| among the points
    evaluated for the ray, and `evaluations` [n], their number."""
    if mode not in MODES:
        raise ValueError(f"restate: mode is one of {MODES}")
    o = np.ascontiguousarray(origins, dtype=np.float64)
    d = np.ascontiguousarray(directions, dtype=np.float64)
    n, D = o.shape
    tb = np.ascontiguousarray(np.broadcast_to(np.asarray(t_begin, np.float64), (n,)))
    te = np.ascontiguousarray(np.broadcast_to(np.asarray(t_end, np.float64), (n,)))
    step, level = float(step), float(level)
    K = intervals(tb, te, step)
    out = {"status": np.zeros(n, np.int32), "interval": np.full(n, -1, np.int64), "bracket": np.full((n, 2), np.nan),
           "point": np.full((n, 3), np.nan), "weight": np.zeros(n), "count": np.zeros(n, np.int64), "sum_pressure": np.zeros(n),
           "sum_density": np.zeros(n), "sum_velocity": np.zeros((n, 3)), "margin": np.full(n, np.inf), "evaluations": np.zeros(n, np.int64)}
    if D == 2:
        out["point"][:, 2] = 0.0

    def weigh(rays, t):
        """S at parameter t [m, w] of rays [m] → [m, w], and the sums; keeps the margin and the count of evaluations"""
        x = ray_points(o[rays][:, None, :], d[rays][:, None, :], t)
        sums = evaluate(np.ascontiguousarray(x.reshape(-1, D)))
        S = np.asarray(sums["weight"], np.float64).reshape(t.shape)
        return S, sums

    def note(rays, S, used):
        gap = np.where(used, np.abs(S - level), np.inf).min(axis=1)
        out["margin"][rays] = np.minimum(out["margin"][rays], gap)
        out["evaluations"][rays] += used.sum(axis=1)

    # the march, 64 points per round as on the device (what is evaluated does not change the result: only where it stops)
    lanes = np.arange(64, dtype=np.int64)
    alive = np.arange(n)
    carry = np.zeros(n, bool)
    side_a = np.zeros(n, bool)
    base = 0
    while len(alive):
        k = base + lanes[None, :]
        Ka = K[alive][:, None]
        used = k <= Ka
        t = march_t(tb[alive][:, None], te[alive][:, None], step, k, Ka)
        S, _ = weigh(alive, t)
        note(alive, S, used)
        inside = used & (S >= level)
        before = np.concatenate([carry[alive][:, None], inside[:, :-1]], axis=1)
        cross = used & (k >= 1) & crosses(before, inside, mode)
        if base == 0:
            out["status"][alive] |= np.where(inside[:, 0], STARTS_INSIDE, 0).astype(np.int32)
        hit = cross.any(axis=1)
        first = cross.argmax(axis=1)
        rows = np.nonzero(hit)[0]
        out["interval"][alive[rows]] = base + first[rows]
        side_a[alive[rows]] = before[rows, first[rows]]
        carry[alive] = inside[:, 63]
        base += 64
        alive = alive[~hit & (base <= K[alive])]

    found = np.nonzero(out["interval"] >= 1)[0]
    out["status"][found] |= FOUND
    if len(found) == 0:
        return out
    kx = out["interval"][found]
    a = march_t(tb[found], te[found], step, kx - 1, K[found])
    b = march_t(tb[found], te[found], step, kx, K[found])
    sa = side_a[found]
    m63 = np.arange(1, 64, dtype=np.int64)
    for _ in range(REFINE_ROUNDS):
        delta = (b - a) * 0.015625
        go = np.nonzero(delta != 0.0)[0]
        if len(go) == 0:
            break
        u = refine_u(a[go][:, None], b[go][:, None], delta[go][:, None], m63[None, :])
        S, _ = weigh(found[go], u)
        note(found[go], S, np.ones_like(S, bool))
        differs = (S >= level) != sa[go][:, None]
        m = np.where(differs.any(axis=1), differs.argmax(axis=1) + 1, 64)
        na, nb = refine_u(a[go], b[go], delta[go], m - 1), refine_u(a[go], b[go], delta[go], m)
        a[go], b[go] = na, nb
    out["bracket"][found, 0], out["bracket"][found, 1] = a, b
    t_in = np.where(sa, a, b)
    x = ray_points(o[found], d[found], t_in)
    out["point"][found, :D] = x
    sums = evaluate(np.ascontiguousarray(x))
    for key in SUMS:
        if key in sums:
            out[key][found] = np.asarray(sums[key])
    return out


def hit_parameter(result, mode: str = "enter") -> np.ndarray:
    """t at the inside end of every bracket ([n], NaN where nothing was hit): b for an entering crossing, a for a leaving one;
    with "any" the first crossing leaves the side the ray starts on (status bit 1)."""
    br, st = np.asarray(result["bracket"]), np.asarray(result["status"])
    leaving = np.ones(len(st), bool) if mode == "leave" else (st & STARTS_INSIDE) != 0 if mode == "any" else np.zeros(len(st), bool)
    return np.where(leaving, br[:, 0], br[:, 1])


def hit_points(result, dims: int = 3):
    """(points [m, dims], rays [m]): the hit points of the rays that found a crossing and the indices of those rays — ready for
    ``Backend.sample_point_gradients`` and ``fields.surface_normal_at``."""
    rays = np.nonzero((np.asarray(result["status"]) & FOUND) != 0)[0]
    return np.ascontiguousarray(np.asarray(result["point"])[rays, :dims]), rays


def water_level(backend, xy, top, bottom, step=None, level=0.5) -> np.ndarray:
    """The height of the free surface above every gauge position `xy` ([n, dims − 1]; 2-D handles: [n]): one ray per gauge from
    the height `top` downwards along the last axis to `bottom`, the first entry into ``S >= level``; the middle of the final
    bracket as a height, NaN where the column is dry."""
    D = backend.D
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, D - 1)
    o = np.concatenate([xy, np.full((len(xy), 1), float(top))], axis=1)
    d = np.zeros_like(o)
    d[:, D - 1] = -1.0
    r = backend.cast_rays(o, d, float(top) - float(bottom), step=step, level=level, mode="enter", fields=("status", "bracket"))
    return float(top) - 0.5 * (r["bracket"][:, 0] + r["bracket"][:, 1])


def pixel_origins(origin, u, v, shape) -> np.ndarray:
    """The origins of the rays of an image of `shape` = (rows, columns): pixel [r, c] starts at ``origin + c·u + r·v``,
    returned as [rows · columns, dims] with the column fastest."""
    origin, u, v = (np.asarray(q, dtype=np.float64) for q in (origin, u, v))
    rows, cols = (int(s) for s in shape)
    r, c = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing="ij")
    return (origin[None, None, :] + c[..., None] * u[None, None, :] + r[..., None] * v[None, None, :]).reshape(rows * cols, -1)


def depth_image(backend, origin, u, v, shape, direction, t_end, step=None, level=0.5, mode="enter") -> dict:
    """Parallel rays along `direction` from the pixel lattice of `pixel_origins`: `t` [rows, columns] — the parameter of the
    hit, the depth where `direction` is a unit vector — `point` [rows, columns, 3] and `status`, NaN where nothing was hit."""
    o = pixel_origins(origin, u, v, shape)
    d = np.broadcast_to(np.asarray(direction, dtype=np.float64), o.shape)
    r = backend.cast_rays(o, d, t_end, step=step, level=level, mode=mode, fields=("status", "bracket", "point"))
    rows, cols = (int(s) for s in shape)
    return {"t": hit_parameter(r, mode).reshape(rows, cols), "point": r["point"].reshape(rows, cols, 3),
            "status": r["status"].reshape(rows, cols)}


__all__ = ["MODES", "REFINE_ROUNDS", "FOUND", "STARTS_INSIDE", "normalize", "intervals", "march_t", "refine_u", "ray_points", "crosses",
           "restate", "hit_parameter", "hit_points", "water_level", "pixel_origins", "depth_image"]
