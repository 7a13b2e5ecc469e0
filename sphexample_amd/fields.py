"""Fields on a regular lattice, on top of ``Backend.sample_grid``, and a free-surface mask on top of
``Backend.particle_fields`` (host only).

The device delivers, per lattice node, the probes' sums (``sphexample_amd.probes``): the Shepard sum ``S`` — about 1 inside the
fluid, about 1/2 at a free surface, 0 in empty space — and the S-weighted means of pressure, density and velocity.  Arrays
are shaped ``counts[::-1]``: x runs fastest, the order of VTK image data, and the LAST lattice axis (y in 2-D, z in 3-D) is
array axis 0.  That last axis is the vertical of the dam-break cases.
"""
from __future__ import annotations

import numpy as np

from .probes import water_level


def _lattice(origin, spacing, counts):
    o = np.asarray(origin, dtype=np.float64).reshape(-1)
    s = np.asarray(spacing, dtype=np.float64).reshape(-1)
    c = np.asarray(counts, dtype=np.int64).reshape(-1)
    if not (len(o) == len(s) == len(c)) or len(o) not in (2, 3):
        raise ValueError("origin, spacing and counts hold 2 or 3 entries each")
    if not np.isfinite(o).all() or not (np.isfinite(s) & (s > 0)).all() or (c < 1).any():
        raise ValueError("a finite origin, finite positive spacings and counts of at least 1 are needed")
    return o, s, c


def grid_axes(origin, spacing, counts):
    """The node coordinates per axis, formed as the kernel forms them: ``origin[d] + float(i) * spacing[d]``, one
    multiply and one add in double precision."""
    o, s, c = _lattice(origin, spacing, counts)
    return [o[d] + np.arange(int(c[d]), dtype=np.float64) * s[d] for d in range(len(o))]


def grid_nodes(origin, spacing, counts) -> np.ndarray:
    """The coordinates of every lattice node, ``[nodes, dims]``, in node order: index = i + nx * (j + ny * k), x fastest —
    row n of it belongs to entry n of every (flattened) array ``Backend.sample_grid`` returns."""
    ax = grid_axes(origin, spacing, counts)
    mesh = np.meshgrid(*ax[::-1], indexing="ij")           # slowest axis first: C order then runs x fastest
    return np.stack([m.reshape(-1) for m in mesh[::-1]], axis=1)


def surface_height(weight, origin, spacing, threshold: float = 0.5) -> np.ndarray:
    """The free-surface height over the lattice's footprint: `probes.water_level` applied to every vertical column.
    `weight` is the Shepard sum as ``Backend.sample_grid`` shapes it, ``(ny, nx)`` in 2-D (vertical: y) or ``(nz, ny, nx)``
    in 3-D (vertical: z); returns ``(nx,)`` or ``(ny, nx)``.  A dry column reads the height of the lowest node, a
    submerged one that of the highest."""
    S = np.asarray(weight, dtype=np.float64)
    if S.ndim not in (2, 3):
        raise ValueError("surface_height: weight is shaped (ny, nx) or (nz, ny, nx)")
    o = np.asarray(origin, dtype=np.float64).reshape(-1)
    s = np.asarray(spacing, dtype=np.float64).reshape(-1)
    if len(o) != S.ndim or len(s) != S.ndim:
        raise ValueError("surface_height: origin and spacing hold one entry per lattice axis")
    z = o[-1] + np.arange(S.shape[0], dtype=np.float64) * s[-1]
    cols = S.reshape(S.shape[0], -1).T                      # [columns, heights]
    return np.asarray(water_level(z, cols, threshold)).reshape(S.shape[1:])


# the usual cuts on div r for a free-surface particle (about dims inside the fluid, lower where the support is cut off)
FREE_SURFACE_DIV_R = {2: 1.5, 3: 2.4}


def free_surface_mask(div_r, dims: int, threshold: float = None) -> np.ndarray:
    """True where a particle lies at a free surface: ``div_r < threshold``, with `div_r` the field of that name of
    ``Backend.particle_fields`` — about `dims` inside the fluid, lower where a part of the kernel support is empty.  The
    default threshold is 1.5 in 2-D and 2.4 in 3-D: the values in common use in the SPH literature, conventions taken over
    as they are, not measured on this engine's cases.  Boundary rows at the edge of the particle set are flagged like any
    other row; select by Type where only the fluid is wanted."""
    if dims not in FREE_SURFACE_DIV_R:
        raise ValueError("free_surface_mask: dims is 2 or 3")
    t = FREE_SURFACE_DIV_R[dims] if threshold is None else float(threshold)
    return np.asarray(div_r, dtype=np.float64) < t


# ---- clouds for ``Backend.sample_points``: a line of points, the panels of a surface mesh and the load on it ---------------------
def segment(a, b, n: int) -> np.ndarray:
    """`n` points from `a` to `b`, both included, evenly spaced: ``[n, dims]`` (n = 1: `a`)."""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    if len(a) != len(b) or len(a) not in (2, 3) or int(n) < 1:
        raise ValueError("segment: two points of 2 or 3 coordinates each and n >= 1 are needed")
    t = np.linspace(0.0, 1.0, int(n))[:, None] if int(n) > 1 else np.zeros((1, 1))
    return a[None, :] + t * (b - a)[None, :]


def _mesh(vertices, elements):
    v = np.asarray(vertices, dtype=np.float64)
    e = np.asarray(elements, dtype=np.int64)
    if v.ndim != 2 or v.shape[1] not in (2, 3) or e.ndim != 2 or e.shape[1] != v.shape[1]:
        raise ValueError("a mesh is vertices [nv, dims] and elements [ne, dims]: triangles in 3-D, segments in 2-D")
    if e.size and (e.min() < 0 or e.max() >= len(v)):
        raise ValueError("an element names a vertex the mesh does not have")
    return v, e


def triangle_centroids(vertices, triangles) -> np.ndarray:
    """The centroid of every element of a surface mesh, ``[ne, dims]`` — the points to hand to ``Backend.sample_points``.
    `triangles` is ``[ne, 3]`` vertex indices in 3-D; in 2-D the mesh is segments, ``[ne, 2]``, and the centroid the midpoint."""
    v, e = _mesh(vertices, triangles)
    return v[e].mean(axis=1)


def _area_vectors(v, e):
    """A_k n̂_k of every element: half the cross product of two edges (3-D, the normal the right-hand rule gives the vertex
    order); the segment a → b turned a quarter to the right, (dy, −dx) (2-D: outward on a counter-clockwise polygon)."""
    p = v[e]
    if v.shape[1] == 3:
        return 0.5 * np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    d = p[:, 1] - p[:, 0]
    return np.stack([d[:, 1], -d[:, 0]], axis=1)


def surface_load(vertices, triangles, pressure, about=None):
    """The pressure load on a surface mesh: the force ``−Σ p_k A_k n̂_k`` with `pressure` [ne] the pressure at the element
    centroids (``Backend.sample_points(triangle_centroids(...))["pressure"]``), A_k the element's area and n̂_k its normal —
    out of the body for triangles ordered counter-clockwise seen from outside.  In 2-D the mesh is segments, the normal lies
    to the right of a → b (out of a counter-clockwise polygon) and the result is a force per unit width.  With `about`
    (a point) returns ``(force, moment)``, the moment ``Σ (c_k − about) × f_k`` of the element forces applied at the centroids:
    a vector in 3-D, the z component in 2-D.  One-point quadrature: exact for the force of a pressure that is linear over
    each element."""
    v, e = _mesh(vertices, triangles)
    p = np.asarray(pressure, dtype=np.float64).reshape(-1)
    if len(p) != len(e):
        raise ValueError("surface_load: one pressure per element is needed")
    f = -p[:, None] * _area_vectors(v, e)
    force = f.sum(axis=0)
    if about is None:
        return force
    r = v[e].mean(axis=1) - np.asarray(about, dtype=np.float64).reshape(1, -1)
    if r.shape[1] != v.shape[1]:
        raise ValueError("surface_load: `about` holds one coordinate per axis")
    moment = np.cross(r, f).sum(axis=0) if v.shape[1] == 3 else float((r[:, 0] * f[:, 1] - r[:, 1] * f[:, 0]).sum())
    return force, moment


# ---- gradients at arbitrary points, from the raw sums of ``Backend.sample_point_gradients`` ----------------------------------------
# The device delivers, per point, S = Σ V_j W, SA = Σ V_j A_j W and GA[b] = Σ V_j A_j ∂W/∂x_b for A = 1 (G), the pressure, the density
# and every velocity component.  GA alone is the gradient of the kernel interpolant of A — it carries the error of the particle
# disorder and, at a free surface, the gradient of the fill itself.  The Shepard-corrected difference form
#     ∇A ≈ (GA − (SA / S) · G) / S            (= Σ V_j (A_j − Ā) ∇W / S with Ā = SA / S the Shepard mean at the point)
# is exact for a constant A whatever the disorder and the cut of the support; it is what every helper below forms, wherever
# S ≥ `min_weight`, and NaN elsewhere (too little fluid within H to speak of a gradient).
MIN_GRADIENT_WEIGHT = 0.1


def _corrected_gradient(sums, ga: str, sa: str, min_weight: float) -> np.ndarray:
    S = np.asarray(sums["weight"], dtype=np.float64)
    G = np.asarray(sums["grad_weight"], dtype=np.float64)
    GA = np.asarray(sums[ga], dtype=np.float64)
    SA = np.asarray(sums[sa], dtype=np.float64)
    n = len(S)
    if G.shape != (n, 3) or GA.shape[:1] != (n,) or GA.shape[-1] != 3 or SA.shape != GA.shape[:-1]:
        raise ValueError(f"the sums of sample_point_gradients are needed: weight [n], grad_weight [n, 3], {sa} and {ga} [.., 3]")
    ok = S >= float(min_weight)
    Ss = np.where(ok, S, 1.0)
    lead = (n,) + (1,) * (GA.ndim - 1)
    mean = SA / Ss.reshape((n,) + (1,) * (SA.ndim - 1))
    out = (GA - mean[..., None] * G.reshape((n,) + (1,) * (GA.ndim - 2) + (3,))) / Ss.reshape(lead)
    out[~ok] = np.nan
    return out


def velocity_gradient(sums, min_weight: float = MIN_GRADIENT_WEIGHT) -> np.ndarray:
    """``L[p, a, b] = ∂v_a/∂x_b`` at every point, ``[n, 3, 3]``, from the dict of ``Backend.sample_point_gradients`` (the keys
    `weight`, `grad_weight`, `sum_velocity`, `grad_velocity`): the Shepard-corrected difference form where
    ``weight >= min_weight``, NaN elsewhere.  2-D: the z row and column are zero."""
    return _corrected_gradient(sums, "grad_velocity", "sum_velocity", min_weight)


def vorticity_at(sums, min_weight: float = MIN_GRADIENT_WEIGHT) -> np.ndarray:
    """``ω = ∇ × v`` at every point, ``[n, 3]`` (2-D: only ω_z is non-zero); a rigid rotation v = Ω × x gives 2Ω, the sign of
    ``Backend.particle_fields``."""
    L = velocity_gradient(sums, min_weight)
    return np.stack([L[:, 2, 1] - L[:, 1, 2], L[:, 0, 2] - L[:, 2, 0], L[:, 1, 0] - L[:, 0, 1]], axis=1)


def divergence_at(sums, min_weight: float = MIN_GRADIENT_WEIGHT) -> np.ndarray:
    """``∇·v`` at every point, ``[n]``: the trace of `velocity_gradient`."""
    L = velocity_gradient(sums, min_weight)
    return L[:, 0, 0] + L[:, 1, 1] + L[:, 2, 2]


def strain_rate(sums, min_weight: float = MIN_GRADIENT_WEIGHT) -> np.ndarray:
    """The rate-of-strain tensor ``½ (L + Lᵀ)`` at every point, ``[n, 3, 3]`` — times 2μ the viscous stress on a panel."""
    L = velocity_gradient(sums, min_weight)
    return 0.5 * (L + np.swapaxes(L, 1, 2))


def pressure_gradient(sums, min_weight: float = MIN_GRADIENT_WEIGHT) -> np.ndarray:
    """``∇P`` at every point, ``[n, 3]`` (the keys `weight`, `grad_weight`, `sum_pressure`, `grad_pressure`)."""
    return _corrected_gradient(sums, "grad_pressure", "sum_pressure", min_weight)


def surface_normal_at(sums, min_weight: float = MIN_GRADIENT_WEIGHT) -> np.ndarray:
    """The unit normal OUT of the fluid at every point, ``[n, 3]``: ``−G / |G|`` with G the gradient of the colour function
    Σ V_j W, which points into the fluid where the support is cut off.  NaN where ``weight < min_weight`` or G vanishes
    (deep inside the fluid G is small and its direction noise: use it near the surface, say ``weight`` below 0.9)."""
    S = np.asarray(sums["weight"], dtype=np.float64)
    G = np.asarray(sums["grad_weight"], dtype=np.float64)
    if G.shape != (len(S), 3):
        raise ValueError("surface_normal_at: weight [n] and grad_weight [n, 3] are needed")
    norm = np.sqrt((G * G).sum(axis=1))
    ok = (S >= float(min_weight)) & (norm > 0.0)
    out = -G / np.where(ok, norm, 1.0)[:, None]
    out[~ok] = np.nan
    return out


# ---- the linear fit at arbitrary points, from the raw sums of ``Backend.sample_point_moments`` --------------------------------------
# A Shepard mean SA / S returns the field at the kernel-weighted centroid of the neighbours, not at the point: on a wall, on the bed
# and within H of the free surface, where the support is one-sided, that is a fraction of h inside the fluid.  With the moments
#     S = Σ w    M1 = Σ w e    M2 = Σ w e ⊗ e    SA = Σ w A    A1 = Σ w A e        (e = x_j − x)
# the weighted least-squares plane a + b·e through the neighbours' values solves, per point and field,
#     [[S, M1ᵀ], [M1, M2]] · [a; b] = [SA; A1]
# — the linear reconstruction mDBC makes at its ghost nodes.  a is the field AT the point, b its gradient, both exact for a linear
# field whatever the disorder and the cut of the support.  The system is solved with the offsets in units of h and divided by S:
# its matrix is then dimensionless — 1 in the corner, the centroid offset / h beside it, the second moments / h² — and its
# reciprocal condition number λ_min / λ_max means the same at every resolution.  Where the support cannot carry a plane the
# point keeps the Shepard mean.  LINEAR_FIT_MIN_RCOND: supports on one line (2-D) or in one plane (3-D) reach 1.6e-16 at the most
# (rounding); the most one-sided full-rank supports of the 700-point clouds on the shipped dam-break fixtures — D + 1 rows or more,
# S ≥ MIN_GRADIENT_WEIGHT — reach 5.4e-3 (2-D) and 3.5e-3 (3-D) at the least (profiles/point_moments.md, "The threshold").  The
# constant is the geometric middle of that gap, 7e-10, in a round figure.  A fit amplifies the error of the sums by 1 / rcond at
# the worst: callers who feed it the sums of an fp32 handle (2e-4) may want a higher floor.
LINEAR_FIT_MIN_RCOND = 1e-9


def _moment_system(sums, h, dims):
    """S [n], the scaled matrices [n, D + 1, D + 1] and their reciprocal condition numbers [n] (0 where S is not positive)."""
    h = float(sums["h"] if h is None else h)
    D = int(sums["dims"] if dims is None else dims)
    if D not in (2, 3) or not h > 0.0:
        raise ValueError("linear_fit: dims is 2 or 3 and h positive (the dict of Backend.sample_point_moments carries both)")
    S = np.asarray(sums["weight"], dtype=np.float64)
    M1 = np.asarray(sums["moment1"], dtype=np.float64)
    M2 = np.asarray(sums["moment2"], dtype=np.float64)
    n = len(S)
    if S.ndim != 1 or M1.shape != (n, 3) or M2.shape != (n, 3, 3):
        raise ValueError("the sums of sample_point_moments are needed: weight [n], moment1 [n, 3], moment2 [n, 3, 3]")
    some = S > 0.0
    Ss = np.where(some, S, 1.0)
    A = np.zeros((n, D + 1, D + 1))
    A[:, 0, 0] = 1.0
    A[:, 0, 1:] = A[:, 1:, 0] = M1[:, :D] / (Ss * h)[:, None]
    A[:, 1:, 1:] = M2[:, :D, :D] / (Ss * h * h)[:, None, None]
    A[~some] = 0.0
    lam = np.linalg.eigvalsh(A) if n else np.zeros((0, D + 1))                     # ascending; A is a Gram matrix: λ ≥ 0 up to rounding
    top = lam[:, -1]
    rcond = np.where(some & (top > 0.0), np.maximum(lam[:, 0], 0.0) / np.where(top > 0.0, top, 1.0), 0.0)
    return h, D, S, A, rcond


def linear_fit_rcond(sums, h: float = None, dims: int = None) -> np.ndarray:
    """The reciprocal condition number λ_min / λ_max of every point's scaled moment matrix, ``[n]`` — what `linear_fit` holds
    against `min_rcond`; 0 where ``weight`` is not positive."""
    return _moment_system(sums, h, dims)[4]


def linear_fit(sums, min_count: int = None, min_rcond: float = LINEAR_FIT_MIN_RCOND, h: float = None, dims: int = None) -> dict:
    """Pressure, density and velocity AT the points and their gradients, from the dict of ``Backend.sample_point_moments``: the
    weighted least-squares plane through the neighbours' values, exact for a linear field however one-sided the support.
    Returns `pressure`, `density` [n], `velocity` [n, 3], `pressure_gradient`, `density_gradient` [n, 3], `velocity_gradient`
    [n, 3, 3] (entry [a, b] = ∂v_a/∂x_b), `linear` [n] bool — the points that were fitted — and `rcond` [n], the reciprocal
    condition number of every point's system.  A point with fewer than `min_count` rows (default dims + 1), with ``weight`` below
    `MIN_GRADIENT_WEIGHT` or with ``rcond < min_rcond`` keeps the Shepard means SA / S, gets zero gradients and
    ``linear == False``; a point without rows reads zeros.  2-D: the z entries are zero.  `h` and `dims` default to the entries
    of those names the backend puts into the dict."""
    h, D, S, A, rcond = _moment_system(sums, h, dims)
    n = len(S)
    cnt = np.asarray(sums["count"])
    SA = np.concatenate([np.asarray(sums["sum_pressure"], dtype=np.float64).reshape(n, 1), np.asarray(sums["sum_density"], dtype=np.float64).reshape(n, 1),
                         np.asarray(sums["sum_velocity"], dtype=np.float64).reshape(n, 3)], axis=1)                       # [n, 5]
    A1 = np.concatenate([np.asarray(sums["moment_pressure"], dtype=np.float64).reshape(n, 1, 3), np.asarray(sums["moment_density"], dtype=np.float64).reshape(n, 1, 3),
                         np.asarray(sums["moment_velocity"], dtype=np.float64).reshape(n, 3, 3)], axis=1)                 # [n, 5, 3]
    need = D + 1 if min_count is None else int(min_count)
    some = (cnt > 0) & (S > 0.0)
    fit = some & (cnt >= need) & (S >= MIN_GRADIENT_WEIGHT) & (rcond >= float(min_rcond))
    Ss = np.where(some, S, 1.0)
    value = np.where(some[:, None], SA / Ss[:, None], 0.0)                         # the Shepard means: what a point keeps without a fit
    grad = np.zeros((n, 5, 3))
    if fit.any():
        rhs = np.concatenate([SA[fit][:, None, :] / S[fit][:, None, None], np.swapaxes(A1[fit][:, :, :D], 1, 2) / (S[fit] * h)[:, None, None]], axis=1)
        sol = np.linalg.solve(A[fit], rhs)                                         # [m, D + 1, 5]: a, then b · h
        value[fit] = sol[:, 0, :]
        g = np.zeros((int(fit.sum()), 5, 3))
        g[:, :, :D] = np.swapaxes(sol[:, 1:, :], 1, 2) / h
        grad[fit] = g
    if D == 2:
        value[:, 4] = 0.0
    return {"pressure": value[:, 0].copy(), "density": value[:, 1].copy(), "velocity": value[:, 2:5].copy(),
            "pressure_gradient": grad[:, 0].copy(), "density_gradient": grad[:, 1].copy(), "velocity_gradient": grad[:, 2:5].copy(),
            "linear": fit, "rcond": rcond}


def _fitted_velocity_gradient(sums, **kw):
    """∂v_a/∂x_b of `linear_fit`, NaN where the point was not fitted — the convention of `velocity_gradient`."""
    f = sums if "velocity_gradient" in sums and "linear" in sums else linear_fit(sums, **kw)
    L = np.array(f["velocity_gradient"], dtype=np.float64)
    L[~np.asarray(f["linear"], dtype=bool)] = np.nan
    return L


def vorticity_linear(sums, **kw) -> np.ndarray:
    """``ω = ∇ × v`` at every point, ``[n, 3]``, from the velocity gradient of `linear_fit` (`sums`: the dict of
    ``Backend.sample_point_moments``, or the result of `linear_fit` itself; keywords go to `linear_fit`): shaped and signed
    like `vorticity_at`, NaN where the point was not fitted."""
    L = _fitted_velocity_gradient(sums, **kw)
    return np.stack([L[:, 2, 1] - L[:, 1, 2], L[:, 0, 2] - L[:, 2, 0], L[:, 1, 0] - L[:, 0, 1]], axis=1)


def divergence_linear(sums, **kw) -> np.ndarray:
    """``∇·v`` at every point, ``[n]``: the trace of the velocity gradient of `linear_fit`; NaN where the point was not fitted."""
    L = _fitted_velocity_gradient(sums, **kw)
    return L[:, 0, 0] + L[:, 1, 1] + L[:, 2, 2]


def strain_rate_linear(sums, **kw) -> np.ndarray:
    """The rate-of-strain tensor ``½ (L + Lᵀ)`` at every point, ``[n, 3, 3]``, of the velocity gradient of `linear_fit`; NaN
    where the point was not fitted."""
    L = _fitted_velocity_gradient(sums, **kw)
    return 0.5 * (L + np.swapaxes(L, 1, 2))


def surface_load_linear(vertices, triangles, backend, about=None, **kw):
    """`surface_load` with the FITTED pressure at the element centroids: the centroids are sampled with
    ``backend.sample_point_moments`` and `linear_fit` (keywords go to it) gives the pressure at the panels themselves, not a
    fraction of h inside the fluid; panels that could not be fitted keep the Shepard mean, dry ones read zero."""
    sums = backend.sample_point_moments(triangle_centroids(vertices, triangles))
    return surface_load(vertices, triangles, linear_fit(sums, **kw)["pressure"], about=about)


__all__ = ["grid_axes", "grid_nodes", "surface_height", "free_surface_mask", "FREE_SURFACE_DIV_R", "segment", "triangle_centroids",
           "surface_load", "MIN_GRADIENT_WEIGHT", "velocity_gradient", "vorticity_at", "divergence_at", "strain_rate",
           "pressure_gradient", "surface_normal_at", "LINEAR_FIT_MIN_RCOND", "linear_fit", "linear_fit_rcond", "vorticity_linear",
           "divergence_linear", "strain_rate_linear", "surface_load_linear"]
