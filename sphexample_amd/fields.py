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


__all__ = ["grid_axes", "grid_nodes", "surface_height", "free_surface_mask", "FREE_SURFACE_DIV_R"]
