"""Selections for ``Backend.select`` (sphmi_select_build, csrc/sphmi_select.h): which rows of an output cross the bus.

A row is selected iff EVERY enabled clause of a `Selection` holds; the boxes inside the spatial clause are ORed::

    rows, got = eng.select(Selection(types=("Fluid",), field="Pressure", field_lo=500.0), fields=("Position", "Pressure"))
    rows, got = eng.select(slab(1, 0.31, eng.cfg.H))                 # a slice one cell thick, every field
    rows, got = eng.select(every(8))                                 # the same particles in every frame: keyed on ID
    rows, got = eng.select(where(free_surface_mask(f["div_r"], 2)))  # what an on-demand result flagged, without the state crossing first

``rows`` are ascending row numbers of what ``download`` delivers at the same point, and every array of ``got`` equals
``download()[name][rows]`` byte for byte.  `restate` forms the same row list in numpy from a full Float64 download, bit for bit what
the device selects.  No device, no library: numpy only."""
from __future__ import annotations

import dataclasses
from typing import Optional, Sequence, Tuple

import numpy as np

TYPES = {"Fluid": 1, "Fixed": 2, "Moving": 3}
FIELDS = {None: 0, "Density": 1, "Pressure": 2, "Speed2": 3}           # SPHMI_SELECT_FIELD_*
MAX_BOXES = MAX_MARKERS = 16


@dataclasses.dataclass
class Selection:
    """Mirrors ``sphmi_selection``.  `types`: names ("Fluid", "Fixed", "Moving") or Type numbers, never empty.  `boxes`: a sequence of
    ``(lo, hi)``, `dims` bounds each, half-open ``lo <= x < hi`` per axis, ``-inf`` / ``+inf`` allowed; the row must lie in one of them.
    `markers`: the GroupMarkers kept.  `id_stride`, `id_phase`: keep ``uint64(ID) % id_stride == id_phase``.  `field`: "Density",
    "Pressure" or "Speed2" (``(vx * vx + vy * vy) + vz * vz``) kept where ``field_lo <= value <= field_hi``; a NaN never is.
    `mask`: one entry per row in the CURRENT order, non-zero keeps."""
    types: Sequence = ("Fluid", "Fixed", "Moving")
    boxes: Sequence = ()
    markers: Sequence[int] = ()
    id_stride: int = 1
    id_phase: int = 0
    field: Optional[str] = None
    field_lo: float = -np.inf
    field_hi: float = np.inf
    mask: Optional[np.ndarray] = None

    def type_mask(self) -> int:
        """Bit (Type - 1): 1 Fluid, 2 Fixed, 4 Moving."""
        types = (self.types,) if isinstance(self.types, (str, int, np.integer)) else tuple(self.types)
        m = 0
        for t in types:
            if isinstance(t, str) and t not in TYPES:
                raise ValueError(f"Selection: unknown type {t!r} (one of {sorted(TYPES)})")
            m |= 1 << ((TYPES[t] if isinstance(t, str) else int(t)) - 1)
        return m

    def field_code(self) -> int:
        if self.field not in FIELDS:
            raise ValueError(f"Selection: unknown field {self.field!r} (one of {[k for k in FIELDS if k]})")
        return FIELDS[self.field]

    def box_tables(self, dims: int) -> Tuple[np.ndarray, np.ndarray]:
        """(lo, hi), float64 [n_boxes, dims] each."""
        lo = np.ascontiguousarray([np.asarray(b[0], dtype=np.float64) for b in self.boxes], dtype=np.float64).reshape(-1, dims)
        hi = np.ascontiguousarray([np.asarray(b[1], dtype=np.float64) for b in self.boxes], dtype=np.float64).reshape(-1, dims)
        if lo.shape != hi.shape or len(lo) != len(self.boxes):
            raise ValueError(f"Selection: every box is (lo, hi) of {dims} bounds each")
        return lo, hi

    def mask_bytes(self, n: int) -> Optional[np.ndarray]:
        """The mask as the library takes it: uint8 [n], 1 where the entry is non-zero (None: no clause)."""
        if self.mask is None:
            return None
        m = np.asarray(self.mask)
        if m.shape != (n,):
            raise ValueError(f"Selection: the mask holds one entry per row ({n})")
        return np.ascontiguousarray(m != 0, dtype=np.uint8)


def slab(axis: int, centre: float, thickness: float, dims: int = None, **clauses) -> Selection:
    """The rows with ``centre - thickness / 2 <= x[axis] < centre + thickness / 2``: a slice through the domain, unbounded along the
    other axes.  `dims` defaults to ``axis + 1`` for the last axis and must be given otherwise; further clauses as keywords."""
    dims = axis + 1 if dims is None else int(dims)
    if not 0 <= axis < dims <= 3:
        raise ValueError("slab: 0 <= axis < dims <= 3")
    lo, hi = np.full(dims, -np.inf), np.full(dims, np.inf)
    lo[axis], hi[axis] = float(centre) - 0.5 * float(thickness), float(centre) + 0.5 * float(thickness)
    return Selection(boxes=((lo, hi),), **clauses)


def every(k: int, phase: int = 0, **clauses) -> Selection:
    """Every k-th particle by ID — the same particles whatever the row order."""
    return Selection(id_stride=int(k), id_phase=int(phase), **clauses)


def where(mask, **clauses) -> Selection:
    """The rows a mask in the current row order flags (``fields.free_surface_mask``, ``components.main_body_mask``, …)."""
    return Selection(mask=np.asarray(mask), **clauses)


def speed2(velocity) -> np.ndarray:
    """``(vx * vx + vy * vy) + vz * vz`` of float64 velocities [n, 2 or 3], one rounding per operation (2 columns: vz = 0)."""
    v = np.asarray(velocity, dtype=np.float64)
    s = v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]
    return s + v[:, 2] * v[:, 2] if v.shape[1] > 2 else s + 0.0


def keep_mask(spec: Selection, fields: dict) -> np.ndarray:
    """bool [n]: the selection rule on a full Float64 download `fields` (only the arrays the enabled clauses read are looked at)."""
    typ = np.asarray(fields["Type"]).astype(np.int64)
    n = len(typ)
    tm = spec.type_mask()
    ok = (typ >= 1) & (typ <= 3)
    keep = ok & (((tm >> np.where(ok, typ - 1, 0)) & 1) == 1)
    if len(spec.boxes):
        x = np.asarray(fields["Position"])
        if x.dtype != np.float64:
            raise ValueError("restate: the clauses read the Float64 download")
        dims = len(np.asarray(spec.boxes[0][0]).reshape(-1))
        lo, hi = spec.box_tables(dims)
        anybox = np.zeros(n, dtype=bool)
        for b in range(len(lo)):
            inside = np.ones(n, dtype=bool)
            for d in range(dims):
                inside &= (lo[b, d] <= x[:, d]) & (x[:, d] < hi[b, d])
            anybox |= inside
        keep &= anybox
    if len(spec.markers):
        keep &= np.isin(np.asarray(fields["GroupMarker"]).astype(np.uint64), np.asarray(list(spec.markers), dtype=np.uint64))
    if spec.id_stride > 1:
        keep &= np.asarray(fields["ID"]).astype(np.int64).view(np.uint64) % np.uint64(spec.id_stride) == np.uint64(spec.id_phase)
    code = spec.field_code()
    if code:
        src = np.asarray(fields["Velocity" if code == 3 else spec.field])
        if src.dtype != np.float64:
            raise ValueError("restate: the clauses read the Float64 download")
        v = speed2(src) if code == 3 else src
        with np.errstate(invalid="ignore"):
            keep &= (float(spec.field_lo) <= v) & (v <= float(spec.field_hi))
    m = spec.mask_bytes(n)
    if m is not None:
        keep &= m != 0
    return keep


def restate(spec: Selection, fields: dict) -> np.ndarray:
    """The rows ``Backend.select`` returns for `spec`, int32 ascending, from a full Float64 download `fields` taken at the same point
    (``components`` = dims or 3 alike: the clauses read the first `dims` columns) — bit for bit what the device selects."""
    return np.flatnonzero(keep_mask(spec, fields)).astype(np.int32)
