"""ctypes view of include/sphmi.h (structs, the prototype table + a thin call-marshalling base class).

``SphmiConfig`` / ``SphmiProgress`` must stay field-for-field identical to the C structs;
``tests/test_abi.py`` cross-checks the sizes against the compiled library.  ``PROTOTYPES`` holds the
ctypes prototype of every entry point Python calls; ``tests/test_prototype_table_host.py`` holds it to the headers.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from .config import (NoMDBC, SimpleMDBC, SimulationConstants, SimulationMetaData, SPHDensityDiffusion,
                     SPHKernelInstance, SPHViscosity)

ABI_VERSION = 5
MAX_DEVICES = 16
MAX_COLUMNS = 16
MAX_COLUMN_ROW_BYTES = 64
MAX_FORCE_GROUPS = 16
MAX_PROBES = 1024
MAX_GRID_NODES = 1 << 24
MAX_SAMPLE_POINTS = 1 << 24
MAX_RAYS = 1 << 20
MAX_RAY_POINTS = 1 << 16
RAY_REFINE_ROUNDS = 4
RAY_ENTER, RAY_LEAVE, RAY_ANY = 0, 1, 2
NEIGHBORS_FULL, NEIGHBORS_HALF = 0, 1
MAX_SELECT_BOXES = MAX_SELECT_MARKERS = 16
SELECT_FIELD_NONE, SELECT_FIELD_DENSITY, SELECT_FIELD_PRESSURE, SELECT_FIELD_SPEED2 = range(4)

OK, ERR_ARGUMENT, ERR_DEVICE, ERR_NUMERIC, ERR_DOMAIN, ERR_STATE = range(6)


class SphmiConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("abi_version", C.c_int32), ("dims", C.c_int32),
        ("host_float_bytes", C.c_int32), ("device_float_bytes", C.c_int32), ("kernel", C.c_int32),
        ("viscosity", C.c_int32), ("density_diffusion", C.c_int32), ("mdbc", C.c_int32),
        ("device", C.c_int32), ("shifting", C.c_int32), ("kernel_output", C.c_int32),
        ("n_particles", C.c_int64), ("max_cells", C.c_int64),
        ("rho0", C.c_double), ("dx", C.c_double), ("m0", C.c_double), ("alpha", C.c_double),
        ("g", C.c_double), ("c0", C.c_double), ("gamma", C.c_double), ("delta_phi", C.c_double),
        ("CFL", C.c_double), ("Cb", C.c_double), ("nu0", C.c_double),
        ("k", C.c_double), ("h", C.c_double), ("h_inv", C.c_double), ("H", C.c_double),
        ("H_inv", C.c_double), ("H2", C.c_double), ("alphaD", C.c_double), ("eta2", C.c_double),
        ("blin_constant", C.c_double), ("smagorinsky_constant", C.c_double), ("cubic_eps", C.c_double),
        ("n_devices", C.c_int32), ("slab_axis", C.c_int32), ("devices", C.c_int32 * MAX_DEVICES),
    ]


class SphmiProgress(C.Structure):
    _fields_ = [
        ("iteration", C.c_int64), ("steps_done", C.c_int64), ("n_rebuilds", C.c_int64),
        ("index_counter", C.c_int64), ("total_time", C.c_double), ("last_dt", C.c_double),
        ("delta_x", C.c_double),
    ]


class SphmiMultiInfo(C.Structure):
    _fields_ = [("world", C.c_int32), ("n_local", C.c_int32), ("axis", C.c_int32), ("halo_width", C.c_int32),
                ("transport", C.c_int32), ("reserved", C.c_int32), ("n_recuts", C.c_int64),
                ("cuts", C.c_int64 * MAX_DEVICES), ("n_live", C.c_int64 * MAX_DEVICES)]


class SphmiSelection(C.Structure):
    _fields_ = [("type_mask", C.c_uint32), ("n_boxes", C.c_int32), ("box_lo", C.c_void_p), ("box_hi", C.c_void_p),
                ("n_markers", C.c_int32), ("markers", C.c_void_p), ("id_stride", C.c_int64), ("id_phase", C.c_int64),
                ("field", C.c_int32), ("field_lo", C.c_double), ("field_hi", C.c_double), ("row_mask", C.c_void_p)]


class SphmiError(RuntimeError):
    def __init__(self, status: int, text: str):
        super().__init__(f"sphmi status {status}: {text}")
        self.status = status


# -- the prototype of every entry point of include/sphmi.h and include/sphmi_internal.h that Python calls ---------------------
# unprefixed name → argtypes, or (argtypes, restype) where the function does not return int.  Array pointers travel as c_void_p,
# POINTER(...) stands where a byref is passed.  `bind` is the one place that applies an entry.
_P, _I32, _I64, _F = C.c_void_p, C.c_int32, C.c_int64, C.c_double
_pI32, _pI64, _pF, _pCfg = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(SphmiConfig)
_SERIES_TAIL = [_pI64, _pI64]              # n_out, n_dropped of every *_read of a step series
PROTOTYPES = {
    "backend_info": ([], C.c_char_p), "last_error": ([_P], C.c_char_p), "auto_device_float_bytes": ([_pCfg], C.c_int32),
    "create": [_pCfg, C.POINTER(_P)], "create_rank": [_pCfg, _I32, _I32, C.c_char_p, C.POINTER(_P)], "destroy": [_P],
    "device_float_bytes": [_P, _pI32], "owned_count": [_P, _pI64], "multi_info_get": [_P, C.POINTER(SphmiMultiInfo)],
    "rccl_unique_id": [_P], "rccl_probe": [],
    "dam_break_3d_count": [_F, _pI64, _pI64], "generate_dam_break_3d": [_P, _F],
    "upload": [_P] * 9, "set_clock": [_P, _I64, _F], "set_motion": [_P, C.c_uint64, _F, _F, _F, _P],
    "advance": [_P, _F, _I64, C.POINTER(SphmiProgress)],
    "download": [_P] * 11, "download_begin": [_P] * 11, "download_end": [_P], "set_output_components": [_P, C.c_int],
    "host_register": [_P, _P, _I64], "host_unregister": [_P, _P],
    "download_kernel_output": [_P, _P, _P], "download_permutation": [_P, _P],
    "attach_columns": [_P, _I32, _P, _P], "download_columns": [_P, _P], "download_columns_begin": [_P, _P],
    "forces_once": [_P, C.c_int, _P, _P], "unique_cells": [_P, _P, _I64, _pI64],
    "timers": [_P, _I32, C.POINTER(C.c_char_p), _pF, _pI64, _pI32], "force_kernel_stats": [_P, C.c_int, _pF, _pI64],
    "device_ptrs": [_P, C.POINTER(_P), C.POINTER(_P), _pI64],
    # the step series
    "group_forces_enable": [_P, _I32, _P, _I64], "group_forces_read": [_P, _I64] + [_P] * 4 + _SERIES_TAIL,
    "probes_enable": [_P, _I32, _P, _I64], "probes_read": [_P, _I64] + [_P] * 8 + _SERIES_TAIL,
    "probe_moments_enable": [_P, _I32, _P, _I64], "probe_moments_read": [_P, _I64] + [_P] * 13 + _SERIES_TAIL,
    "budgets_enable": [_P, _I64], "budgets_read": [_P, _I64] + [_P] * 10 + _SERIES_TAIL,
    "flow_enable": [_P, _I32, _P, _P, _I64], "flow_read": [_P, _I64] + [_P] * 8 + _SERIES_TAIL,
    "tracers_enable": [_P, _I32, _P, _I32, _P, _F, _I64], "tracers_read": [_P, _I64] + [_P] * 6 + _SERIES_TAIL,
    # the accumulated records
    "envelopes_enable": [_P, _I32], "envelopes_read": [_P, _pI64, _P] + [_P] * 8,
    "maps_enable": [_P, _P, _P, _P, _I32], "maps_disable": [_P], "maps_read": [_P, _pI64, _P] + [_P] * 14,
    # the results on demand
    "sample_grid": [_P] * 9, "sample_points": [_P, _I64] + [_P] * 6, "sample_point_gradients": [_P, _I64] + [_P] * 10,
    "sample_point_moments": [_P, _I64] + [_P] * 11,
    "cast_rays": [_P, _I64] + [_P] * 4 + [_F, _F, _I32] + [_P] * 9, "particle_fields": [_P] * 7,
    "neighbors_build": [_P, _I32, _pI64, _pI64], "neighbors_read": [_P] * 3, "neighbors_release": [_P],
    "isosurface_build": [_P] * 4 + [_F, _pI64, _pI64], "isosurface_read": [_P] * 5, "isosurface_release": [_P],
    "components_build": [_P, _F, C.c_uint32, _pI64, _pI64], "components_read": [_P] * 5, "components_release": [_P],
    "select_build": [_P, _P, _pI64, _pI64], "select_read": [_P, _P], "select_download": [_P] * 11, "select_download_columns": [_P, _P],
    "select_release": [_P],
    # include/sphmi_internal.h: the hooks of tests and tools
    "shm_selftest": [C.c_char_p, _I32, _I32, _I64], "plan_slabs": [_P, _P, _P, _I64, _I32] + [_P] * 5,
    "multi_set_cuts": [_P, _P, _I32], "multi_column_cost": [_P, _I64, _I32, _P], "multi_halo_info": [_P, _pI64, _I32, _pI32],
}


def bind(lib, name: str, prefix: str = "sphmi_"):
    """The entry point `prefix + name` of `lib` under its prototype of PROTOTYPES.  The prototype is assigned on every call:
    whoever widened it on the (shared) function object to call it raw leaves the next caller unharmed."""
    fn = getattr(lib, prefix + name)
    proto = PROTOTYPES[name]
    if isinstance(proto, tuple):
        proto, fn.restype = proto
    fn.argtypes = list(proto)
    return fn


def last_error(lib, handle=None, prefix: str = "sphmi_") -> str:
    return (bind(lib, "last_error", prefix)(handle) or b"").decode()


def make_config(n_particles: int, SimConstants: SimulationConstants, SimKernel: SPHKernelInstance,
                SimMetaData: SimulationMetaData, SimViscosity: SPHViscosity,
                SimDensityDiffusion: SPHDensityDiffusion, *, device_float_bytes: int = 0,
                host_float_bytes: int = 8, device: int = 0, max_cells: int = 0) -> SphmiConfig:
    """Flatten the reference's configuration objects into the C parameter block.

    Model tags the engine does not implement raise here, which is where the Julia shim falls back
    to the stock CPU path.  device_float_bytes: 4 / 8, or 0 = the library chooses
    (`sphmi_auto_device_float_bytes`: fp32 kernels when H >= 2h without mDBC, fp64 when the kernel is cut off before it vanishes or mDBC is on)."""
    for tag, what in ((SimViscosity, "viscosity"), (SimDensityDiffusion, "density diffusion")):
        if getattr(tag, "abi_value", None) is None:
            raise NotImplementedError(f"{type(tag).__name__}: {what} model not implemented by the engine")
    if getattr(SimKernel.kernel, "abi_value", None) is None:
        raise NotImplementedError(f"{type(SimKernel.kernel).__name__}: kernel not implemented by the engine")
    c = SphmiConfig()
    c.struct_size = C.sizeof(SphmiConfig)
    c.abi_version = ABI_VERSION
    c.dims = SimMetaData.Dimensions
    c.host_float_bytes = host_float_bytes
    c.device_float_bytes = device_float_bytes
    c.kernel = SimKernel.kernel.abi_value
    c.viscosity = SimViscosity.abi_value
    c.density_diffusion = SimDensityDiffusion.abi_value
    c.mdbc = 1 if SimMetaData.BMode is SimpleMDBC else 0
    c.shifting = 1 if SimMetaData.SMode.__name__ == "PlanarShifting" else 0
    c.kernel_output = 1 if SimMetaData.KMode.__name__ == "StoreKernelOutput" else 0
    c.cubic_eps = float(getattr(SimKernel.kernel, "eps", 0.0))
    c.blin_constant = SimConstants.BlinConstant
    c.smagorinsky_constant = SimConstants.SmagorinskyConstant
    c.device = device
    c.n_particles = n_particles
    c.max_cells = max_cells
    for k in ("rho0", "dx", "m0", "alpha", "g", "c0", "gamma", "delta_phi", "CFL", "Cb", "nu0"):
        setattr(c, k, getattr(SimConstants, k))
    for k in ("k", "h", "h_inv", "H", "H_inv", "H2", "alphaD", "eta2"):
        setattr(c, k, getattr(SimKernel, k))
    return c


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


_F64, _INT64 = np.float64, np.int64

# What sphmi_download delivers, in the order of its prototype: name, dtype (None: the host float), vector.  Host-float vectors
# have `components` columns on request; Cells always has dims.
DOWNLOAD_FIELDS = (("Position", None, True), ("Velocity", None, True), ("Acceleration", None, True), ("Density", None, False),
                   ("Pressure", None, False), ("ID", np.int64, False), ("Type", np.uint8, False), ("GroupMarker", np.uint64, False),
                   ("GhostPoints", None, True), ("Cells", np.int64, True))
DOWNLOAD_NAMES = tuple(k for k, _, _ in DOWNLOAD_FIELDS)

# has_<feature>() is true iff the library exports every one of these entry points
FEATURES = {
    "columns": ("attach_columns", "download_columns", "download_columns_begin"),
    "neighbor_list": ("neighbors_build", "neighbors_read", "neighbors_release"),
    "maps": ("maps_enable", "maps_read", "maps_disable"),
    **{k: (k + "_enable", k + "_read") for k in ("group_forces", "probes", "probe_moments", "budgets", "flow", "envelopes", "tracers")},
    **{k: (k + "_build", k + "_read", k + "_release") for k in ("isosurface", "components")},
    "select": ("select_build", "select_read", "select_download", "select_download_columns", "select_release"),
    **{k: (k,) for k in ("sample_grid", "sample_points", "sample_point_gradients", "sample_point_moments", "cast_rays", "particle_fields")},
}


class Backend:
    """Call marshalling shared by the HIP engine binding and (in tests) the oracle binding.

    A backend is `lib` + symbol `prefix`; every entry point has the signature declared in
    include/sphmi.h."""

    # what this object enabled, attached, pinned and built (class-level: objects made with __new__ start from them too)
    _column_widths = None
    _force_groups = _probes = _moment_probes = _flow_boxes = _map_bins = 0
    _tracers = (0, 0, 0.5)
    _pinned = ()
    _neighbor_shape = _isosurface_shape = _components_shape = _select_shape = None

    def __init__(self, lib: C.CDLL, prefix: str, cfg: SphmiConfig, create=None):
        self._lib, self._p = lib, prefix
        self.cfg = cfg
        self.N, self.D = int(cfg.n_particles), int(cfg.dims)
        self._ft = np.float64 if cfg.host_float_bytes == 8 else np.float32
        self._h = C.c_void_p()
        rc = (create or self._fn("create"))(C.byref(cfg), C.byref(self._h))
        if rc != OK:
            raise SphmiError(rc, last_error(lib, None, prefix))

    def _fn(self, name):
        return bind(self._lib, name, self._p)

    def _check(self, rc: int):
        if rc != OK:
            raise SphmiError(rc, last_error(self._lib, self._h, self._p))

    def _has(self, name: str) -> bool:
        return hasattr(self._lib, self._p + name)

    def _has_all(self, names) -> bool:
        return all(self._has(n) for n in names)

    def close(self):
        if self._h:
            self._fn("destroy")(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- the call shapes --------------------------------------------------------------------
    @staticmethod
    def empty_series(schema, *lead, steps: int = 0) -> dict:
        """The dict a series read delivers for `steps` steps, zeroed: iteration, time, dt and one [steps, *lead, *shape] array per
        (key, shape, dtype) of `schema`."""
        out = {"iteration": np.zeros(steps, dtype=np.int64), "time": np.zeros(steps), "dt": np.zeros(steps)}
        out.update({key: np.zeros((steps, *lead, *shape), dtype=dtype) for key, shape, dtype in schema})
        return out

    def _read_series(self, name, columns, *lead, tail=()) -> dict:
        """`<name>_read` of a step series: a call with capacity 0 learns how many steps wait, the second one fetches them.  `columns`
        is the (key, trailing shape, dtype) list behind iteration, time, dt, `lead` what stands in front of every trailing shape
        (the probes, boxes, groups); `tail` arrays that hold one state, not one row per step.  Returns the dict cut to the steps
        delivered and sets `<name>_dropped`."""
        f = self._fn(name + "_read")
        n, dropped = C.c_int64(), C.c_int64()
        self._check(f(self._h, 0, *[None] * (3 + len(columns) + len(tail)), C.byref(n), C.byref(dropped)))
        k = max(n.value, 1)
        out = self.empty_series(columns, *lead, steps=k)
        self._check(f(self._h, k, *[_ptr(a) for a in (*out.values(), *tail)], C.byref(n), C.byref(dropped)))
        setattr(self, name + "_dropped", dropped.value)
        return {key: a[:n.value] for key, a in out.items()}

    def _read_window(self, name, out) -> dict:
        """`<name>_read` of records accumulated since the enable: the steps, the time window, and the arrays of `out` filled."""
        steps, window = C.c_int64(), np.zeros(3)
        self._check(self._fn(name + "_read")(self._h, C.byref(steps), _ptr(window), *[_ptr(a) for a in out.values()]))
        return {"steps": int(steps.value), "t_begin": float(window[0]), "t_end": float(window[1]), "duration": float(window[2]), **out}

    @staticmethod
    def _wanted(who, table, fields):
        fields = tuple(table) if fields is None else tuple(fields)
        unknown = [k for k in fields if k not in table]
        if unknown:
            raise ValueError(f"{who}: unknown fields {unknown}")
        return fields

    def _sample(self, name, table, fields, lead, *inputs) -> dict:
        """A result with selectable outputs: `table` maps name → (dtype, trailing shape) in the order of the C prototype, behind
        `inputs`.  The outputs not in `fields` travel as NULL and are left out of the dict."""
        fields = self._wanted(name, table, fields)
        out = {k: (np.zeros((*lead, *shape), dtype=dtype) if k in fields else None) for k, (dtype, shape) in table.items()}
        self._check(self._fn(name)(self._h, *inputs, *[_ptr(out[k]) for k in table]))
        return {k: v for k, v in out.items() if v is not None}

    def _lattice(self, who, origin, spacing, counts):
        o = np.ascontiguousarray(origin, dtype=np.float64).reshape(-1)
        s = np.ascontiguousarray(spacing, dtype=np.float64).reshape(-1)
        c = np.ascontiguousarray(counts, dtype=np.int64).reshape(-1)
        if not (len(o) == len(s) == len(c) == self.D):
            raise ValueError(f"{who}: origin, spacing and counts hold {self.D} entries each")
        return o, s, c

    def _cloud(self, who, positions):
        x = np.ascontiguousarray(positions, dtype=np.float64)
        if x.ndim != 2 or x.shape[1] != self.D:
            raise ValueError(f"{who}: positions is shaped [n, {self.D}]")
        return x

    # A result held on the device (<name>_build / _read / _release).  The reads take no capacities: the arrays are sized from the
    # two counts THIS object's build reported, kept in the attribute named here; the second entry words the refusal.
    _HELD = {"neighbors": ("_neighbor_shape", "a list"), "isosurface": ("_isosurface_shape", "a mesh"),
             "components": ("_components_shape", "components"), "select": ("_select_shape", "a selection")}

    def _held_build(self, name, *args):
        a, b = C.c_int64(), C.c_int64()
        setattr(self, self._HELD[name][0], None)                                  # (a refused build leaves nothing this object may read)
        self._check(self._fn(name + "_build")(self._h, *args, C.byref(a), C.byref(b)))
        setattr(self, self._HELD[name][0], (a.value, b.value))
        return a.value, b.value

    def _held_read(self, name, arrays):
        """`arrays(count, count)` makes the outputs (None skips one).  Without a build of its own the library is asked with every
        pointer NULL — it words the refusal — and a result it then turns out to hold is refused here."""
        f = self._fn(name + "_read")
        attr, what = self._HELD[name]
        shape = getattr(self, attr)
        if shape is None:
            self._check(f(self._h, *[None] * (len(PROTOTYPES[name + "_read"]) - 1)))
            raise RuntimeError(f"{name}_read: the handle holds {what} this object did not build; call {name}_build first")
        out = arrays(*shape)
        self._check(f(self._h, *[_ptr(a) for a in out]))
        return out

    def _held_release(self, name) -> None:
        self._check(self._fn(name + "_release")(self._h))
        setattr(self, self._HELD[name][0], None)

    # -- data movement ----------------------------------------------------------------------
    def _f(self, a, shape):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=self._ft)
        assert a.shape == shape, (a.shape, shape)
        return a

    def upload(self, Position, Velocity, Acceleration, Density, Type, ID, GroupMarker=None,
               GhostPoints=None):
        N, D = self.N, self.D
        keep = [self._f(Position, (N, D)), self._f(Velocity, (N, D)), self._f(Acceleration, (N, D)),
                self._f(Density, (N,)), np.ascontiguousarray(Type, dtype=np.uint8),
                np.ascontiguousarray(ID, dtype=np.int64),
                None if GroupMarker is None else np.ascontiguousarray(GroupMarker, dtype=np.uint64),
                self._f(GhostPoints, (N, D))]
        self._check(self._fn("upload")(self._h, *[_ptr(a) for a in keep]))
        self._column_widths = None         # (sphmi_upload detaches the columns)
        self._force_groups = 0             # (… and disables the group forces)
        self._probes = 0                   # (… and the probes)
        self._moment_probes = 0            # (… and their moments)

    def upload_particles(self, p):
        self.upload(p.Position, p.Velocity, p.Acceleration, p.Density, p.Type, p.ID, p.GroupMarker,
                    p.GhostPoints if self.cfg.mdbc else None)

    def set_motion(self, group_marker: int, motion):
        """MotionDetails of one Geometry (src/SimulationGeometry.jl:17-22) → ProgressMotion of that group."""
        d = np.zeros(3)
        d[:self.D] = np.asarray(motion.Direction, dtype=np.float64)[:self.D]
        self._check(self._fn("set_motion")(self._h, int(group_marker), float(motion.Velocity), float(motion.StartTime),
                                            float(motion.Duration), d.ctypes.data_as(C.c_void_p)))

    def set_motions(self, geometries):
        """Register the Motion of every Geometry that has one (RunSimulation's MotionDefinition dict, :846-850)."""
        for g in geometries or ():
            if getattr(g, "Motion", None) is not None:
                self.set_motion(g.GroupMarker, g.Motion)

    def set_clock(self, iteration: int, total_time: float):
        self._check(self._fn("set_clock")(self._h, iteration, total_time))

    def advance(self, t_target: float, max_steps: int = -1) -> SphmiProgress:
        prog = SphmiProgress()
        self._check(self._fn("advance")(self._h, t_target, max_steps, C.byref(prog)))
        return prog

    def download(self, fields=DOWNLOAD_NAMES, components: Optional[int] = None) -> dict:
        """`components=3`: vector fields as n×3 (2-D vectors padded with a zero — the VTKHDF point layout the reference
        produces with to_3d!, src/ProduceHDFVTK.jl:251-325), packed that way on the device."""
        N, D = self.N, self.D
        Cv = D if components is None else int(components)
        native = Cv != D and self._has("set_output_components")
        Cd = Cv if native else D
        out = {k: (np.empty((N, Cd if dtype is None else D) if vector else (N,), dtype=dtype or self._ft) if k in fields else None)
               for k, dtype, vector in DOWNLOAD_FIELDS}
        if native:
            self._check(self._fn("set_output_components")(self._h, Cv))
        try:
            self._check(self._fn("download")(self._h, *[_ptr(a) for a in out.values()]))
        finally:
            if native:
                self._check(self._fn("set_output_components")(self._h, D))
        if Cv != D and not native:          # backends without the entry point (the oracle): pad on the host
            if Cv != 3:
                raise ValueError("components must be dims or 3")
            for k, dtype, vector in DOWNLOAD_FIELDS:
                if vector and dtype is None and out[k] is not None:
                    out[k] = np.concatenate([out[k], np.zeros((N, 3 - D), dtype=out[k].dtype)], axis=1)
        return {k: v for k, v in out.items() if v is not None}

    def download_into(self, p, begin_only: bool = False) -> None:
        """Write the engine state back into the arrays of a SimParticles IN PLACE (what the reference's loop leaves in
        its StructArray).  Call pin(p) once when the same arrays receive every output."""
        args = [getattr(p, k, None) for k in DOWNLOAD_NAMES]
        # a field absent or in another layout: fall back to the copying path below
        if all(isinstance(a, np.ndarray) and a.dtype == (dtype or self._ft) and a.flags.c_contiguous and len(a) == self.N
               for a, (_, dtype, _) in zip(args, DOWNLOAD_FIELDS)):
            name = "download_begin" if begin_only and self._has("download_begin") else "download"
            self._check(self._fn(name)(self._h, *[_ptr(a) for a in args]))
            return
        for k, v in self.download().items():
            setattr(p, k, v)

    def download_into_begin(self, p) -> None:
        """Start an asynchronous download_into: the arrays of `p` must not be touched until download_end()."""
        self.download_into(p, begin_only=True)

    def download_end(self) -> None:
        if self._has("download_end"):
            self._check(self._fn("download_end")(self._h))

    def pin(self, p) -> None:
        """Page-lock the field arrays of a SimParticles that will receive every output (engine backend only).  The
        arrays must stay alive until unpin() / close()."""
        if not self._has("host_register"):
            return
        if isinstance(p, np.ndarray) or isinstance(p, (list, tuple)):        # arbitrary arrays: the targets of download_columns
            arrays = [p] if isinstance(p, np.ndarray) else list(p)
        else:
            arrays = [getattr(p, k, None) for k in DOWNLOAD_NAMES]
        for a in arrays:
            if isinstance(a, np.ndarray) and a.flags.c_contiguous and a.nbytes and not any(a is b for b in self._pinned):
                self._check(self._fn("host_register")(self._h, _ptr(a), a.nbytes))
                self._pinned = (*self._pinned, a)

    def unpin(self) -> None:
        if not self._has("host_unregister"):
            return
        for a in self._pinned:
            self._fn("host_unregister")(self._h, _ptr(a))
        self._pinned = ()

    def kernel_output(self):
        """(Kernel, KernelGradient) of StoreKernelOutput runs, current order."""
        k = np.empty(self.N, dtype=self._ft)
        g = np.empty((self.N, self.D), dtype=self._ft)
        self._check(self._fn("download_kernel_output")(self._h, _ptr(k), _ptr(g)))
        return k, g

    def download_permutation(self) -> np.ndarray:
        """prev_row: row i of what download() returns now was row prev_row[i] at the previous call (at the upload for the
        first).  The reference's sort! permutes all 17 fields of the StructArray (src/SPHCellList.jl:142); this is what lets
        the caller bring along the fields the engine does not carry (`permute_passive_fields`)."""
        out = np.empty(self.N, dtype=np.int64)
        self._check(self._fn("download_permutation")(self._h, _ptr(out)))
        return out

    # -- the caller's passive columns on the device (sphmi_attach_columns / sphmi_download_columns*) --------------------
    def _column_table(self, arrays, what):
        arrays = list(arrays)
        for a in arrays:
            if a is None:
                continue
            if not (isinstance(a, np.ndarray) and a.flags.c_contiguous and len(a) == self.N and a.nbytes % self.N == 0):
                raise ValueError(f"{what}: every column is a C-contiguous array of {self.N} rows")
        return arrays, (C.c_void_p * max(len(arrays), 1))(*[None if a is None else a.ctypes.data for a in arrays])

    def attach_columns(self, arrays) -> None:
        """Hand the engine columns it does not carry: C-contiguous arrays of N rows in the order download() delivers NOW
        (`row_bytes = a.nbytes // N`, opaque).  The data are copied; every download_columns delivers them in the then
        current cell-sorted order.  An empty sequence detaches."""
        arrays, table = self._column_table(arrays, "attach_columns")
        if any(a is None for a in arrays):
            raise ValueError("attach_columns: a column is None")
        widths = (C.c_int32 * max(len(arrays), 1))(*[a.nbytes // self.N for a in arrays])
        self._check(self._fn("attach_columns")(self._h, len(arrays), table, widths))
        self._column_widths = [a.nbytes // self.N for a in arrays]

    def _download_columns(self, name, outs) -> None:
        outs, table = self._column_table(outs, name)
        widths = self._column_widths
        if widths is not None and (len(outs) != len(widths) or any(a is not None and a.nbytes // self.N != w for a, w in zip(outs, widths))):
            raise ValueError(f"{name}: the arrays do not match the attached columns")
        self._check(self._fn(name)(self._h, table))

    def download_columns(self, outs) -> None:
        """Write the attached columns IN PLACE into `outs` (one array per attached column, None skips one)."""
        self._download_columns("download_columns", outs)

    def download_columns_begin(self, outs) -> None:
        """Asynchronous download_columns — on its own or directly after download_into_begin: `outs` must not be touched
        until download_end(), which completes both."""
        self._download_columns("download_columns_begin", outs)

    # -- the per-step force on particle groups (sphmi_group_forces_enable / sphmi_group_forces_read) ---------------------
    GROUP_FORCE_FIELDS = (("force", (3,), np.float64),)

    def group_forces_enable(self, markers, capacity: int = 4096) -> None:
        """Record F_g = m0 * sum(Acceleration[GroupMarker == g]) of every executed step on the device, for the listed
        GroupMarkers (at most 16, distinct); the newest `capacity` unread samples are kept.  An empty list disables."""
        m = np.ascontiguousarray(list(markers), dtype=np.uint64)
        self._check(self._fn("group_forces_enable")(self._h, len(m), _ptr(m) if len(m) else None, int(capacity)))
        self._force_groups = len(m)

    def group_forces_read(self):
        """(iteration[n], time[n], dt[n], F[n, groups, 3]) of the steps executed since the last read, oldest first, and clears
        them; `group_forces_dropped` holds how many older samples the capacity pushed out."""
        return tuple(self._read_series("group_forces", self.GROUP_FORCE_FIELDS, int(self._force_groups)).values())

    # -- kernel sums at fixed probe points (sphmi_probes_enable / sphmi_probes_read) ---------------------------------------
    PROBE_FIELDS = (("weight", (), np.float64), ("count", (), np.int64), ("pressure", (), np.float64), ("density", (), np.float64),
                    ("velocity", (3,), np.float64))

    def probes_enable(self, positions, capacity: int = 4096) -> None:
        """Sample S = sum w_j, and the w-weighted means of Pressure, Density and Velocity over the Fluid rows within H, at the
        fixed points `positions` [n, dims] (at most 1024) after every executed step, on the device; the newest `capacity`
        unread samples are kept.  An empty array disables."""
        x = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1, self.D)
        self._check(self._fn("probes_enable")(self._h, len(x), _ptr(x) if len(x) else None, int(capacity)))
        self._probes = len(x)

    def probes_read(self) -> dict:
        """The steps executed since the last read, oldest first, and clears them: a dict of iteration[n], time[n], dt[n],
        weight[n, probes] (S), count[n, probes], pressure[n, probes], density[n, probes], velocity[n, probes, 3];
        `probes_dropped` holds how many older samples the capacity pushed out."""
        return self._read_series("probes", self.PROBE_FIELDS, int(self._probes))

    # -- moment sums at fixed probe points (sphmi_probe_moments_enable / sphmi_probe_moments_read) ---------------------------
    def probe_moments_enable(self, positions, capacity: int = 4096) -> None:
        """Record the RAW kernel sums and their moments of `sample_point_moments` at the fixed points `positions` [n, dims] (at most
        1024) after every executed step, on the device; the newest `capacity` unread samples are kept.  An observer of its own:
        its point set is independent of `probes_enable`, and both may be on together.  An empty array disables."""
        x = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1, self.D)
        self._check(self._fn("probe_moments_enable")(self._h, len(x), _ptr(x) if len(x) else None, int(capacity)))
        self._moment_probes = len(x)

    def probe_moments_read(self) -> dict:
        """The steps executed since the last read, oldest first, and clears them: a dict of iteration[n], time[n], dt[n] and the ten
        arrays of `sample_point_moments` under its key names with a leading steps axis — `weight`, `count`, `sum_pressure`,
        `sum_density` [n, probes], `sum_velocity`, `moment1`, `moment_pressure`, `moment_density` [n, probes, 3], `moment2`
        (symmetric) and `moment_velocity` [n, probes, 3, 3] — RAW, plus the handle's `h` and `dims`:
        ``sphexample_amd.probes.fit_series`` turns the record into fitted values and gradients per step and probe.
        `probe_moments_dropped` (also in the dict) holds how many older samples the capacity pushed out."""
        schema = tuple((key, shape, dtype) for key, (dtype, shape) in self.MOMENT_FIELDS.items())
        out = self._read_series("probe_moments", schema, int(self._moment_probes))
        out["moment2"] = np.ascontiguousarray(out["moment2"][:, :, self._SYMMETRIC])
        out["h"], out["dims"] = float(self.cfg.h), int(self.D)
        out["probe_moments_dropped"] = int(self.probe_moments_dropped)
        return out

    # -- the budgets of the fluid at every step (sphmi_budgets_enable / sphmi_budgets_read) ---------------------------------
    BUDGET_FIELDS = (("count", (), np.int64), ("energy", (3,), np.float64), ("momentum", (3,), np.float64), ("angular", (3,), np.float64),
                     ("centre", (3,), np.float64), ("extremes", (3,), np.float64), ("box", (6,), np.float64))

    def budgets_enable(self, capacity: int = 4096) -> None:
        """Record the energy, momentum and extent budgets of the Fluid rows after every executed step, on the device; the newest
        `capacity` unread samples are kept.  `capacity = 0` disables."""
        self._check(self._fn("budgets_enable")(self._h, int(capacity)))

    def budgets_read(self) -> dict:
        """The steps executed since the last read, oldest first, and clears them: a dict of iteration[n], time[n], dt[n], count[n]
        (Fluid rows), energy[n, 3] (kinetic, potential, compressive), momentum[n, 3], angular[n, 3] (about the origin), centre[n, 3]
        (of mass), extremes[n, 3] (largest speed, smallest and largest density) and box[n, 6] (min x, max x);
        `budgets_dropped` holds how many older samples the capacity pushed out."""
        return self._read_series("budgets", self.BUDGET_FIELDS)

    # -- the flow through control boxes at every step (sphmi_flow_enable / sphmi_flow_read) ----------------------------------
    FLOW_FIELDS = (("count", (), np.int64), ("volume", (), np.float64), ("momentum", (3,), np.float64), ("entered", (), np.int64),
                   ("left", (), np.int64))

    def flow_enable(self, lo, hi, capacity: int = 4096) -> None:
        """Record, after every executed step and on the device, how many Fluid rows lie in each of the half-open boxes
        ``lo[b] <= x < hi[b]`` (`lo`, `hi` [n, dims], at most 16, -inf / +inf allowed), their volume and momentum, and how many
        entered and left during that step; the newest `capacity` unread samples are kept.  Empty arrays disable."""
        a = np.ascontiguousarray(lo, dtype=np.float64).reshape(-1, self.D)
        b = np.ascontiguousarray(hi, dtype=np.float64).reshape(-1, self.D)
        if a.shape != b.shape:
            raise ValueError("flow_enable: lo and hi hold one row of `dims` bounds per box each")
        self._check(self._fn("flow_enable")(self._h, len(a), _ptr(a) if len(a) else None, _ptr(b) if len(b) else None, int(capacity)))
        self._flow_boxes = len(a)

    def flow_read(self) -> dict:
        """The steps executed since the last read, oldest first, and clears them: a dict of iteration[n], time[n], dt[n],
        count[n, boxes] (Fluid rows inside after the step), volume[n, boxes] (m0 * sum 1/rho), momentum[n, boxes, 3],
        entered[n, boxes] and left[n, boxes] (rows that crossed into / out of the box during the step);
        `flow_dropped` holds how many older samples the capacity pushed out."""
        return self._read_series("flow", self.FLOW_FIELDS, int(self._flow_boxes))

    # -- per-particle pressure and speed envelopes at every step (sphmi_envelopes_enable / sphmi_envelopes_read) ---------------
    ENVELOPE_FIELDS = ("p_max", "t_p_max", "p_min", "impulse", "square", "loaded", "speed_max", "t_arrival")

    def envelopes_enable(self, types=("Fluid",)) -> None:
        """Accumulate, after every executed step and on the device, what each row of `types` ("Fluid", "Fixed", "Moving", or their
        Type numbers) experiences: the largest and smallest pressure, when the largest occurred, the pressure impulse, the time
        under load, the largest speed and the arrival time of the first positive pressure.  The records follow the particle
        through every sort.  A second call replaces the selection and restarts the window; an empty `types` disables."""
        self._check(self._fn("envelopes_enable")(self._h, self._type_mask(types)))

    def envelopes_read(self) -> dict:
        """The envelopes as they stand, without clearing them: `steps` (executed steps since the enable), `t_begin`, `t_end`,
        `duration` (sum of dt) and float64 [n] arrays `p_max`, `t_p_max`, `p_min`, `impulse` (sum P dt), `square` (sum P^2 dt),
        `loaded` (sum dt over steps with P > 0), `speed_max` and `t_arrival` (+inf: never loaded); row i is row i of what `download`
        delivers now.  Rows of a type that is not selected hold the start record (-inf, 0, +inf, 0, 0, 0, 0, +inf)."""
        return self._read_window("envelopes", {name: np.zeros(self.N) for name in self.ENVELOPE_FIELDS})

    # -- per-bin maps of crest, arrival and mean flow at every step (sphmi_maps_enable / _read / _disable) ----------------------
    MAP_FIELDS = ("top_max", "t_top_max", "bottom_min", "t_arrival", "wet", "fill", "flux", "speed2_max", "t_speed2_max", "n_max")
    MAP_LAST = ("last_n", "last_top", "last_bottom", "last_velocity_sum")

    def maps_enable(self, origin, spacing, counts, up_axis: int = None) -> None:
        """Accumulate, after every executed step and on the device, what every bin of a lattice experiences: bin (k0, k1[, k2]) holds
        the Fluid rows with ``k = floor((x - origin) / spacing)``, ``0 <= k < counts`` per axis; ``counts[d] = 1`` with
        ``spacing[d] = inf`` collapses axis d (a column map over the floor of a 3-D tank: ``counts = (nx, ny, 1)``).  `up_axis`
        (default: the last axis) names the coordinate whose extremes are kept.  A second call restarts the records."""
        o, s, c = self._lattice("maps_enable", origin, spacing, counts)
        self._check(self._fn("maps_enable")(self._h, _ptr(o), _ptr(s), _ptr(c), self.D - 1 if up_axis is None else int(up_axis)))
        self._map_bins = int(np.prod(c))

    def maps_disable(self) -> None:
        """Stop accumulating and free the device memory of the maps."""
        self._check(self._fn("maps_disable")(self._h))
        self._map_bins = 0

    def maps_read(self) -> dict:
        """The maps as they stand, without clearing them: `steps`, `t_begin`, `t_end`, `duration` and float64 arrays over the bins
        (bin ``k0 + counts[0] * (k1 + counts[1] * k2)``): `top_max`, `t_top_max`, `bottom_min`, `t_arrival` (+inf: never wet), `wet`,
        `fill`, `flux` [bins, 3], `speed2_max` (the square; `sphexample_amd.maps.max_speed` takes the root), `t_speed2_max`, `n_max`;
        then the map of the last executed step: `last_n` (int64), `last_top`, `last_bottom`, `last_velocity_sum` [bins, 3]."""
        B = int(self._map_bins)
        shape = lambda k: (B, 3) if k in ("flux", "last_velocity_sum") else (B,)       # noqa: E731
        return self._read_window("maps", {k: np.zeros(shape(k), dtype=np.int64 if k == "last_n" else np.float64)
                                          for k in self.MAP_FIELDS + self.MAP_LAST})

    # -- tracers: tracked particles and advected drifters at every step (sphmi_tracers_enable / sphmi_tracers_read) -------------
    TRACER_PARTICLE_VALUES, TRACER_DRIFTER_VALUES = 8, 10

    def tracers_enable(self, particles=None, drifters=None, min_weight: float = 0.5, capacity: int = 4096) -> None:
        """Follow, after every executed step and on the device, the rows `particles` (at most 1024 row numbers of what `download`
        delivers NOW; they follow the particle through every sort) and advect the massless points `drifters` [m, dims] (at most
        1024) with the Shepard-mean velocity of the fluid around them: ``X += (Sv / S) * dt`` where ``S >= min_weight``, else the
        drifter is dry and stays.  The newest `capacity` unread samples are kept; the drifters move whether or not they are read.
        A second call replaces both sets and restarts the drifters; neither set disables."""
        rows = np.ascontiguousarray([] if particles is None else particles, dtype=np.int64).reshape(-1)
        x = np.ascontiguousarray(np.zeros((0, self.D)) if drifters is None else drifters, dtype=np.float64).reshape(-1, self.D)
        self._check(self._fn("tracers_enable")(self._h, len(rows), _ptr(rows) if len(rows) else None, len(x), _ptr(x) if len(x) else None,
                                               float(min_weight), int(capacity)))
        self._tracers = (len(rows), len(x), float(min_weight))

    def tracers_read(self) -> dict:
        """The steps executed since the last read, oldest first, and clears them: iteration[K], time[K], dt[K];
        ``particles``: ``values`` [K, n, 8] and its views ``position`` [K, n, 3], ``velocity`` [K, n, 3], ``density`` [K, n],
        ``pressure`` [K, n] - what `download` would have delivered for those particles after each step;
        ``drifters``: ``position`` [K, m, 3] (where the sums of that step were taken, BEFORE its move), ``sums`` [K, m, 7] (raw S, SP,
        Srho, Sv[3], n) and, normalised as `probes_read` does, ``weight``, ``count``, ``pressure``, ``density``, ``velocity``;
        ``drifter_position`` [m, 3]: where the drifters are NOW; ``min_weight``; ``dropped``: older samples the capacity pushed out."""
        np_, nd, min_weight = self._tracers
        x = np.zeros((nd, 3))
        got = self._read_series("tracers", (("particles", (np_, self.TRACER_PARTICLE_VALUES), np.float64),
                                            ("drifters", (nd, self.TRACER_DRIFTER_VALUES), np.float64)), tail=(x,))
        pv, dv = got["particles"], got["drifters"]
        sums = dv[:, :, 3:]
        S, cnt = sums[:, :, 0], sums[:, :, 6]
        some = (cnt > 0) & (S > 0)
        safe = np.where(some, S, 1.0)
        mean = lambda a: np.where(some if a.ndim == 2 else some[:, :, None], a / (safe if a.ndim == 2 else safe[:, :, None]), 0.0)    # noqa: E731
        return {"iteration": got["iteration"], "time": got["time"], "dt": got["dt"],
                "particles": {"values": pv, "position": pv[:, :, 0:3], "velocity": pv[:, :, 3:6], "density": pv[:, :, 6], "pressure": pv[:, :, 7]},
                "drifters": {"position": dv[:, :, 0:3], "sums": sums, "weight": S, "count": cnt.astype(np.int64), "pressure": mean(sums[:, :, 1]),
                             "density": mean(sums[:, :, 2]), "velocity": mean(sums[:, :, 3:6])},
                "drifter_position": x, "min_weight": min_weight, "dropped": int(self.tracers_dropped)}

    # -- kernel sums on a regular lattice, on demand (sphmi_sample_grid) -----------------------------------------------------
    # the selectable outputs: name → (dtype, trailing shape), in the order of the C prototype
    _GRID = {"weight": (_F64, ()), "count": (_INT64, ()), "pressure": (_F64, ()), "density": (_F64, ()), "velocity": (_F64, (3,))}
    GRID_FIELDS = tuple(_GRID)

    def sample_grid(self, origin, spacing, counts, fields=None) -> dict:
        """The probes' sums at every node of a regular lattice, evaluated now: node (i, j, k) lies at
        ``origin + (i, j, k) * spacing`` (`sphexample_amd.fields.grid_nodes` forms the same doubles), `counts` = (nx, ny[, nz])
        nodes per axis, at most 2**24 in all.  Returns a dict of `weight` (S), `count`, `pressure`, `density`, each shaped
        ``counts[::-1]`` — x fastest, the order of VTK image data — and `velocity` shaped ``counts[::-1] + (3,)``; `fields`
        names the ones wanted (default: all).  Call it between `advance` calls, after the first executed step."""
        o, s, c = self._lattice("sample_grid", origin, spacing, counts)
        fields = self._wanted("sample_grid", self._GRID, fields)
        if (c < 1).any() or int(np.prod(c, dtype=object)) > MAX_GRID_NODES:
            self._sample("sample_grid", self._GRID, (), (), _ptr(o), _ptr(s), _ptr(c))     # the library words the refusal (state errors come first)
            raise ValueError("sample_grid: counts out of range")
        return self._sample("sample_grid", self._GRID, fields, tuple(int(v) for v in c[::-1]), _ptr(o), _ptr(s), _ptr(c))

    # -- kernel sums at arbitrary points, on demand (sphmi_sample_points) -----------------------------------------------------
    def sample_points(self, positions, fields=None) -> dict:
        """The sums of `sample_grid` at every point of `positions` ([n, dims]: panel centroids, mesh nodes, a ring of sensors —
        any cloud of up to 2**24 points), evaluated now.  Returns the dict of `sample_grid` with a leading axis of n instead of
        the lattice's: `weight`, `count`, `pressure`, `density` [n] and `velocity` [n, 3], entry p belonging to
        ``positions[p]``; `fields` names the ones wanted (default: all).  A point's result does not depend on the other points
        of the call.  Call it between `advance` calls, after the first executed step."""
        x = self._cloud("sample_points", positions)
        return self._sample("sample_points", self._GRID, fields, (len(x),), len(x), _ptr(x))

    # -- gradient sums at arbitrary points, on demand (sphmi_sample_point_gradients) ---------------------------------------------
    GRADIENT_FIELDS = {"weight": (_F64, ()), "count": (_INT64, ()), "sum_pressure": (_F64, ()), "sum_density": (_F64, ()),
                       "sum_velocity": (_F64, (3,)), "grad_weight": (_F64, (3,)), "grad_pressure": (_F64, (3,)),
                       "grad_density": (_F64, (3,)), "grad_velocity": (_F64, (3, 3))}

    def sample_point_gradients(self, positions, fields=None) -> dict:
        """The RAW kernel sums and gradient sums at every point of `positions` ([n, dims], up to 2**24 points), evaluated now:
        `weight` S, `count` n, `sum_pressure`, `sum_density` [n], `sum_velocity` [n, 3], and with g_j = ∇W(x − x_j):
        `grad_weight` Σ V_j g_j, `grad_pressure`, `grad_density` [n, 3], `grad_velocity` [n, 3, 3] with entry [a, b] =
        Σ V_j v_j[a] g_j[b].  Nothing is divided by S; ``sphexample_amd.fields`` normalises (`velocity_gradient`,
        `vorticity_at`, `divergence_at`, `strain_rate`, `pressure_gradient`, `surface_normal_at`).  `fields` names the sums
        wanted (default: all).  Entry p belongs to ``positions[p]`` and does not depend on the other points of the call;
        multi-device handles of one process deliver the sums over all slabs.  Call it between `advance` calls, after the
        first executed step."""
        x = self._cloud("sample_point_gradients", positions)
        return self._sample("sample_point_gradients", self.GRADIENT_FIELDS, fields, (len(x),), len(x), _ptr(x))

    # -- moment sums at arbitrary points, on demand (sphmi_sample_point_moments) --------------------------------------------------
    # (moment2 travels as the six entries xx, xy, xz, yy, yz, zz and is handed out as the symmetric [n, 3, 3])
    MOMENT_FIELDS = {"weight": (_F64, ()), "count": (_INT64, ()), "sum_pressure": (_F64, ()), "sum_density": (_F64, ()),
                     "sum_velocity": (_F64, (3,)), "moment1": (_F64, (3,)), "moment2": (_F64, (6,)), "moment_pressure": (_F64, (3,)),
                     "moment_density": (_F64, (3,)), "moment_velocity": (_F64, (3, 3))}
    _SYMMETRIC = np.array([[0, 1, 2], [1, 3, 4], [2, 4, 5]])

    def sample_point_moments(self, positions, fields=None) -> dict:
        """The RAW kernel sums and their moments at every point of `positions` ([n, dims], up to 2**24 points), evaluated now, with
        w_j = (m0 / ρ_j) W(r) and e_j = x_j − x: `weight` S, `count` n, `sum_pressure`, `sum_density` [n], `sum_velocity` [n, 3],
        `moment1` Σ w e [n, 3], `moment2` Σ w e ⊗ e [n, 3, 3] (symmetric), `moment_pressure` Σ w P e, `moment_density` Σ w ρ e
        [n, 3] and `moment_velocity` [n, 3, 3] with entry [a, b] = Σ w v[a] e[b].  Nothing is divided by S;
        ``sphexample_amd.fields.linear_fit`` solves the per-point system for the values AT the points and their gradients, exact
        for a linear field however one-sided the support (`vorticity_linear`, `divergence_linear`, `strain_rate_linear`,
        `surface_load_linear` build on it).  `fields` names the sums wanted (default: all); the dict also carries the handle's `h`
        and `dims`, which `linear_fit` scales its system with.  Entry p belongs to ``positions[p]``
        and does not depend on the other points of the call; multi-device handles of one process deliver the sums over all
        slabs.  Call it between `advance` calls, after the first executed step."""
        x = self._cloud("sample_point_moments", positions)
        out = self._sample("sample_point_moments", self.MOMENT_FIELDS, fields, (len(x),), len(x), _ptr(x))
        if "moment2" in out:
            out["moment2"] = np.ascontiguousarray(out["moment2"][:, self._SYMMETRIC])
        out["h"], out["dims"] = float(self.cfg.h), int(self.D)                 # what `fields.linear_fit` scales the system with
        return out

    # -- the first crossing of S = level along rays, on demand (sphmi_cast_rays) ---------------------------------------------------
    RAY_FIELDS = {"status": (np.int32, ()), "interval": (_INT64, ()), "bracket": (_F64, (2,)), "point": (_F64, (3,)),
                  "weight": (_F64, ()), "count": (_INT64, ()), "sum_pressure": (_F64, ()), "sum_density": (_F64, ()),
                  "sum_velocity": (_F64, (3,))}
    RAY_MODES = {"enter": RAY_ENTER, "leave": RAY_LEAVE, "any": RAY_ANY}

    def cast_rays(self, origins, directions, t_end, t_begin=0.0, step=None, level=0.5, mode="enter", fields=None) -> dict:
        """Where along each ray ``origins[r] + t * directions[r]`` ([n, dims]; `t_begin`, `t_end` numbers or [n]; t and `step` in
        units of |direction|) does ``S >= level`` begin (`mode` "enter"), end ("leave") or change ("any"): a march in steps of
        `step` (default h / 2) to the first such interval, then four subdivisions by 64.  A dict: `status` (bit 0 found, bit 1
        the ray starts inside), `interval` (k, or −1), `bracket` [n, 2], `point` [n, 3] (the inside end of the bracket) and the
        raw sums of ``sample_point_gradients`` there: `weight`, `count`, `sum_pressure`, `sum_density` [n], `sum_velocity`
        [n, 3].  NaN brackets and points and zero sums where nothing was hit.  `fields` names the outputs wanted (default: all).
        A ray's result depends on its own arguments and the state alone.  Single-device handles; call it between `advance`
        calls, after the first executed step.  ``sphexample_amd.rays`` builds gauges and depth images on it."""
        o = np.ascontiguousarray(origins, dtype=np.float64)
        d = np.ascontiguousarray(directions, dtype=np.float64)
        if o.ndim != 2 or o.shape[1] != self.D or d.shape != o.shape:
            raise ValueError(f"cast_rays: origins and directions are both shaped [n, {self.D}]")
        n = len(o)
        tb = np.ascontiguousarray(np.broadcast_to(np.asarray(t_begin, dtype=np.float64), (n,)))
        te = np.ascontiguousarray(np.broadcast_to(np.asarray(t_end, dtype=np.float64), (n,)))
        if mode not in self.RAY_MODES:
            raise ValueError(f"cast_rays: mode is one of {sorted(self.RAY_MODES)}")
        fields = self._wanted("cast_rays", self.RAY_FIELDS, fields)
        step = 0.5 * float(self.cfg.h) if step is None else float(step)
        return self._sample("cast_rays", self.RAY_FIELDS, fields, (n,), n, _ptr(o), _ptr(d), _ptr(tb), _ptr(te), step, float(level),
                            self.RAY_MODES[mode])

    # -- differential fields at the particles, on demand (sphmi_particle_fields) ------------------------------------------------
    _PARTICLE = {"count": (_INT64, ()), "shepard": (_F64, ()), "normal": (_F64, (3,)), "div_r": (_F64, ()), "div_v": (_F64, ()),
                 "vorticity": (_F64, (3,))}
    PARTICLE_FIELDS = tuple(_PARTICLE)

    def particle_fields(self, fields=PARTICLE_FIELDS) -> dict:
        """Vorticity, velocity divergence, the free-surface indicator div r, the free-surface normal, the Shepard sum and the
        neighbour count of every row, evaluated now over all rows within H on the current positions: a dict of `count` [n]
        (int64), `shepard`, `div_r`, `div_v` [n] and `normal`, `vorticity` [n, 3] (2-D: only the z component of the vorticity
        and the x, y of the normal are non-zero), row i being row i of what `download` delivers now.  Only the fields named are
        computed into host arrays.  Single-device handles; call it between `advance` calls, after the first executed step."""
        return self._sample("particle_fields", self._PARTICLE, fields, (self.N,))

    # -- the neighbour list of every row, on demand (sphmi_neighbors_build / _read / _release) ----------------------------------
    def neighbors_build(self, half: bool = False):
        """Build the CSR neighbour list of every row on the device and keep it there: (n_rows, n_pairs).  `half`: only j > i,
        every pair once.  It stays until the next build, `neighbors_release` or `close`; a step, an upload or `forces_once`
        marks it stale."""
        return self._held_build("neighbors", NEIGHBORS_HALF if half else NEIGHBORS_FULL)

    def neighbors_read(self, offsets: bool = True, neighbors: bool = True):
        """(offsets int64 [n_rows + 1], neighbors int32 [n_pairs]) of the list built last; False skips one (None in its place).
        sphmi_neighbors_read takes no capacities: the arrays are sized from what THIS object's `neighbors_build` reported, so a
        list built through the raw entry point behind its back must not be read here.  Without a build of its own the library
        is asked with both pointers NULL — it words the refusal — and a list it then turns out to hold is refused here."""
        return self._held_read("neighbors", lambda rows, pairs: (np.zeros(rows + 1, dtype=np.int64) if offsets else None,
                                                                 np.zeros(pairs, dtype=np.int32) if neighbors else None))

    def neighbors_release(self) -> None:
        self._held_release("neighbors")

    def neighbor_list(self, half: bool = False):
        """The neighbour list of every row, evaluated now: (offsets int64 [n + 1], neighbors int32 [total]); row i — row i of what
        `download` delivers now — lists neighbors[offsets[i]:offsets[i + 1]], every row j != i within H on the current positions,
        ascending (`half`: only j > i).  `sphexample_amd.neighbors` forms pair sums from it.  Single-device handles; call it
        between `advance` calls, after the first executed step.  The device memory is given back before it returns."""
        self.neighbors_build(half)
        try:
            return self.neighbors_read()
        finally:
            self.neighbors_release()

    # -- the free surface as a mesh, on demand (sphmi_isosurface_build / _read / _release) ---------------------------------------
    def isosurface_build(self, origin, spacing, counts, level: float = 0.5):
        """Sample the Shepard sum on the lattice of `sample_grid` and extract the surface ``S == level`` on the device, where it
        stays: (n_vertices, n_elements).  It is held until the next build, `isosurface_release` or `close`; a step, an upload or
        `forces_once` marks it stale."""
        o, s, c = self._lattice("isosurface_build", origin, spacing, counts)
        return self._held_build("isosurface", _ptr(o), _ptr(s), _ptr(c), float(level))

    def isosurface_read(self, vertices: bool = True, elements: bool = True, pressure: bool = False, velocity: bool = False):
        """(vertices float64 [nv, 3], elements int32 [ne, D], pressure [nv], velocity [nv, 3]) of the mesh built last; False skips
        one (None in its place).  sphmi_isosurface_read takes no capacities: the arrays are sized from what THIS object's
        `isosurface_build` reported, so a mesh built through the raw entry point behind its back must not be read here."""
        return self._held_read("isosurface", lambda nv, ne: (np.zeros((nv, 3)) if vertices else None,
                                                             np.zeros((ne, self.D), dtype=np.int32) if elements else None,
                                                             np.zeros(nv) if pressure else None, np.zeros((nv, 3)) if velocity else None))

    def isosurface_release(self) -> None:
        self._held_release("isosurface")

    def isosurface(self, origin, spacing, counts, level: float = 0.5, attributes: bool = False):
        """The free surface as a mesh, evaluated now: ``(vertices [nv, 3], elements [ne, D] int32)`` — triangles on 3-D handles,
        the segments of a contour polyline on 2-D handles (a zero third coordinate), normals out of the fluid / the fluid to the
        left — of the surface ``S == level`` of the Shepard sum on the lattice `sample_grid` takes; `attributes` adds the pressure
        [nv] and velocity [nv, 3] interpolated to the vertices.  `sphexample_amd.isosurface` restates the extraction in numpy and
        measures the result.  Single-device handles; call it between `advance` calls, after the first executed step.  The device
        memory is given back before it returns."""
        self.isosurface_build(origin, spacing, counts, level)
        try:
            got = self.isosurface_read(pressure=attributes, velocity=attributes)
            return got if attributes else got[:2]
        finally:
            self.isosurface_release()

    # -- the connected bodies of selected rows, on demand (sphmi_components_build / _read / _release) ----------------------------
    COMPONENT_TYPES = {"Fluid": 1, "Fixed": 2, "Moving": 3}

    def _type_mask(self, types) -> int:
        if isinstance(types, (str, int, np.integer)):
            types = (types,)
        mask = 0
        for t in types:
            if isinstance(t, str) and t not in self.COMPONENT_TYPES:
                raise ValueError(f"components: unknown type {t!r} (one of {sorted(self.COMPONENT_TYPES)})")
            mask |= 1 << (self.COMPONENT_TYPES[t] if isinstance(t, str) else int(t))
        return mask

    def components_build(self, link=None, types=("Fluid",)):
        """Label the connected bodies of the rows of `types` ("Fluid", "Fixed", "Moving", or their Type numbers) on the device and
        keep the result there: (n_rows, n_components).  Two selected rows are linked iff r^2 <= link^2 on the current positions;
        `link=None` means H, the longest the library serves.  It stays until the next build, `components_release` or `close`; a
        step, an upload or `forces_once` marks it stale."""
        return self._held_build("components", float(self.cfg.H if link is None else link), self._type_mask(types))

    def components_read(self, label: bool = True, first_row: bool = True, count: bool = True, box: bool = True):
        """(label int32 [n_rows], first_row int32 [C], count int32 [C], box float64 [C, 6]) of the components built last; False
        skips one (None in its place).  sphmi_components_read takes no capacities: the arrays are sized from what THIS object's
        `components_build` reported, so a result built through the raw entry point behind its back must not be read here."""
        return self._held_read("components", lambda rows, comps: (np.zeros(rows, dtype=np.int32) if label else None,
                                                                  np.zeros(comps, dtype=np.int32) if first_row else None,
                                                                  np.zeros(comps, dtype=np.int32) if count else None,
                                                                  np.zeros((comps, 6)) if box else None))

    def components_release(self) -> None:
        self._held_release("components")

    def components(self, link=None, types=("Fluid",)) -> dict:
        """The connected bodies of the rows of `types`, evaluated now: a dict of `label` int32 [n] (the component of row i — row i of
        what `download` delivers now — or -1 if it is not selected), `first_row`, `count` int32 [C] and `box` float64 [C, 6]
        (min x, y, z, max x, y, z); components are numbered in ascending first (smallest) row.  `sphexample_amd.components` finds
        the main body, tabulates the droplets and restates the labelling in numpy.  Single-device handles; call it between
        `advance` calls, after the first executed step.  The device memory is given back before it returns."""
        self.components_build(link, types)
        try:
            return dict(zip(("label", "first_row", "count", "box"), self.components_read()))
        finally:
            self.components_release()

    # -- a selected subset of the rows, compacted on the device (sphmi_select_build / _read / _download* / _release) -----------------
    def select_build(self, spec):
        """Flag, scan and list the rows `spec` (a ``sphexample_amd.selection.Selection``) selects, on the device, and keep the list
        there: (n_rows, n_selected).  It needs an upload and nothing more.  It stays until the next build, `select_release` or
        `close`; a step, an upload or `forces_once` marks it stale."""
        lo, hi = spec.box_tables(self.D)
        markers = np.ascontiguousarray(list(spec.markers), dtype=np.uint64)
        mask = spec.mask_bytes(self.N)
        sel = SphmiSelection(spec.type_mask(), len(lo), lo.ctypes.data if len(lo) else None, hi.ctypes.data if len(hi) else None,
                             len(markers), markers.ctypes.data if len(markers) else None, int(spec.id_stride), int(spec.id_phase),
                             spec.field_code(), float(spec.field_lo), float(spec.field_hi), None if mask is None else mask.ctypes.data)
        return self._held_build("select", C.byref(sel))                           # (lo, hi, markers, mask live until the call returns)

    def select_read(self) -> np.ndarray:
        """The selected rows, int32 ascending: row numbers of what `download` delivers now."""
        return self._held_read("select", lambda rows, kept: (np.zeros(kept, dtype=np.int32),))[0]

    def _select_shape_or_refusal(self, name):
        if self._select_shape is None:                                             # the library words the refusal
            self._check(self._fn(name)(self._h, *[None] * (len(PROTOTYPES[name]) - 1)))
            raise RuntimeError(f"{name}: the handle holds a selection this object did not build; call select_build first")
        return self._select_shape

    def select_download(self, fields=DOWNLOAD_NAMES, components: Optional[int] = None) -> dict:
        """`download` for the selected rows only: every array holds n_selected rows, slot s being row ``select_read()[s]``, and equals
        ``download(fields, components)[name][rows]`` byte for byte."""
        _, kept = self._select_shape_or_refusal("select_download")
        D = self.D
        Cv = D if components is None else int(components)
        if Cv not in (D, 3):
            raise ValueError("components must be dims or 3")
        out = {k: (np.empty((kept, Cv if dtype is None else D) if vector else (kept,), dtype=dtype or self._ft) if k in fields else None)
               for k, dtype, vector in DOWNLOAD_FIELDS}
        if Cv != D:
            self._check(self._fn("set_output_components")(self._h, Cv))
        try:
            self._check(self._fn("select_download")(self._h, *[_ptr(a) for a in out.values()]))
        finally:
            if Cv != D:
                self._check(self._fn("set_output_components")(self._h, D))
        return {k: v for k, v in out.items() if v is not None}

    def select_download_columns(self, which=None) -> list:
        """The attached columns of the selected rows: one uint8 array [n_selected, row_bytes] per attached column, opaque bytes as
        `attach_columns` took them (``.view(dtype)`` restores the type); `which`: one bool per column, False skips it (None in its
        place)."""
        _, kept = self._select_shape_or_refusal("select_download_columns")
        widths = self._column_widths
        if widths is None:
            self._check(self._fn("select_download_columns")(self._h, (C.c_void_p * 1)(None)))      # (nothing attached: the library words the refusal)
            raise RuntimeError("select_download_columns: this object attached no columns")
        which = [True] * len(widths) if which is None else [bool(w) for w in which]
        if len(which) != len(widths):
            raise ValueError("select_download_columns: one entry per attached column")
        outs = [np.zeros((kept, w), dtype=np.uint8) if on else None for w, on in zip(widths, which)]
        table = (C.c_void_p * max(len(outs), 1))(*[None if a is None else a.ctypes.data for a in outs])
        self._check(self._fn("select_download_columns")(self._h, table))
        return outs

    def select_release(self) -> None:
        self._held_release("select")

    def select(self, spec, fields=DOWNLOAD_NAMES, columns: bool = False, components: Optional[int] = None):
        """The rows `spec` selects and their fields, evaluated now: ``(rows, dict of arrays)``, or ``(rows, dict, columns)`` with
        `columns` — rows int32 ascending, every array ``download()[name][rows]`` byte for byte, only the selected rows crossing the
        bus.  ``sphexample_amd.selection`` builds selections (`slab`, `every`, `where`) and restates the rule in numpy.
        Single-device handles; call it between `advance` calls, any time after the upload.  The device memory is given back
        before it returns."""
        self.select_build(spec)
        try:
            got = (self.select_read(), self.select_download(fields, components))
            return (*got, self.select_download_columns()) if columns else got
        finally:
            self.select_release()

    def forces_once(self, apply_mdbc: bool = False):
        drho = np.empty(self.N, dtype=self._ft)
        acc = np.empty((self.N, self.D), dtype=self._ft)
        self._check(self._fn("forces_once")(self._h, int(apply_mdbc), _ptr(drho), _ptr(acc)))
        return drho, acc

    def unique_cells(self) -> np.ndarray:
        n = C.c_int64()
        self._check(self._fn("unique_cells")(self._h, None, 0, C.byref(n)))
        out = np.empty((n.value, self.D), dtype=np.int64)
        self._check(self._fn("unique_cells")(self._h, _ptr(out), n.value, C.byref(n)))
        return out


for _feature, _symbols in FEATURES.items():       # has_columns(), has_group_forces(), … has_components()
    setattr(Backend, "has_" + _feature, lambda self, _symbols=_symbols: self._has_all(_symbols))
