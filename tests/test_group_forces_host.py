"""CPU-side checks of the group-force entry points (sphmi_group_forces_enable / sphmi_group_forces_read): declared with the arity the
bindings use, exported, wrapped, bound by the Julia shim behind its opt-in; the ABI version stays 5; the kernels live in a header of
their own, hold no floating-point atomic and the two bench kernels did not move; RunSimulation's default keeps the callback's shape."""
import copy
import inspect
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"sphmi_group_forces_enable": 4, "sphmi_group_forces_read": 8}


def test_the_entry_points_are_declared_and_exported():
    from test_julia_shim import c_prototypes
    from sphexample_amd.engine import load_library
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sphmi.h")).read(), flags=re.S)
    protos = c_prototypes()
    lib = load_library()
    for s, arity in SYMBOLS.items():
        assert s in protos, f"{s} is not declared in include/sphmi.h"
        assert protos[s][0] == "int" and len(protos[s][1]) == arity, protos[s]
        assert hasattr(lib, s), f"libsphmi.so does not export {s}"
    assert re.search(r"#define\s+SPHMI_MAX_FORCE_GROUPS\s+16\b", text)
    assert re.search(r"#define\s+SPHMI_ABI_VERSION\s+5\b", text)


def test_the_ctypes_wrappers_bind_them_with_the_header_arity(monkeypatch):
    """The wrappers are run against a recording stand-in for the library: the argtypes they declare and the arguments they pass have
    the header's arity, and the two-call read (how many wait, then the samples) delivers arrays of the documented shapes."""
    from sphexample_amd import _abi
    assert (_abi.MAX_FORCE_GROUPS, _abi.ABI_VERSION) == (16, 5)
    for name in ("group_forces_enable", "group_forces_read", "has_group_forces"):
        assert callable(getattr(_abi.Backend, name))
    seen = []

    class Fn:
        def __init__(self, name):
            self.name, self.argtypes = name, None

        def __call__(self, *args):
            seen.append((self.name, len(self.argtypes), len(args)))
            if self.name == "x_group_forces_read":
                args[6]._obj.value = 3                             # three samples wait, then are delivered
                args[7]._obj.value = 2
            return 0

    class Lib:
        def __init__(self):
            self.fns = {n: Fn(n) for n in ("x_group_forces_enable", "x_group_forces_read")}

        def __getattr__(self, n):
            try:
                return self.__dict__["fns"][n]
            except KeyError:
                raise AttributeError(n)

    b = _abi.Backend.__new__(_abi.Backend)
    b._lib, b._p, b._h = Lib(), "x_", None
    assert b.has_group_forces()
    b.group_forces_enable([1, 2], capacity=7)
    it, t, dt, F = b.group_forces_read()
    assert seen == [("x_group_forces_enable", 4, 4), ("x_group_forces_read", 8, 8), ("x_group_forces_read", 8, 8)]
    assert it.dtype == np.int64 and it.shape == t.shape == dt.shape == (3,) and F.shape == (3, 2, 3) and F.dtype == np.float64
    assert b.group_forces_dropped == 2


def test_the_julia_shim_binds_the_calls_behind_an_opt_in():
    from test_julia_shim import shim_ccalls
    called = [c[0] for c in shim_ccalls()]
    assert called.count("sphmi_group_forces_enable") == 1 and called.count("sphmi_group_forces_read") == 2
    shim = open(os.path.join(ROOT, "julia", "SPHExampleMI355X.jl")).read()
    assert 'ENV, "SPHMI_GROUP_FORCES", ""' in shim            # unset: no marker, no enable, no read


def test_run_simulation_default_keeps_the_callback(dam_break_2d):
    """group_forces=None: the oracle-backed driver (which has no such entry points) runs as before and calls back with two arguments."""
    from oracle.oracle import Oracle
    from sphexample_amd import simulation
    assert inspect.signature(simulation.RunSimulation).parameters["group_forces"].default is None
    p, s = dam_break_2d
    meta = copy.deepcopy(s.SimMetaData)
    meta.SimulationTime, meta.OutputTimes = 0.0004, 0.0002
    shapes = []
    simulation.RunSimulation(SimGeometry=None, SimMetaData=meta, SimConstants=s.SimConstants, SimKernel=s.SimKernel, SimLogger=None,
                             SimParticles=p.copy(), SimViscosity=s.SimViscosity, SimDensityDiffusion=s.SimDensityDiffusion, backend_factory=Oracle,
                             on_output=lambda *a: shapes.append(len(a)))
    assert len(shapes) >= 2 and set(shapes) == {2}


def test_sampling_kernels_isa_and_the_bench_kernels(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench
    import isa_report
    from sphexample_amd import build
    lib = build.build()
    co = isa_report.code_object(lib, str(tmp_path))
    meta, isa = isa_report.metadata(co), isa_report.kernels(co)
    names = isa_report.demangle(list(meta))
    for kernel, copies in (("k_gf_count", 1), ("k_gf_offsets", 1), ("k_gf_fill", 1), ("k_gf_final", 1), ("k_gf_partial", 2), ("k_gf_small", 2)):
        mine = [k for k, d in names.items() if re.search(r"\b%s\b" % kernel, d)]
        assert len(mine) == copies, (kernel, mine)
        for k in mine:
            assert meta[k]["scratch_bytes"] == 0, kernel
            # a fixed summation order: no floating-point atomic anywhere in the feature's kernels
            assert not [ln for ln in isa[k] if re.search(r"atomic_(add|pk_add|min|max)_f(16|32|64)", ln)], kernel
    record = json.load(open(os.path.join(ROOT, bench.COUNTER_RECORD)))
    ident = bench.loaded_kernel_identity()
    assert "error" not in ident, ident
    for which in ("predictor", "corrector"):
        assert ident[which]["isa_sha16"] == record["kernels"][which]["isa_sha16"], which
