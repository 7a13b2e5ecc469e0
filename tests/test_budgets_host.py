"""CPU-side checks of the budgets of the fluid (sphmi_budgets_enable / sphmi_budgets_read): the two prototypes are declared with the
arity the bindings use, exported, wrapped, bound by the Julia shim behind its opt-in; the ABI version stays 5; the kernels live in a
header of their own, hold no floating-point atomic and do not spill; the host side (deliver_budgets, the slab combine) runs on
hand-made records under the address and undefined-behaviour sanitizers (tests/host_series/budgets_main.cpp); the helpers of
sphexample_amd.budgets; RunSimulation's default keeps the callback's shape."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np

from test_step_series_host import CSRC, SANITIZE, host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "host_series", "budgets_main.cpp")
SYMBOLS = {"sphmi_budgets_enable": 2, "sphmi_budgets_read": 14}


def test_the_entry_points_are_declared_and_exported():
    from test_julia_shim import c_class, c_prototypes
    from sphexample_amd.engine import load_library
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sphmi.h")).read(), flags=re.S)
    protos = c_prototypes()
    lib = load_library()
    for s, arity in SYMBOLS.items():
        assert s in protos, f"{s} is not declared in include/sphmi.h"
        assert protos[s][0] == "int" and len(protos[s][1]) == arity, protos[s]
        assert hasattr(lib, s), f"libsphmi.so does not export {s}"
    assert [c_class(a) for a in protos["sphmi_budgets_enable"][1]] == ["ptr", "i8"]
    assert [c_class(a) for a in protos["sphmi_budgets_read"][1]] == ["ptr", "i8"] + ["ptr"] * 12
    assert re.search(r"#define\s+SPHMI_ABI_VERSION\s+5\b", text)


def test_the_ctypes_wrappers_bind_them_with_the_header_arity():
    """The wrappers run against a recording stand-in for the library: the argtypes they declare and the arguments they pass have the
    header's arity, and the two-call read (how many wait, then the samples) delivers arrays of the documented shapes."""
    from sphexample_amd import _abi
    assert _abi.ABI_VERSION == 5
    seen = []

    class Fn:
        def __init__(self, name):
            self.name, self.argtypes = name, None

        def __call__(self, *args):
            seen.append((self.name, len(self.argtypes), len(args)))
            if self.name == "x_budgets_read":
                args[12]._obj.value = 3                            # three samples wait, then are delivered
                args[13]._obj.value = 2
            return 0

    class Lib:
        def __init__(self):
            self.fns = {n: Fn(n) for n in ("x_budgets_enable", "x_budgets_read")}

        def __getattr__(self, n):
            try:
                return self.__dict__["fns"][n]
            except KeyError:
                raise AttributeError(n)

    b = _abi.Backend.__new__(_abi.Backend)
    b._lib, b._p, b._h = Lib(), "x_", None
    assert b.has_budgets()
    assert inspect.signature(_abi.Backend.budgets_enable).parameters["capacity"].default == 4096
    b.budgets_enable(capacity=7)
    out = b.budgets_read()
    assert seen == [("x_budgets_enable", 2, 2), ("x_budgets_read", 14, 14), ("x_budgets_read", 14, 14)]
    assert list(out) == ["iteration", "time", "dt", "count", "energy", "momentum", "angular", "centre", "extremes", "box"]
    assert out["iteration"].dtype == np.int64 and out["count"].dtype == np.int64
    assert out["iteration"].shape == out["time"].shape == out["dt"].shape == out["count"].shape == (3,)
    for k in ("energy", "momentum", "angular", "centre", "extremes"):
        assert out[k].shape == (3, 3) and out[k].dtype == np.float64, k
    assert out["box"].shape == (3, 6) and b.budgets_dropped == 2


def test_the_julia_shim_binds_the_calls_behind_an_opt_in():
    from test_julia_shim import shim_ccalls
    called = [c[0] for c in shim_ccalls()]
    assert called.count("sphmi_budgets_enable") == 1 and called.count("sphmi_budgets_read") == 2
    shim = open(os.path.join(ROOT, "julia", "SPHExampleMI355X.jl")).read()
    assert 'ENV, "SPHMI_BUDGETS", ""' in shim                 # unset: no enable, no read
    assert "budgets_wanted()" in shim and "haskey(BUDGETS, P) && read_budgets!" in shim


def test_the_kernels_hold_no_float_atomic_and_do_not_spill(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_report
    from sphexample_amd import build
    text = open(os.path.join(ROOT, "sphexample_amd", "csrc", "sphmi_budgets.h")).read()
    assert "atomic" not in text.split("#pragma once", 1)[1]
    lib = build.build()
    co = isa_report.code_object(lib, str(tmp_path))
    meta, isa = isa_report.metadata(co), isa_report.kernels(co)
    names = isa_report.demangle(list(meta))
    for kernel in ("k_bg_partial", "k_bg_final", "k_bg_small"):
        mine = [k for k, d in names.items() if re.search(r"\b%s\b" % kernel, d)]
        assert len(mine) == 2, (kernel, mine)                  # fp32 and fp64 handles
        for k in mine:
            assert meta[k]["scratch_bytes"] == 0, kernel
            # a fixed order of every sum: no floating-point atomic anywhere in the feature's kernels
            assert not [ln for ln in isa[k] if re.search(r"atomic_(add|pk_add|min|max)_f(16|32|64)", ln)], kernel
            assert not [ln for ln in isa[k] if re.search(r"\batomic", ln)], kernel       # … and no other atomic either


def test_the_host_side_under_the_sanitizers(tmp_path):
    """deliver_budgets and the slab combine on hand-made records: a record with n = 0 delivers zeros, extremes that lie in different
    slabs combine, a read with capacity = 0 clears nothing, samples beyond capacity_steps are dropped and counted."""
    main = [ln.split()[1] for ln in open(MAIN).read().splitlines() if ln.startswith("#include")]
    assert [i for i in main if i.startswith('"')] == ['"sphmi_series.h"']
    cxx = host_compiler()
    exe = str(tmp_path / "budgets_main")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", CSRC, MAIN, "-o", exe]
    for extra in (SANITIZE + ("-static-libasan", "-static-libubsan"), SANITIZE, ()):
        built = subprocess.run(base + list(extra), capture_output=True, text=True)
        if built.returncode == 0:
            break
    assert built.returncode == 0, built.stderr
    print("sanitizers:", " ".join(extra) or "none")
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().splitlines()[-1] == "ok", run.stdout
    assert not run.stderr.strip(), run.stderr               # a sanitizer report would be here


def test_the_helpers():
    from sphexample_amd import budgets
    empty = budgets.empty_budgets()
    assert list(empty) == ["iteration", "time", "dt", "count", "energy", "momentum", "angular", "centre", "extremes", "box"]
    assert all(len(a) == 0 for a in empty.values()) and empty["box"].shape == (0, 6) and empty["energy"].shape == (0, 3)
    assert budgets.total_energy(empty).shape == (0,) and budgets.front_position(empty).shape == (0,)
    s = {"energy": np.array([[1.0, 2.0, 0.5], [1e16, 1.0, -1e16]]), "box": np.array([[0.0, 1.0, 2.0, 3.0, 4.0, 5.0], [-1.0, 0.0, 0.0, 0.25, 0.0, 0.0]])}
    np.testing.assert_array_equal(budgets.total_energy(s), [3.5, (1e16 + 1.0) - 1e16])
    np.testing.assert_array_equal(budgets.front_position(s), [3.0, 0.25])
    np.testing.assert_array_equal(budgets.front_position(s, axis=2), [5.0, 0.0])
    np.testing.assert_array_equal(budgets.front_position(s, axis=0, side="min"), [0.0, -1.0])
    for bad in (lambda: budgets.front_position(s, axis=3), lambda: budgets.front_position(s, side="left"),
                lambda: budgets.total_energy({"energy": np.zeros((2, 2))}), lambda: budgets.front_position({"box": np.zeros(6)})):
        try:
            bad()
        except ValueError:
            continue
        raise AssertionError("a malformed argument was accepted")


def test_run_simulation_default_keeps_the_callback(dam_break_2d):
    """budgets=False: the oracle-backed driver (which has no such entry points) runs as before and calls back with two arguments."""
    import copy
    from oracle.oracle import Oracle
    from sphexample_amd import simulation
    assert inspect.signature(simulation.RunSimulation).parameters["budgets"].default is False
    p, s = dam_break_2d
    meta = copy.deepcopy(s.SimMetaData)
    meta.SimulationTime, meta.OutputTimes = 0.0004, 0.0002
    shapes = []
    simulation.RunSimulation(SimGeometry=None, SimMetaData=meta, SimConstants=s.SimConstants, SimKernel=s.SimKernel, SimLogger=None,
                             SimParticles=p.copy(), SimViscosity=s.SimViscosity, SimDensityDiffusion=s.SimDensityDiffusion, backend_factory=Oracle,
                             on_output=lambda *a: shapes.append(len(a)))
    assert len(shapes) >= 2 and set(shapes) == {2}
