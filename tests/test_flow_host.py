"""CPU-side checks of the flow through control boxes (sphmi_flow_enable / sphmi_flow_read): the two prototypes are declared with the
arity the bindings use, exported, wrapped, bound by the Julia shim behind its opt-in; the ABI version stays 5; the kernels live in a
header of their own, hold no atomic and do not spill; the host side (check_flow_table, deliver_flow, the series arithmetic) runs on
hand-made tables and records under the address and undefined-behaviour sanitizers (tests/host_flow/flow_main.cpp); the helpers of
sphexample_amd.flow on hand-made clouds; RunSimulation's default keeps the callback's shape."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_step_series_host import CSRC, SANITIZE, host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "host_flow", "flow_main.cpp")
SYMBOLS = {"sphmi_flow_enable": 5, "sphmi_flow_read": 12}
KEYS = ["iteration", "time", "dt", "count", "volume", "momentum", "entered", "left"]
INF = np.inf


def test_the_entry_points_are_declared_and_exported():
    from test_julia_shim import c_class, c_prototypes, macros
    from sphexample_amd.engine import load_library
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sphmi.h")).read(), flags=re.S)
    protos = c_prototypes()
    lib = load_library()
    for s, arity in SYMBOLS.items():
        assert s in protos, f"{s} is not declared in include/sphmi.h"
        assert protos[s][0] == "int" and len(protos[s][1]) == arity, protos[s]
        assert hasattr(lib, s), f"libsphmi.so does not export {s}"
    assert [c_class(a) for a in protos["sphmi_flow_enable"][1]] == ["ptr", "i4", "ptr", "ptr", "i8"]
    assert [c_class(a) for a in protos["sphmi_flow_read"][1]] == ["ptr", "i8"] + ["ptr"] * 10
    assert macros()["SPHMI_MAX_FLOW_BOXES"] == "16"
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
            if self.name == "x_flow_read":
                args[10]._obj.value = 3                            # three samples wait, then are delivered
                args[11]._obj.value = 2
            return 0

    class Lib:
        def __init__(self):
            self.fns = {n: Fn(n) for n in ("x_flow_enable", "x_flow_read")}

        def __getattr__(self, n):
            try:
                return self.__dict__["fns"][n]
            except KeyError:
                raise AttributeError(n)

    b = _abi.Backend.__new__(_abi.Backend)
    b._lib, b._p, b._h, b.D = Lib(), "x_", None, 2
    assert b.has_flow()
    assert inspect.signature(_abi.Backend.flow_enable).parameters["capacity"].default == 4096
    b.flow_enable([[0.0, -INF], [1.0, -INF]], [[1.0, INF], [INF, INF]], capacity=7)
    out = b.flow_read()
    assert seen == [("x_flow_enable", 5, 5), ("x_flow_read", 12, 12), ("x_flow_read", 12, 12)]
    assert list(out) == KEYS
    assert out["iteration"].shape == out["time"].shape == out["dt"].shape == (3,)
    for k in ("count", "entered", "left", "iteration"):
        assert out[k].dtype == np.int64, k
    for k in ("count", "volume", "entered", "left"):
        assert out[k].shape == (3, 2), k
    assert out["momentum"].shape == (3, 2, 3) and out["volume"].dtype == out["momentum"].dtype == np.float64 and b.flow_dropped == 2
    with pytest.raises(ValueError):
        b.flow_enable([[0.0, 0.0]], [[1.0, 1.0], [2.0, 2.0]])


def test_the_julia_shim_binds_the_calls_behind_an_opt_in():
    from test_julia_shim import shim_ccalls
    called = [c[0] for c in shim_ccalls()]
    assert called.count("sphmi_flow_enable") == 1 and called.count("sphmi_flow_read") == 2
    shim = open(os.path.join(ROOT, "julia", "SPHExampleMI355X.jl")).read()
    assert 'ENV, "SPHMI_FLOW_BOXES", ""' in shim                # unset: no enable, no read
    assert "haskey(FLOW, P) && read_flow!" in shim


def test_the_kernels_hold_no_atomic_and_do_not_spill(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_report
    from sphexample_amd import build
    text = open(os.path.join(ROOT, "sphexample_amd", "csrc", "sphmi_flow.h")).read()
    code = text.split("#pragma once", 1)[1]
    assert "atomic" not in code and code.count("#pragma clang fp contract(off)") >= 3
    # … and the butterfly of the four sums, which the observers share, keeps contraction off as well
    shared = open(os.path.join(ROOT, "sphexample_amd", "csrc", "sphmi_step_record.h")).read()
    assert "#pragma clang fp contract(off)" in shared.split("double wave_sum(double v)", 1)[1].split("\n}\n", 1)[0] and "wave_sum(" in code
    host = open(os.path.join(ROOT, "sphexample_amd", "csrc", "sphmi_series.h")).read()
    assert "#include <hip" not in host and "__device__" not in host and "__global__" not in host          # the host side stays plain C++
    lib = build.build()
    co = isa_report.code_object(lib, str(tmp_path))
    meta, isa = isa_report.metadata(co), isa_report.kernels(co)
    names = isa_report.demangle(list(meta))
    for kernel in ("k_fl_mark", "k_fl_partial", "k_fl_final", "k_fl_small"):
        mine = [k for k, d in names.items() if re.search(r"\b%s\b" % kernel, d)]
        assert len(mine) == 2, (kernel, mine)                  # fp32 and fp64 handles
        for k in mine:
            assert meta[k]["scratch_bytes"] == 0, kernel
            assert meta[k]["vgprs"] <= 64, (kernel, meta[k]["vgprs"])          # nothing indexed per lane: eight waves per SIMD fit
            assert not [ln for ln in isa[k] if "atomic" in ln], kernel          # global_atomic_*, buffer_atomic_*, flat_atomic_*, ds_*: none
            # contraction off: no fused multiply-add on doubles except inside the division's own sequence (k_fl_mark divides nothing)
            if kernel == "k_fl_mark":
                assert not [ln for ln in isa[k] if re.search(r"v_fma_f64|v_div", ln)], kernel


def test_the_host_side_under_the_sanitizers(tmp_path):
    """check_flow_table on every argument error, ±inf bounds and lo == hi; deliver_flow on hand-made records; the capacity and
    dropped arithmetic of a read."""
    main = [ln.split()[1] for ln in open(MAIN).read().splitlines() if ln.startswith("#include")]
    assert [i for i in main if i.startswith('"')] == ['"sphmi_series.h"']
    cxx = host_compiler()
    exe = str(tmp_path / "flow_main")
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


def _cloud(pos, types=None, ids=None):
    pos = np.asarray(pos, dtype=np.float64)
    n = len(pos)
    return {"Position": pos, "Type": np.ones(n, dtype=np.uint8) if types is None else np.asarray(types, dtype=np.uint8),
            "ID": np.arange(1, n + 1) if ids is None else np.asarray(ids, dtype=np.int64)}


def test_restate_on_hand_made_clouds():
    from sphexample_amd import flow
    # boxes: A = [0, 1) x [0, 1);  B = [0.5, 2) x (-inf, +inf), overlapping A;  C = [1, 1.5) x [0, 1), adjacent to A
    lo = np.array([[0.0, 0.0], [0.5, -INF], [1.0, 0.0]])
    hi = np.array([[1.0, 1.0], [2.0, INF], [1.5, 1.0]])
    # a row exactly on lo is inside, a row exactly on hi is outside (and inside the adjacent box: no gap, no overlap)
    edge = flow.inside([[0.0, 0.0], [1.0, 0.5], [np.nextafter(1.0, 0.0), 0.5], [0.5, 1.0], [2.0, 7.0], [0.5, -1e300]], lo, hi)
    np.testing.assert_array_equal(edge, [[True, False, False], [False, True, True], [True, True, False], [False, True, False],
                                         [False, False, False], [False, True, False]])
    before = _cloud([[0.25, 0.5],      # stays in A, enters B
                     [0.25, 0.5],      # A -> C, through B's lo
                     [-0.5, 0.5],      # jumps from left of A across the whole of A and C to x = 1.75: counts nowhere in A or C, enters B
                     [0.75, 0.5],      # in A and B, leaves both through the top and the right
                     [0.75, 0.5],      # Fixed: ignored although it moves like the row above
                     [1.0, 0.25],      # on C's lo (inside C, B), moves onto A's hi = C's lo again: nothing changes
                     [3.0, 0.5]],      # outside everything, comes to rest exactly on B's hi: still outside
                    types=[1, 1, 1, 1, 2, 1, 1])
    after = _cloud([[0.5, 0.5], [1.25, 0.5], [1.75, 0.5], [2.5, 1.5], [2.5, 1.5], [1.0, 0.75], [2.0, 0.5]], types=[1, 1, 1, 1, 2, 1, 1])
    r = flow.restate(before, after, lo, hi)
    np.testing.assert_array_equal(r["count"], [1, 4, 2])
    np.testing.assert_array_equal(r["entered"], [0, 3, 1])
    np.testing.assert_array_equal(r["left"], [2, 1, 0])
    n_before = flow.restate(before, before, lo, hi)["count"]
    np.testing.assert_array_equal(r["count"] - n_before, r["entered"] - r["left"])
    # the rows of the second download in another order (a rebuild permutes them): matched by ID, the same answer
    perm = np.array([3, 0, 6, 2, 5, 1, 4])
    shuffled = {k: v[perm] for k, v in after.items()}
    for k, v in flow.restate(before, shuffled, lo, hi).items():
        np.testing.assert_array_equal(v, r[k], err_msg=k)
    # downloads that do not hold the same Fluid rows, or ambiguous IDs, are refused
    with pytest.raises(ValueError):
        flow.restate(before, _cloud(after["Position"], types=[1, 1, 1, 1, 1, 1, 1]), lo, hi)
    with pytest.raises(ValueError):
        flow.restate(_cloud(before["Position"], ids=[1, 1, 2, 3, 4, 5, 6]), after, lo, hi)


def test_strips_tile_space():
    from sphexample_amd import flow
    rng = np.random.default_rng(5)
    for dims in (2, 3):
        for axis in range(dims):
            edges = [-0.5, 0.0, 0.25, 1.0]
            lo, hi = flow.strips(axis, edges, dims)
            assert lo.shape == hi.shape == (5, dims)
            assert lo[0, axis] == -INF and hi[-1, axis] == INF
            np.testing.assert_array_equal(lo[1:, axis], edges)
            np.testing.assert_array_equal(hi[:-1, axis], edges)             # adjacent: one's hi is the next one's lo
            other = [d for d in range(dims) if d != axis]
            assert (lo[:, other] == -INF).all() and (hi[:, other] == INF).all() and (lo < hi).all()
            pos = rng.normal(0.0, 1.0, (400, dims))
            pos[:len(edges), axis] = edges                                  # rows exactly on every edge
            types = rng.integers(1, 4, 400).astype(np.uint8)
            member = flow.inside(pos, lo, hi)
            assert (member.sum(axis=1) == 1).all()                          # every row in exactly one strip
            np.testing.assert_array_equal(np.nonzero(member[:len(edges)])[1], [1, 2, 3, 4])      # a row on an edge: the strip that starts there
            d = _cloud(pos, types=types)
            assert flow.restate(d, d, lo, hi)["count"].sum() == int((types == 1).sum())         # counts sum to the fluid count
    for bad in (lambda: flow.strips(2, [0.0], 2), lambda: flow.strips(0, [0.0, 0.0], 3), lambda: flow.strips(0, [1.0, 0.0], 3),
                lambda: flow.strips(0, [np.nan], 2), lambda: flow.strips(0, [INF], 2), lambda: flow.strips(0, [0.0], 4)):
        with pytest.raises(ValueError):
            bad()
    lo, hi = flow.strips(1, [], 3)                                          # no edge: the one box that holds everything
    assert lo.shape == (1, 3) and (lo == -INF).all() and (hi == INF).all()


def test_the_series_helpers():
    from sphexample_amd import flow
    empty = flow.empty_flow(3)
    assert list(empty) == KEYS and all(len(a) == 0 for a in empty.values())
    assert empty["count"].shape == (0, 3) and empty["momentum"].shape == (0, 3, 3) and empty["entered"].dtype == np.int64
    assert flow.cumulative(empty).shape == (0, 3) and flow.net_mass_rate(empty, 0.5).shape == (0, 3)
    s = {"dt": np.array([0.5, 0.25, 0.125]), "entered": np.array([[4, 0], [1, 2], [0, 0]]), "left": np.array([[1, 0], [3, 0], [0, 5]])}
    np.testing.assert_array_equal(flow.net_mass_rate(s, 2.0), [[12.0, 0.0], [-16.0, 16.0], [0.0, -80.0]])
    np.testing.assert_array_equal(flow.discharge(s, 2.0, 1000.0), np.array([[12.0, 0.0], [-16.0, 16.0], [0.0, -80.0]]) / 1000.0)
    np.testing.assert_array_equal(flow.cumulative(s), [[3, 0], [1, 2], [1, -3]])


def test_run_simulation_default_keeps_the_callback(dam_break_2d):
    """flow_boxes=None: the oracle-backed driver (which has no such entry points) runs as before and calls back with two arguments."""
    import copy
    from oracle.oracle import Oracle
    from sphexample_amd import simulation
    assert inspect.signature(simulation.RunSimulation).parameters["flow_boxes"].default is None
    p, s = dam_break_2d
    meta = copy.deepcopy(s.SimMetaData)
    meta.SimulationTime, meta.OutputTimes = 0.0004, 0.0002
    shapes = []
    simulation.RunSimulation(SimGeometry=None, SimMetaData=meta, SimConstants=s.SimConstants, SimKernel=s.SimKernel, SimLogger=None,
                             SimParticles=p.copy(), SimViscosity=s.SimViscosity, SimDensityDiffusion=s.SimDensityDiffusion, backend_factory=Oracle,
                             on_output=lambda *a: shapes.append(len(a)))
    assert len(shapes) >= 2 and set(shapes) == {2}
