"""CPU-side checks of the tracers (sphmi_tracers_enable / sphmi_tracers_read): the two prototypes are declared with the argument
classes the bindings use, exported, wrapped, bound by the Julia shim behind its opt-in; the ABI version stays 5; the kernels live in a
header of their own, hold no atomic and use no scratch, and the drifters call the probes' walk instead of copying it; the argument
checks (check_tracer_table) and the delivery run under the address and undefined-behaviour sanitizers
(tests/host_tracers/tracers_main.cpp); `sphexample_amd.tracers.step` against a direct O(M·N) enumeration on a small random cloud;
`pathlines`, `dry` and `by_id` on hand-made reads; RunSimulation's default keeps the callback's shape."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from test_step_series_host import CSRC, SANITIZE, host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "host_tracers", "tracers_main.cpp")
ENABLE = ["ptr", "i4", "ptr", "i4", "ptr", "f8", "i8"]
READ = ["ptr", "i8"] + ["ptr"] * 8


def test_the_entry_points_are_declared_and_exported():
    from test_julia_shim import c_class, c_prototypes, macros
    from sphexample_amd.engine import load_library
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sphmi.h")).read(), flags=re.S)
    protos = c_prototypes()
    lib = load_library()
    for s in ("sphmi_tracers_enable", "sphmi_tracers_read"):
        assert s in protos, f"{s} is not declared in include/sphmi.h"
        assert protos[s][0] == "int"
        assert hasattr(lib, s), f"libsphmi.so does not export {s}"
    assert [c_class(a) for a in protos["sphmi_tracers_enable"][1]] == ENABLE
    assert [c_class(a) for a in protos["sphmi_tracers_read"][1]] == READ
    assert macros()["SPHMI_MAX_TRACERS"] == "1024"
    assert re.search(r"#define\s+SPHMI_ABI_VERSION\s+5\b", text)


def test_the_ctypes_wrappers_bind_them_with_the_header_arity():
    """The wrappers run against a recording stand-in for the library: the argtypes they declare and the arguments they pass have the
    header's arity, and a read delivers the documented keys, shapes and views."""
    from sphexample_amd import _abi
    seen = []

    class Fn:
        def __init__(self, name):
            self.name, self.argtypes = name, None

        def __call__(self, *args):
            seen.append((self.name, len(self.argtypes), len(args), args[1], args[3] if self.name == "x_tracers_enable" else None))
            if self.name == "x_tracers_read":
                args[8]._obj.value = 2                             # two steps wait
                args[9]._obj.value = 5
                if args[1]:
                    np.ctypeslib.as_array((C.c_int64 * 2).from_address(args[2].value))[:] = [7, 8]
                    np.ctypeslib.as_array((C.c_double * (2 * 3 * 8)).from_address(args[5].value))[:] = np.arange(48.0)
                    dv = np.ctypeslib.as_array((C.c_double * (2 * 2 * 10)).from_address(args[6].value)).reshape(2, 2, 10)
                    dv[:] = 0.0
                    dv[0, 0] = [1.0, 2.0, 3.0, 0.5, 1.5, 500.0, 0.25, -0.5, 1.0, 4.0]      # X, S, SP, Srho, Sv, n
                    dv[1, 1, :3] = [9.0, 9.0, 9.0]                                          # an empty drifter: S = 0, n = 0
                    np.ctypeslib.as_array((C.c_double * 6).from_address(args[7].value))[:] = [1.5, 1.0, 5.0, 9.0, 9.0, 9.0]
            return 0

    class Lib:
        def __init__(self):
            self.fns = {n: Fn(n) for n in ("x_tracers_enable", "x_tracers_read")}

        def __getattr__(self, n):
            try:
                return self.__dict__["fns"][n]
            except KeyError:
                raise AttributeError(n)

    b = _abi.Backend.__new__(_abi.Backend)
    b._lib, b._p, b._h, b.D, b.N = Lib(), "x_", None, 3, 50
    assert b.has_tracers()
    sig = inspect.signature(_abi.Backend.tracers_enable).parameters
    assert sig["particles"].default is None and sig["drifters"].default is None and sig["min_weight"].default == 0.5
    b.tracers_enable(particles=[4, 0, 49], drifters=[[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]])
    out = b.tracers_read()
    assert seen == [("x_tracers_enable", 7, 7, 3, 2), ("x_tracers_read", 10, 10, 0, None), ("x_tracers_read", 10, 10, 2, None)]
    assert list(out) == ["iteration", "time", "dt", "particles", "drifters", "drifter_position", "min_weight", "dropped"]
    assert list(out["particles"]) == ["values", "position", "velocity", "density", "pressure"]
    assert list(out["drifters"]) == ["position", "sums", "weight", "count", "pressure", "density", "velocity"]
    np.testing.assert_array_equal(out["iteration"], [7, 8])
    P = out["particles"]
    assert P["values"].shape == (2, 3, 8) and P["position"].shape == (2, 3, 3) and P["velocity"].shape == (2, 3, 3) and P["density"].shape == (2, 3)
    np.testing.assert_array_equal(P["values"].reshape(-1), np.arange(48.0))
    np.testing.assert_array_equal(P["position"][1, 2], [40.0, 41.0, 42.0]); np.testing.assert_array_equal(P["velocity"][0, 1], [11.0, 12.0, 13.0])
    assert P["density"][0, 0] == 6.0 and P["pressure"][1, 2] == 47.0
    Dr = out["drifters"]
    assert Dr["position"].shape == (2, 2, 3) and Dr["sums"].shape == (2, 2, 7) and Dr["velocity"].shape == (2, 2, 3) and Dr["count"].dtype == np.int64
    assert Dr["weight"][0, 0] == 0.5 and Dr["count"][0, 0] == 4 and Dr["pressure"][0, 0] == 3.0 and Dr["density"][0, 0] == 1000.0
    np.testing.assert_array_equal(Dr["velocity"][0, 0], [0.5, -1.0, 2.0])
    assert Dr["weight"][1, 1] == 0 and Dr["count"][1, 1] == 0 and Dr["pressure"][1, 1] == 0 and (Dr["velocity"][1, 1] == 0).all()      # empty: zeros, no NaN
    np.testing.assert_array_equal(out["drifter_position"], [[1.5, 1.0, 5.0], [9.0, 9.0, 9.0]])
    assert out["dropped"] == 5 and b.tracers_dropped == 5 and out["min_weight"] == 0.5
    # either kind may be absent; neither disables
    seen.clear()
    b.tracers_enable(drifters=np.zeros((4, 3)), min_weight=0.25)
    b.tracers_enable(particles=np.arange(5))
    b.tracers_enable()
    assert [(s[3], s[4]) for s in seen] == [(0, 4), (5, 0), (0, 0)]


def test_the_julia_shim_binds_the_calls_behind_an_opt_in():
    from test_julia_shim import shim_ccalls
    called = [c[0] for c in shim_ccalls()]
    assert called.count("sphmi_tracers_enable") == 1 and called.count("sphmi_tracers_read") == 1
    shim = open(os.path.join(ROOT, "julia", "SPHExampleMI355X.jl")).read()
    assert 'ENV, "SPHMI_TRACERS", ""' in shim                    # unset: no enable, no read
    assert "haskey(TRACERS, P) && read_tracers!" in shim
    assert "function tracers_enable(" in shim and "function read_tracers!(" in shim


def test_the_kernels_hold_no_atomic_and_use_no_scratch(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_report
    from sphexample_amd import build
    text = open(os.path.join(ROOT, "sphexample_amd", "csrc", "sphmi_tracers.h")).read()
    head, code = text.split("#pragma once", 1)
    assert "first order" in head.lower() and "X_k[d] = X_{k−1}[d] + U_d * dt" in head        # the scheme and its update rule are stated
    assert "atomic" not in code and "#pragma clang fp contract(off)" in code
    assert "eos7<T>" in code and "pr_walk<T>(A.s" in code        # the Pressure of k_pack_output, the walk of k_probe_sample: shared, not copied
    probes = open(os.path.join(ROOT, "sphexample_amd", "csrc", "sphmi_probes.h")).read()
    assert probes.count("pr_walk<T>(A,") == 1 and code.count("r2 <= ") == 0
    host = open(os.path.join(ROOT, "sphexample_amd", "csrc", "sphmi_series.h")).read()
    assert "#include <hip" not in host and "__device__" not in host and "__global__" not in host          # the host side stays plain C++
    lib = build.build()
    co = isa_report.code_object(lib, str(tmp_path))
    meta, isa = isa_report.metadata(co), isa_report.kernels(co)
    names = isa_report.demangle(list(meta))
    for kernel, variants in (("k_tr_particles", 2), ("k_tr_drift", 2), ("k_tr_map_init", 1)):
        mine = [k for k, d in names.items() if re.search(r"\b%s\b" % kernel, d)]
        assert len(mine) == variants, (kernel, mine)             # fp32 and fp64 handles
        for k in mine:
            assert meta[k]["scratch_bytes"] == 0 and meta[k]["lds_bytes"] == 0, kernel
            assert not [ln for ln in isa[k] if "atomic" in ln], kernel
    for k in [k for k, d in names.items() if re.search(r"\bk_tr_particles\b", d)]:
        assert meta[k]["vgprs"] <= 64, meta[k]["vgprs"]
    for k in [k for k, d in names.items() if re.search(r"\bk_tr_particles<float>", d)]:
        # record + low word is an addition: on fp32 handles (whose equation of state runs in fp32) no double is ever fused
        assert not [ln for ln in isa[k] if "v_fma_f64" in ln or "v_fmac_f64" in ln]
    # the drifters run the probes' walk: the same butterfly, the same loads in flight
    for ty in ("float", "double"):
        walk = [k for k, d in names.items() if re.search(r"\bk_probe_sample<%s>" % ty, d)]
        drift = [k for k, d in names.items() if re.search(r"\bk_tr_drift<%s>" % ty, d)]
        assert len(walk) == 1 and len(drift) == 1
        count = lambda k, pat: len([ln for ln in isa[k] if re.search(pat, ln)])               # noqa: E731
        for pat in (r"ds_bpermute_b32", r"v_rsq_f64", r"v_ceil_f64", r"v_floor_f64"):
            assert count(drift[0], pat) == count(walk[0], pat), (ty, pat)
        assert count(drift[0], r"v_rcp_f64") == count(walk[0], r"v_rcp_f64") + 3              # … and three divisions more: U = Sv / S


def test_the_host_side_under_the_sanitizers(tmp_path):
    """check_tracer_table on every refusal (SPHMI_ERR_ARGUMENT, the prefix `sphmi_tracers_enable: `), deliver_tracers."""
    main = [ln.split()[1] for ln in open(MAIN).read().splitlines() if ln.startswith("#include")]
    assert [i for i in main if i.startswith('"')] == ['"sphmi_series.h"']
    cxx = host_compiler()
    exe = str(tmp_path / "tracers_main")
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


# ---- tracers.step against a direct enumeration -----------------------------------------------------------------------------------
def _cfg(D, kernel=0):
    h = 0.0625                                                            # H = 1/8 and H² = 1/64 are exact doubles
    H = 2 * h
    alphaD = (7 / (4 * math.pi * h * h) if D == 2 else 21 / (16 * math.pi * h ** 3)) if kernel == 0 else (10 / (7 * math.pi * h * h) if D == 2 else 1 / (math.pi * h ** 3))
    return SimpleNamespace(kernel=kernel, alphaD=alphaD, h=h, h_inv=1 / h, H=H, H2=H * H, m0=0.8, dims=D)


def _w(cfg, q):
    """W(q), scalar, written out from the definition (Wendland C2 / cubic spline)."""
    if cfg.kernel == 1:
        a = 1 - 1.5 * q * q + 0.75 * q ** 3 if q <= 1 else 0.0
        b = 0.25 * (2 - q) ** 3 if 1 < q <= 2 else 0.0
        return cfg.alphaD * (a + b)
    return cfg.alphaD * (1 - q / 2) ** 4 * (2 * q + 1)


def _enumerate(cfg, X, st):
    """Every drifter against every row, one pair at a time, in Python floats."""
    M, D = X.shape
    out = {"n": np.zeros(M, np.int64), "S": np.zeros(M), "SP": np.zeros(M), "Srho": np.zeros(M), "Sv": np.zeros((M, 3))}
    for k in range(M):
        for j in range(len(st["Type"])):
            if st["Type"][j] != 1:
                continue
            d = [float(X[k, a]) - float(st["Position"][j, a]) for a in range(D)]
            r2 = d[0] * d[0] + d[1] * d[1]
            if D == 3:
                r2 = r2 + d[2] * d[2]
            if not r2 <= cfg.H2:
                continue
            w = (cfg.m0 / float(st["Density"][j])) * _w(cfg, math.sqrt(r2) * cfg.h_inv)
            out["n"][k] += 1; out["S"][k] += w; out["SP"][k] += w * float(st["Pressure"][j]); out["Srho"][k] += w * float(st["Density"][j])
            for a in range(D):
                out["Sv"][k, a] += w * float(st["Velocity"][j, a])
    return out


@pytest.mark.parametrize("D,kernel", [(2, 0), (3, 0), (2, 1)])
def test_step_against_a_direct_enumeration(D, kernel):
    from sphexample_amd import tracers
    cfg = _cfg(D, kernel)
    rng = np.random.default_rng(17 + D)
    N = 400
    dp = 0.025
    st = {"Position": rng.uniform(0.0, 0.5 if D == 2 else 0.3, (N, D)), "Velocity": rng.normal(0.0, 2.0, (N, D)), "Density": rng.uniform(990.0, 1010.0, N),
          "Pressure": rng.normal(0.0, 500.0, N), "Type": np.where(rng.uniform(size=N) < 0.8, 1, 2).astype(np.uint8)}
    # the cloud is dense enough for S ~ 1 in its middle: m0 / rho · (rows per unit volume) = 1
    cfg.m0 = 1000.0 * (0.5 ** 2 if D == 2 else 0.3 ** 3) / (0.8 * N)
    F = np.flatnonzero(st["Type"] == 1)
    X = rng.uniform(0.13, 0.37 if D == 2 else 0.17, (12, D))
    X[0] = st["Position"][F[3]]                                           # exactly on a particle: r = 0 is legal
    # a row exactly at r² = H²: the drifter H away from a Fluid row along x, where the subtraction and the square are exact
    st["Position"][F[5]] = 0.25
    X[1] = 0.25; X[1, 0] = 0.375
    d = X[1] - st["Position"][F[5]]
    assert d[0] * d[0] + d[1] * d[1] + (d[2] * d[2] if D == 3 else 0.0) == cfg.H2
    X[2] = 5.0                                                            # nothing within H: empty
    X[3] = st["Position"][F[np.argmin(st["Position"][F, 0])]]             # outside the cloud, 0.7 H from its outermost Fluid row: a few rows,
    X[3, 0] -= 0.7 * cfg.H                                                # S below min_weight — dry
    dt, min_weight = 1e-3, 0.5
    Xn, s = tracers.step(X, st, cfg, dt, min_weight)
    ref = _enumerate(cfg, X, st)
    np.testing.assert_array_equal(s["n"], ref["n"])
    for q in ("S", "SP", "Srho", "Sv"):
        scale = np.abs(ref[q]).max()
        assert np.abs(s[q] - ref[q]).max() <= 1e-12 * scale, q            # the same terms, added in another order
    assert ref["n"][0] > 0 and ref["n"][2] == 0 and s["S"][2] == 0 and ref["n"][3] > 0 and 0 < ref["S"][3] < min_weight
    # the row at the cut counts (inclusive), and is flagged; W vanishes there, so it adds to n alone
    without = dict(st, Type=st["Type"].copy()); without["Type"][F[5]] = 2
    assert ref["n"][1] == _enumerate(cfg, X[1:2], without)["n"][0] + 1 and s["near"][1]
    # the move, operation by operation in Python floats: wet drifters move, dry and empty ones have not moved by a bit
    wet = ref["S"] >= min_weight
    assert wet[0] and wet.sum() >= 6 and not wet[2] and not wet[3]
    for k in range(len(X)):
        for a in range(D):
            want = float(X[k, a]) + (float(s["Sv"][k, a]) / float(s["S"][k])) * dt if s["S"][k] >= min_weight else float(X[k, a])
            assert Xn[k, a] == want, (k, a)
    assert Xn.shape == X.shape and (Xn[wet] != X[wet]).any()
    # move() alone: NaN and negative weights are dry; a 3-column X of a 2-D run keeps its third column
    Y = tracers.move(np.array([[1.0, 2.0, 0.0]] * 3), [np.nan, -1.0, 2.0], [[1.0, 1.0, 7.0]] * 3, 0.5, 0.5)
    np.testing.assert_array_equal(Y, [[1.0, 2.0, 0.0], [1.0, 2.0, 0.0], [1.25, 2.25, 1.75]])


def _read(K, m, n, x0, it0, min_weight=0.5):
    pos = x0 + np.arange(K)[:, None, None] * np.ones((K, m, 3))
    values = np.arange(K * n * 8, dtype=np.float64).reshape(K, n, 8) + 1000 * it0
    return {"iteration": np.arange(it0, it0 + K), "time": 0.1 * np.arange(it0, it0 + K), "dt": np.full(K, 0.1),
            "particles": {"values": values, "position": values[:, :, :3], "velocity": values[:, :, 3:6], "density": values[:, :, 6], "pressure": values[:, :, 7]},
            "drifters": {"position": pos, "weight": np.tile(np.linspace(0.0, 1.0, m), (K, 1))},
            "drifter_position": x0 + K * np.ones((m, 3)), "min_weight": min_weight, "dropped": 0}


def test_pathlines_dry_and_by_id():
    from sphexample_amd import tracers
    a, b = _read(3, 4, 2, 0.0, 1), _read(2, 4, 2, 3.0, 4)
    path = tracers.pathlines([None, a, b])                               # the first callback of a run hands over None
    assert path.shape == (6, 4, 3)                                        # five executed steps and the position now
    np.testing.assert_array_equal(path[:, 0, 0], np.arange(6.0))
    np.testing.assert_array_equal(tracers.pathlines(a), np.concatenate([a["drifters"]["position"], a["drifter_position"][None]]))
    dry = tracers.dry([a, b])
    assert dry.shape == (5, 4) and dry.dtype == bool
    np.testing.assert_array_equal(dry[0], [True, True, False, False])     # weights 0, 1/3, 2/3, 1 against 0.5
    keyed = tracers.by_id([a, b], [30, 10])
    np.testing.assert_array_equal(keyed["id"], [10, 30])
    np.testing.assert_array_equal(keyed["iteration"], np.arange(1, 6))
    assert keyed["values"].shape == (5, 2, 8) and keyed["position"].shape == (5, 2, 3)
    np.testing.assert_array_equal(keyed["values"][:3, 0], a["particles"]["values"][:, 1])
    np.testing.assert_array_equal(keyed["pressure"][3:, 1], b["particles"]["pressure"][:, 0])
    with pytest.raises(ValueError):
        tracers.by_id(a, [1, 1])
    with pytest.raises(ValueError):
        tracers.by_id(a, [1, 2, 3])
    with pytest.raises(ValueError):
        tracers.pathlines([None])


def test_run_simulation_default_keeps_the_callback(dam_break_2d):
    """tracers=None: the oracle-backed driver (which has no such entry points) runs as before and calls back with two arguments."""
    import copy
    from oracle.oracle import Oracle
    from sphexample_amd import simulation
    assert inspect.signature(simulation.RunSimulation).parameters["tracers"].default is None
    p, s = dam_break_2d
    meta = copy.deepcopy(s.SimMetaData)
    meta.SimulationTime, meta.OutputTimes = 0.0004, 0.0002
    shapes = []
    simulation.RunSimulation(SimGeometry=None, SimMetaData=meta, SimConstants=s.SimConstants, SimKernel=s.SimKernel, SimLogger=None,
                             SimParticles=p.copy(), SimViscosity=s.SimViscosity, SimDensityDiffusion=s.SimDensityDiffusion, backend_factory=Oracle,
                             on_output=lambda *a: shapes.append(len(a)))
    assert len(shapes) >= 2 and set(shapes) == {2}
