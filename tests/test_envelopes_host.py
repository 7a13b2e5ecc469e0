"""CPU-side checks of the per-particle envelopes (sphmi_envelopes_enable / sphmi_envelopes_read): the two prototypes are declared
with the arity the bindings use, exported, wrapped, bound by the Julia shim behind its opt-in; the ABI version stays 5; the kernels
live in a header of their own, hold no atomic and use no scratch; the host side (check_envelope_mask, deliver_envelope_window,
deliver_envelope_speed) runs under the address and undefined-behaviour sanitizers (tests/host_envelopes/envelopes_main.cpp);
`sphexample_amd.envelopes.update` on hand-made sequences; RunSimulation's default keeps the callback's shape."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_step_series_host import CSRC, SANITIZE, host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "host_envelopes", "envelopes_main.cpp")
SYMBOLS = {"sphmi_envelopes_enable": 2, "sphmi_envelopes_read": 11}
KEYS = ["steps", "t_begin", "t_end", "duration", "p_max", "t_p_max", "p_min", "impulse", "square", "loaded", "speed_max", "t_arrival"]
INF = np.inf


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
    assert [c_class(a) for a in protos["sphmi_envelopes_enable"][1]] == ["ptr", "i4"]
    assert [c_class(a) for a in protos["sphmi_envelopes_read"][1]] == ["ptr"] * 11
    assert re.search(r"#define\s+SPHMI_ABI_VERSION\s+5\b", text)


def test_the_ctypes_wrappers_bind_them_with_the_header_arity():
    """The wrappers run against a recording stand-in for the library: the argtypes they declare and the arguments they pass have the
    header's arity, the mask is built from the type names, and a read delivers the documented keys and shapes."""
    from sphexample_amd import _abi
    assert _abi.ABI_VERSION == 5
    seen = []

    class Fn:
        def __init__(self, name):
            self.name, self.argtypes = name, None

        def __call__(self, *args):
            seen.append((self.name, len(self.argtypes), len(args), args[1] if self.name == "x_envelopes_enable" else None))
            if self.name == "x_envelopes_read":
                args[1]._obj.value = 12                            # steps
                np.ctypeslib.as_array((C.c_double * 3).from_address(args[2].value))[:] = [0.5, 2.0, 1.5]
                np.ctypeslib.as_array((C.c_double * 5).from_address(args[9].value))[:] = [0.0, 1.0, 2.0, 3.0, 4.0]
            return 0

    class Lib:
        def __init__(self):
            self.fns = {n: Fn(n) for n in ("x_envelopes_enable", "x_envelopes_read")}

        def __getattr__(self, n):
            try:
                return self.__dict__["fns"][n]
            except KeyError:
                raise AttributeError(n)

    b = _abi.Backend.__new__(_abi.Backend)
    b._lib, b._p, b._h, b.D, b.N = Lib(), "x_", None, 2, 5
    assert b.has_envelopes()
    assert inspect.signature(_abi.Backend.envelopes_enable).parameters["types"].default == ("Fluid",)
    b.envelopes_enable()
    b.envelopes_enable(("Fluid", "Fixed", 3))
    b.envelopes_enable("Moving")
    b.envelopes_enable(())
    out = b.envelopes_read()
    assert seen == [("x_envelopes_enable", 2, 2, 2), ("x_envelopes_enable", 2, 2, 14), ("x_envelopes_enable", 2, 2, 8), ("x_envelopes_enable", 2, 2, 0),
                    ("x_envelopes_read", 11, 11, None)]
    assert list(out) == KEYS
    assert out["steps"] == 12 and isinstance(out["steps"], int) and (out["t_begin"], out["t_end"], out["duration"]) == (0.5, 2.0, 1.5)
    for k in KEYS[4:]:
        assert out[k].shape == (5,) and out[k].dtype == np.float64, k
    np.testing.assert_array_equal(out["speed_max"], [0.0, 1.0, 2.0, 3.0, 4.0])       # the eighth pointer of the ten
    with pytest.raises(ValueError):
        b.envelopes_enable(("Water",))


def test_the_julia_shim_binds_the_calls_behind_an_opt_in():
    from test_julia_shim import shim_ccalls
    called = [c[0] for c in shim_ccalls()]
    assert called.count("sphmi_envelopes_enable") == 1 and called.count("sphmi_envelopes_read") == 1
    shim = open(os.path.join(ROOT, "julia", "SPHExampleMI355X.jl")).read()
    assert 'ENV, "SPHMI_ENVELOPES", ""' in shim                  # unset: no enable, no read
    assert "haskey(ENVELOPES, P) && read_envelopes!" in shim
    assert "function envelopes_enable(" in shim and "function envelopes_read(" in shim


def test_the_kernels_hold_no_atomic_and_use_no_scratch(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_report
    from sphexample_amd import build
    text = open(os.path.join(ROOT, "sphexample_amd", "csrc", "sphmi_envelopes.h")).read()
    code = text.split("#pragma once", 1)[1]
    assert "atomic" not in code and "#pragma clang fp contract(off)" in code and "sqrt" not in code
    assert "eos7<T>" in code                                     # the Pressure is formed by the function k_pack_output uses …
    pack = open(os.path.join(ROOT, "sphexample_amd", "csrc", "sphmi_rebuild.h")).read().split("k_pack_output(", 1)[1].split("\n}\n", 1)[0]
    assert "eos7<T>(half0[i].w" in pack                          # … shared, not copied
    host = open(os.path.join(ROOT, "sphexample_amd", "csrc", "sphmi_series.h")).read()
    assert "#include <hip" not in host and "__device__" not in host and "__global__" not in host          # the host side stays plain C++
    lib = build.build()
    co = isa_report.code_object(lib, str(tmp_path))
    meta, isa = isa_report.metadata(co), isa_report.kernels(co)
    names = isa_report.demangle(list(meta))
    for kernel, variants in (("k_en_update", 2), ("k_en_fill", 1)):
        mine = [k for k, d in names.items() if re.search(r"\b%s\b" % kernel, d)]
        assert len(mine) == variants, (kernel, mine)             # k_en_update: fp32 and fp64 handles
        for k in mine:
            assert meta[k]["scratch_bytes"] == 0 and meta[k]["lds_bytes"] == 0, kernel
            assert meta[k]["vgprs"] <= 64, (kernel, meta[k]["vgprs"])          # nothing indexed per lane: eight waves per SIMD fit
            assert not [ln for ln in isa[k] if "atomic" in ln], kernel
            assert not [ln for ln in isa[k] if re.search(r"v_sqrt|v_rsq", ln)], kernel
            # the record travels in 16-byte pieces
            assert len([ln for ln in isa[k] if "global_store_dwordx4" in ln]) >= 4, kernel
    for k in [k for k, d in names.items() if re.search(r"\bk_en_update<float>", d)]:
        # contraction off: on fp32 handles (whose equation of state runs in fp32) no double is ever fused
        assert not [ln for ln in isa[k] if "v_fma_f64" in ln]


def test_the_host_side_under_the_sanitizers(tmp_path):
    """check_envelope_mask on every mask, the window header's delivery, the sqrt of the largest speed."""
    main = [ln.split()[1] for ln in open(MAIN).read().splitlines() if ln.startswith("#include")]
    assert [i for i in main if i.startswith('"')] == ['"sphmi_series.h"']
    cxx = host_compiler()
    exe = str(tmp_path / "envelopes_main")
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


def test_update_on_hand_made_sequences():
    from sphexample_amd import envelopes
    st = envelopes.start(6, t_begin=1.0)
    for k, v in (("p_max", -INF), ("t_p_max", 0.0), ("p_min", INF), ("impulse", 0.0), ("square", 0.0), ("loaded", 0.0), ("speed2_max", 0.0), ("t_arrival", INF)):
        assert st[k].shape == (6,) and st[k].dtype == np.float64 and (st[k] == v).all(), k
    assert (st["steps"], st["t_begin"], st["t_end"], st["duration"]) == (0, 1.0, 1.0, 0.0)
    sel = np.array([True, True, True, True, False, True])
    # rows: 0 rises and repeats its peak | 1 never loaded | 2 NaN in the middle | 3 loaded from the second step | 4 unselected | 5 2-D speed
    P = [[5.0, -1.0, 2.0, 0.0, 9.0, 1.0],
         [7.0, -3.0, np.nan, 4.0, 9.0, 1.0],
         [7.0, -2.0, 8.0, -4.0, 9.0, 1.0]]
    V = [[[3.0, 4.0]] * 6, [[0.0, 1.0]] * 6, [[6.0, 8.0]] * 5 + [[1.0, 1.0]]]
    t, dt = [1.5, 1.75, 2.0], [0.5, 0.25, 0.25]
    for k in range(3):
        assert envelopes.update(st, sel, P[k], V[k], t[k], dt[k]) is st
    r = envelopes.result(st)
    assert list(r) == KEYS
    assert (r["steps"], r["t_begin"], r["t_end"], r["duration"]) == (3, 1.0, 2.0, 1.0)
    # strict first attainment: row 0 reaches 7.0 at t = 1.75 and again at 2.0 — the first time stays
    assert r["p_max"][0] == 7.0 and r["t_p_max"][0] == 1.75 and r["p_min"][0] == 5.0
    assert r["impulse"][0] == 5.0 * 0.5 + 7.0 * 0.25 + 7.0 * 0.25 and r["square"][0] == 25.0 * 0.5 + 49.0 * 0.25 + 49.0 * 0.25
    assert r["loaded"][0] == 1.0 and r["t_arrival"][0] == 1.5
    # never loaded: t_arrival stays inf, loaded stays 0; the peak of a negative history is its least negative value, at its first time
    assert r["t_arrival"][1] == INF and r["loaded"][1] == 0.0 and r["p_max"][1] == -1.0 and r["t_p_max"][1] == 1.5 and r["p_min"][1] == -3.0
    # a NaN never wins a comparison and poisons the sums
    assert r["p_max"][2] == 8.0 and r["t_p_max"][2] == 2.0 and r["p_min"][2] == 2.0 and np.isnan(r["impulse"][2]) and np.isnan(r["square"][2])
    assert r["loaded"][2] == 0.75 and r["t_arrival"][2] == 1.5
    # P == 0 is not a load; the arrival is the END of the first step with P > 0
    assert r["t_arrival"][3] == 1.75 and r["loaded"][3] == 0.25 and r["p_max"][3] == 4.0 and r["p_min"][3] == -4.0
    # an unselected row keeps the start record
    for k, v in (("p_max", -INF), ("t_p_max", 0.0), ("p_min", INF), ("impulse", 0.0), ("square", 0.0), ("loaded", 0.0), ("speed_max", 0.0), ("t_arrival", INF)):
        assert r[k][4] == v, k
    # the largest speed: |(6, 8)| = 10, 2-D rows carry vz = 0; row 5 peaked at the first step
    assert (r["speed_max"][[0, 1, 2, 3]] == 10.0).all() and r["speed_max"][5] == 5.0
    # 3-D: vz takes part
    st3 = envelopes.start(1)
    envelopes.update(st3, [True], [1.0], [[1.0, 2.0, 2.0]], 0.1, 0.1)
    assert envelopes.result(st3)["speed_max"][0] == 3.0
    # a NaN speed never wins either
    envelopes.update(st3, [True], [1.0], [[np.nan, 0.0, 0.0]], 0.2, 0.1)
    assert envelopes.result(st3)["speed_max"][0] == 3.0
    # the products are rounded on their own, in the order of the table: impulse + (P * dt), square + ((P * P) * dt)
    a, d = 1.0 + 2.0 ** -30, 1.0 / 3.0
    st1 = envelopes.start(1)
    envelopes.update(st1, [True], [a], [[0.0, 0.0]], d, d)
    envelopes.update(st1, [True], [a], [[0.0, 0.0]], 2 * d, d)
    assert st1["impulse"][0] == (a * d) + (a * d) and st1["square"][0] == ((a * a) * d) + ((a * a) * d)
    assert st1["duration"] == d + d


def test_the_derived_quantities():
    from sphexample_amd import envelopes
    env = {"steps": 4, "t_begin": 1.0, "t_end": 3.0, "duration": 2.0, "impulse": np.array([4.0, 0.0, -1.0]), "square": np.array([18.0, 0.0, 2.0]),
           "t_arrival": np.array([1.5, INF, 3.0]), "p_max": np.array([5.0, -INF, 1.0])}
    np.testing.assert_array_equal(envelopes.mean_pressure(env), [2.0, 0.0, -0.5])
    np.testing.assert_array_equal(envelopes.rms_pressure(env), [3.0, 0.0, 1.0])
    arrival = envelopes.arrival_map(env)
    assert arrival[0] == 0.5 and np.isnan(arrival[1]) and arrival[2] == 2.0
    keyed = envelopes.by_id(env, [30, 10, 20])
    np.testing.assert_array_equal(keyed["id"], [10, 20, 30])
    np.testing.assert_array_equal(keyed["impulse"], [0.0, -1.0, 4.0])
    np.testing.assert_array_equal(keyed["p_max"], [-INF, 1.0, 5.0])
    assert keyed["steps"] == 4 and keyed["duration"] == 2.0
    with pytest.raises(ValueError):
        envelopes.by_id(env, [1, 1, 2])


def test_run_simulation_default_keeps_the_callback(dam_break_2d):
    """envelopes=None: the oracle-backed driver (which has no such entry points) runs as before and calls back with two arguments."""
    import copy
    from oracle.oracle import Oracle
    from sphexample_amd import simulation
    assert inspect.signature(simulation.RunSimulation).parameters["envelopes"].default is None
    p, s = dam_break_2d
    meta = copy.deepcopy(s.SimMetaData)
    meta.SimulationTime, meta.OutputTimes = 0.0004, 0.0002
    shapes = []
    simulation.RunSimulation(SimGeometry=None, SimMetaData=meta, SimConstants=s.SimConstants, SimKernel=s.SimKernel, SimLogger=None,
                             SimParticles=p.copy(), SimViscosity=s.SimViscosity, SimDensityDiffusion=s.SimDensityDiffusion, backend_factory=Oracle,
                             on_output=lambda *a: shapes.append(len(a)))
    assert len(shapes) >= 2 and set(shapes) == {2}
