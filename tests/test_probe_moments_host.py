"""Host side of the per-step moment sums (sphmi_probe_moments_enable / sphmi_probe_moments_read, csrc/sphmi_probe_moments.h): the two
prototypes, their entries in the prototype table and the feature map, their export and their wrappers; the Julia shim's binding; the
argument check and the delivery under the address and undefined-behaviour sanitizers (tests/host_probe_moments/probe_moments_main.cpp);
what the cross-compiled code object says about k_probe_moments; `probes.fit_series` — exact for a linear field at probes with
one-sided supports, and equal to `fields.linear_fit` applied step by step; the RunSimulation plumbing with a stand-in backend.
No GPU.

Bar of the linear-exactness test: the fitted value within 1e-12 of the field's range over the probe's support.  The fit solves a
(D + 1) × (D + 1) system in fp64 whose reciprocal condition number the test asserts to be above 1e-3: rounding of the sums (n ≤ 60
rows: a few 1e-16 relative) times 1 / rcond stays below 1e-12."""
import copy
import ctypes as C
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

from sphexample_amd import _abi
from test_field_grid_host import _StandIn, _prototype
from test_point_gradients_host import _cfg
from test_point_moments_host import KEYS, as_sums, brute_force_point_moments
from test_step_series_host import CSRC, SANITIZE, host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "host_probe_moments", "probe_moments_main.cpp")
SHAPES = {"weight": (), "count": (), "sum_pressure": (), "sum_density": (), "sum_velocity": (3,), "moment1": (3,), "moment2": (3, 3),
          "moment_pressure": (3,), "moment_density": (3,), "moment_velocity": (3, 3)}


# ---- the symbols ------------------------------------------------------------------------------------------------------------------
def test_header_table_and_library_agree():
    text = open(os.path.join(ROOT, "include", "sphmi.h")).read()
    assert re.search(r"#define\s+SPHMI_ABI_VERSION\s+5\b", text) and _abi.ABI_VERSION == 5      # append-only: the version stays
    assert _prototype("sphmi_probe_moments_enable") == _prototype("sphmi_probes_enable") == ["sphmi_handle*", "int32_t", "const double*", "int64_t"]
    read = _prototype("sphmi_probe_moments_read")
    assert read == ["sphmi_handle*", "int64_t", "int64_t*", "double*", "double*", "double*", "int64_t*"] + ["double*"] * 8 + ["int64_t*", "int64_t*"]
    assert read[:7] == _prototype("sphmi_probes_read")[:7] and read[-2:] == _prototype("sphmi_probes_read")[-2:]      # the calling convention of the probes
    assert read[5:15] == _prototype("sphmi_sample_point_moments")[3:]             # … delivering the outputs of the on-demand sampler
    assert text.index("int sphmi_select_release(") < text.index("int sphmi_probe_moments_enable(") < text.index("int sphmi_probe_moments_read(")      # appended
    P = _abi.PROTOTYPES
    assert P["probe_moments_enable"] == P["probes_enable"] and len(P["probe_moments_read"]) == len(read) == len(P["probes_read"]) + 5
    assert P["probe_moments_read"][-2:] == _abi._SERIES_TAIL
    assert list(P).index("probes_read") + 1 == list(P).index("probe_moments_enable")      # in the one table, beside the probes
    assert _abi.FEATURES["probe_moments"] == ("probe_moments_enable", "probe_moments_read") and list(_abi.FEATURES).index("probe_moments") == list(_abi.FEATURES).index("probes") + 1
    from sphexample_amd.engine import load_library
    lib = load_library()
    assert hasattr(lib, "sphmi_probe_moments_enable") and hasattr(lib, "sphmi_probe_moments_read")
    series = open(os.path.join(CSRC, "sphmi_series.h")).read()
    assert series.count("inline void check_probe_table(") == 1 and "const char* fn = \"sphmi_probes_enable\"" in series      # one check, two names
    assert "deliver_probe_moments(" in series and series.count("constexpr OutputSlots kPmOutputs[]") == 1
    engine = open(os.path.join(CSRC, "sphmi_engine.hip")).read()
    assert engine.count("RawOutputs out(sphmi::kPmOutputs") == 2                   # both moment entry points read the layout from the one table


class _ReadFn:
    """Stands in for sphmi_probe_moments_read: two steps wait, three were dropped; fills count and moment2 with known values."""
    argtypes = None

    def __init__(self, probes):
        self.calls, self.probes = [], probes

    def __call__(self, *a):
        self.calls.append(a)
        a[15]._obj.value, a[16]._obj.value = 2, 3
        if a[1]:
            np.ctypeslib.as_array((C.c_int64 * 2).from_address(a[2].value))[:] = [7, 8]
            np.ctypeslib.as_array((C.c_int64 * (2 * self.probes)).from_address(a[6].value))[:] = np.arange(2 * self.probes)
            np.ctypeslib.as_array((C.c_double * (2 * self.probes * 6)).from_address(a[11].value))[:] = np.tile([11.0, 12.0, 13.0, 22.0, 23.0, 33.0], 2 * self.probes)
        return _abi.OK


def test_the_wrappers_bind_them_with_the_header_arity():
    from test_field_grid_host import _Recorder
    b = _abi.Backend.__new__(_abi.Backend)
    b._lib, b._p, b._h, b.N, b.D = _Recorder(), "sphmi_", C.c_void_p(), 10, 2
    b.cfg = types.SimpleNamespace(h=0.02)
    assert b.has_probe_moments() is True
    b.probe_moments_enable([[0.1, 0.2], [0.3, 0.4], [0.5, 0.6]], capacity=9)
    fe = b._lib.fns["sphmi_probe_moments_enable"]
    assert fe.argtypes == [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64] and fe.calls[0][1] == 3 and fe.calls[0][3] == 9
    assert b._moment_probes == 3 and b._probes == 0                               # a point set of its own
    b._lib.fns["sphmi_probe_moments_read"] = fr = _ReadFn(3)
    out = b.probe_moments_read()
    assert len(fr.argtypes) == 17 == len(_prototype("sphmi_probe_moments_read")) and [len(c) for c in fr.calls] == [17, 17]
    assert fr.calls[0][1] == 0 and all(a is None for a in fr.calls[0][2:15]) and fr.calls[1][1] == 2      # the question, then the fetch
    assert list(out) == ["iteration", "time", "dt"] + list(KEYS) + ["h", "dims", "probe_moments_dropped"] and list(KEYS) == list(_abi.Backend.MOMENT_FIELDS)
    assert (out["h"], out["dims"], out["probe_moments_dropped"], b.probe_moments_dropped) == (0.02, 2, 3, 3)
    assert out["iteration"].tolist() == [7, 8] and out["count"].dtype == np.int64 and out["count"].tolist() == [[0, 1, 2], [3, 4, 5]]
    for key, shape in SHAPES.items():
        assert out[key].shape == (2, 3, *shape) and out[key].flags.c_contiguous, key
    np.testing.assert_array_equal(out["moment2"][1, 2], [[11, 12, 13], [12, 22, 23], [13, 23, 33]])      # the six fill the symmetric matrix
    b.probe_moments_enable(np.zeros((0, 2)))                                       # an empty set travels as n = 0 with a null table
    assert fe.calls[1][1] == 0 and fe.calls[1][2] is None and b._moment_probes == 0
    b._moment_probes = 5
    b.upload = _abi.Backend.upload.__get__(b)
    b._ft = np.float64
    b.upload(np.zeros((10, 2)), np.zeros((10, 2)), np.zeros((10, 2)), np.zeros(10), np.ones(10), np.arange(10))
    assert b._moment_probes == 0                                                   # sphmi_upload disables


def test_the_julia_shim_binds_the_calls_behind_an_opt_in():
    from test_julia_shim import c_prototypes, shim_ccalls
    calls = [c for c in shim_ccalls() if c[0].startswith("sphmi_probe_moments_")]
    assert [c[0] for c in calls].count("sphmi_probe_moments_enable") == 1 and [c[0] for c in calls].count("sphmi_probe_moments_read") == 2
    for sym, _, tys, args in calls:
        assert len(tys) == len(args) == len(c_prototypes()[sym][1])
    shim = open(os.path.join(ROOT, "julia", "SPHExampleMI355X.jl"), encoding="utf-8").read()
    assert 'probe_positions(D, "SPHMI_PROBE_MOMENTS")' in shim                    # the syntax of SPHMI_PROBES: unset, no enable and no read
    assert "haskey(PROBE_MOMENTS, P) && read_probe_moments!" in shim and "function read_probe_moments!(" in shim


# ---- the stand-alone host program ---------------------------------------------------------------------------------------------------
def test_the_host_side_under_the_sanitizers(tmp_path):
    """check_probe_table under both names on every refusal, deliver_probe_moments against a hand-built record."""
    main = [ln.split()[1] for ln in open(MAIN).read().splitlines() if ln.startswith("#include")]
    assert [i for i in main if i.startswith('"')] == ['"sphmi_series.h"']
    cxx = host_compiler()
    exe = str(tmp_path / "probe_moments_main")
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


# ---- the code object ----------------------------------------------------------------------------------------------------------------
def test_the_kernel_is_built_for_gfx950_without_scratch(tmp_path):
    """The code object's metadata: both instantiations of k_probe_moments — float and double records — use no scratch and no LDS,
    are declared for workgroups of 256 (one wave per SIMD) and stay within the 512 registers that leaves a lane; the probes' walk
    they share keeps its figures; no kernel of the library uses scratch.  The walk is stated once: the kernel's header calls pr_walk
    and holds no cut of its own."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_report
    from sphexample_amd import build
    text = open(os.path.join(CSRC, "sphmi_probe_moments.h"), encoding="utf-8").read()
    head, code = text.split("#pragma once", 1)
    assert "not to the bit" in head.lower() and "k_point_moments" in head          # the order of summation differs: said in the header
    assert "pr_walk<T>(A, xp, lane, m)" in code and "r2 <= " not in code and "cstart" not in code and "atomic" not in code
    assert "#pragma clang fp contract(off)" in code and "z.add(" in code            # slots 0 … 6 by the probes' own statements
    probes = open(os.path.join(CSRC, "sphmi_probes.h"), encoding="utf-8").read()
    assert probes.count("r2 <= A.H2") == 1 and probes.count("template <class T, class Sums>") == 1
    if not os.path.exists(build.LIB):
        pytest.skip("the library is not built (python -m sphexample_amd.build)")
    co = isa_report.code_object(build.LIB, str(tmp_path))
    meta, isa = isa_report.metadata(co), isa_report.kernels(co)
    names = isa_report.demangle(list(meta))
    mine = {names[k]: k for k in meta if "sphmi::k_probe_moments<" in names[k]}
    assert len(mine) == 2 and any("<float>" in n for n in mine) and any("<double>" in n for n in mine), sorted(mine)
    for d, k in sorted(mine.items()):
        v = meta[k]
        print(f"{d}: {v['vgprs']} VGPRs, {v['agprs']} AGPRs, {v['sgprs']} SGPRs, {v['lds_bytes']} B LDS, {v['scratch_bytes']} B scratch")
        assert v["scratch_bytes"] == 0 and v["lds_bytes"] == 0, (d, v)
        assert v["max_flat_workgroup_size"] == 256 and v["vgprs"] + v["agprs"] <= 512, (d, v)
        assert v["vgprs"] >= 62, (d, v)                                            # 31 fp64 sums live in registers
        assert not [ln for ln in isa[k] if "atomic" in ln], d
    for ty in ("float", "double"):
        walk = [k for k, d in names.items() if re.search(r"\bk_probe_sample<%s>" % ty, d)]
        assert len(walk) == 1 and meta[walk[0]]["scratch_bytes"] == 0 and meta[walk[0]]["vgprs"] <= 128, ty
    spilling = [names[k] for k, v in meta.items() if v["scratch_bytes"] != 0]
    assert not spilling, spilling[:4]


# ---- fit_series -----------------------------------------------------------------------------------------------------------------------
def _record(dims, steps=3, probes=12, seed=2):
    """A synthetic record: `probes` points ON the plane x = 0 with rows only on the side x ≤ 0 (one-sided supports), random volumes,
    and per step another linear field P = a + b·x, ρ = a' + b'·x, v likewise.  Returns (record, coefficients per step, points, rows, cfg)."""
    cfg = _cfg(0, dims)
    rng = np.random.default_rng(seed)
    pts = np.concatenate([np.zeros((probes, 1)), rng.uniform(-0.3, 0.3, (probes, dims - 1))], axis=1)
    rows = rng.uniform(-0.6, 0.6, (4000 if dims == 2 else 9000, dims))
    rows = rows[rows[:, 0] <= 0.0]
    vol = cfg.dx ** dims * rng.uniform(0.5, 1.5, len(rows))
    rec = {"iteration": np.arange(1, steps + 1), "time": 0.1 * np.arange(1, steps + 1), "dt": np.full(steps, 0.1), "h": cfg.h, "dims": dims}
    per_step, coefs = [], []
    for k in range(steps):
        coef = {name: (rng.uniform(-2.0, 2.0) * scale, rng.standard_normal(dims) * scale) for name, scale in (("P", 3000.0), ("v0", 1.0), ("v1", 1.0), ("v2", 1.0))}
        field = lambda name: coef[name][0] + rows @ coef[name][1]                  # noqa: E731
        vel = np.stack([field(f"v{a}") for a in range(dims)], axis=1)
        ref = brute_force_point_moments(cfg, pts, rows, vel, cfg.m0 / vol, field("P"), np.ones(len(rows), np.uint8))
        per_step.append(as_sums(ref, cfg, dims))
        coefs.append(coef)
    for key in KEYS:
        rec[key] = np.stack([s[key] for s in per_step])
    return rec, coefs, per_step, pts, rows, cfg


@pytest.mark.parametrize("dims", [2, 3])
def test_fit_series_reproduces_a_linear_field_at_one_sided_probes(dims):
    from sphexample_amd.probes import fit_series
    rec, coefs, per_step, pts, rows, cfg = _record(dims)
    fit = fit_series(rec)
    K, M = rec["weight"].shape
    assert fit["pressure"].shape == fit["density"].shape == fit["linear"].shape == fit["rcond"].shape == (K, M)
    assert fit["velocity"].shape == fit["pressure_gradient"].shape == (K, M, 3) and fit["velocity_gradient"].shape == (K, M, 3, 3)
    assert fit["linear"].all() and fit["rcond"].min() > 1e-3                       # the conditioning the bar relies on
    assert np.array_equal(fit["iteration"], rec["iteration"]) and np.array_equal(fit["time"], rec["time"])
    # one-sided: the centroid of every support lies a fraction of h inside x < 0
    assert ((rec["moment1"][:, :, 0] / rec["weight"]) < -0.15 * cfg.h).all()
    worst, shepard = 0.0, np.inf
    for k in range(K):
        for name, got, mean in [("P", fit["pressure"][k], rec["sum_pressure"][k] / rec["weight"][k])] + \
                [(f"v{a}", fit["velocity"][k][:, a], rec["sum_velocity"][k][:, a] / rec["weight"][k]) for a in range(dims)]:
            a0, b = coefs[k][name]
            want = a0 + pts @ b
            span = np.array([np.ptp(a0 + rows[((rows - x) ** 2).sum(1) <= cfg.H2] @ b) for x in pts])
            assert (span > 0).all()
            worst = max(worst, (np.abs(got - want) / span).max())
            shepard = min(shepard, np.median(np.abs(mean - want) / span))
    print(f"{dims}-D: {K} steps x {M} probes, rcond {fit['rcond'].min():.3g} … {fit['rcond'].max():.3g}; fit within {worst:.3g} of the range, the Shepard mean misses by {shepard:.3g} (median)")
    assert worst <= 1e-12, worst
    assert shepard > 1e-3                                                          # what the fit removes
    if dims == 2:
        assert (fit["velocity"][:, :, 2] == 0).all() and (fit["pressure_gradient"][:, :, 2] == 0).all()


@pytest.mark.parametrize("dims", [2, 3])
def test_fit_series_is_linear_fit_step_by_step(dims):
    from sphexample_amd.fields import linear_fit
    from sphexample_amd.probes import empty_probe_moments, fit_series
    rec, _, per_step, pts, rows, cfg = _record(dims, steps=4, probes=9, seed=5)
    # make some entries fall back: a probe without rows at one step, one below the row count at another
    for key in KEYS:
        rec[key][1, 2] = 0
        per_step[1][key][2] = 0
    rec["count"][2, 4] = dims
    per_step[2]["count"][4] = dims
    for kw in ({}, {"min_rcond": 0.05}, {"min_count": 12}):
        fit = fit_series(rec, **kw)
        for k in range(rec["weight"].shape[0]):
            one = linear_fit(per_step[k], **kw)
            assert set(one) <= set(fit)
            for name, v in one.items():
                assert np.array_equal(fit[name][k], v), (kw, k, name)
    fit = fit_series(rec)
    assert not fit["linear"][1, 2] and fit["pressure"][1, 2] == 0 and not fit["linear"][2, 4] and fit["linear"].sum() == fit["linear"].size - 2
    assert fit["pressure"][2, 4] == rec["sum_pressure"][2, 4] / rec["weight"][2, 4] and (fit["pressure_gradient"][2, 4] == 0).all()      # the Shepard mean
    empty = fit_series(empty_probe_moments(5, dims, cfg.h))
    assert empty["pressure"].shape == (0, 5) and empty["velocity_gradient"].shape == (0, 5, 3, 3) and len(empty["iteration"]) == 0
    with pytest.raises(ValueError):
        fit_series(per_step[0])                                                    # the dict of one on-demand call: no steps axis


# ---- RunSimulation ----------------------------------------------------------------------------------------------------------------------
class _SeriesStandIn(_StandIn):
    def probe_moments_enable(self, positions, capacity):
        self.log.append(("probe_moments_enable", len(positions), capacity))
        self.points = np.array(positions)

    def probe_moments_read(self):
        self.log.append(("probe_moments_read", self.iteration))
        return {"iteration": np.arange(self.iteration - 2, self.iteration + 1), "weight": np.zeros((3, len(self.points)))}


def test_run_simulation_hands_the_records_to_the_callback():
    from conftest import load_dam_break_2d
    from sphexample_amd import simulation
    p, s = load_dam_break_2d()
    cloud = [[0.1, 0.2], [0.3, 0.4]]

    def run(**kw):
        meta = copy.deepcopy(s.SimMetaData)
        meta.SimulationTime, meta.OutputTimes = 0.002, 0.001
        got = []
        _StandIn.instances.clear()
        steps = simulation.RunSimulation(SimGeometry=None, SimMetaData=meta, SimConstants=s.SimConstants, SimKernel=s.SimKernel, SimLogger=None,
                                         SimParticles=p.copy(), SimViscosity=s.SimViscosity, SimDensityDiffusion=s.SimDensityDiffusion,
                                         backend_factory=_SeriesStandIn, on_output=lambda m, pp, *extra: got.append((m.Iteration, extra)), **kw)
        return steps, got, _StandIn.instances[0]

    steps, got, eng = run(probe_moments=cloud)
    assert len(got) == len(steps) + 1 >= 3
    first = got[0][1][0]                                                           # before the first step: an empty record, as probes= hands one over
    assert got[0][0] == 0 and len(first["iteration"]) == 0 and first["moment2"].shape == (0, 2, 3, 3) and (first["h"], first["dims"]) == (s.SimKernel.h, 2)
    assert eng.points.tolist() == cloud and ("probe_moments_enable", 2, 1 << 16) in eng.log
    for iteration, extra in got[1:]:
        assert len(extra) == 1 and extra[0]["iteration"][-1] == iteration          # the steps of THIS interval
    seq = [e[0] for e in eng.log if isinstance(e, tuple)]
    assert seq == ["probe_moments_enable"] + ["advance", "probe_moments_read", "download"] * len(steps)
    _, got2, eng2 = run()
    assert all(extra == () for _, extra in got2) and not any(e[0].startswith("probe_moments") for e in eng2.log if isinstance(e, tuple))
