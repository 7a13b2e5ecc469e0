"""CPU-side checks of the attached-columns entry points (sphmi_attach_columns / sphmi_download_columns*): declared, exported,
wrapped and bound; the gather kernel is one straight kernel with 16-byte loads; the bench kernels did not move; and the oracle-backed
RunSimulation still takes the host gathers."""
import copy
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("sphmi_attach_columns", "sphmi_download_columns_begin", "sphmi_download_columns")


def test_the_entry_points_are_declared_and_exported():
    from sphexample_amd.engine import load_library
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sphmi.h")).read(), flags=re.S)
    lib = load_library()
    for s in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, text), f"{s} is not declared in include/sphmi.h"
        assert hasattr(lib, s), f"libsphmi.so does not export {s}"
    assert re.search(r"#define\s+SPHMI_MAX_COLUMNS\s+16\b", text) and re.search(r"#define\s+SPHMI_MAX_COLUMN_ROW_BYTES\s+64\b", text)
    assert re.search(r"#define\s+SPHMI_ABI_VERSION\s+5\b", text)


def test_the_ctypes_wrappers_exist():
    from sphexample_amd import _abi
    for name in ("attach_columns", "download_columns", "download_columns_begin", "has_columns"):
        assert callable(getattr(_abi.Backend, name))
    assert (_abi.MAX_COLUMNS, _abi.MAX_COLUMN_ROW_BYTES, _abi.ABI_VERSION) == (16, 64, 5)


def test_the_julia_shim_binds_the_columns_and_keeps_the_permutation():
    from test_julia_shim import shim_ccalls
    called = [c[0] for c in shim_ccalls()]
    assert "sphmi_attach_columns" in called and "sphmi_download_columns_begin" in called
    assert called.count("sphmi_download_permutation") == 1
    assert 'ENV, "SPHMI_COLUMNS"' in open(os.path.join(ROOT, "julia", "SPHExampleMI355X.jl")).read()


def test_gather_kernel_isa_and_the_bench_kernels(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench
    import isa_report
    from sphexample_amd import build
    lib = build.build()
    co = isa_report.code_object(lib, str(tmp_path))
    meta, isa = isa_report.metadata(co), isa_report.kernels(co)
    names = isa_report.demangle(list(meta))
    gather = [k for k, d in names.items() if "k_gather_columns" in d]
    assert len(gather) == 1
    assert meta[gather[0]]["scratch_bytes"] == 0
    loads = [ln for ln in isa[gather[0]] if re.search(r"\b(global|buffer)_load_dwordx4\b", ln)]
    assert loads, "k_gather_columns has no 16-byte global load"
    for helper in ("k_columns_base_init", "k_columns_base_compose"):
        assert sum(helper in d for d in names.values()) == 1
    # the committed counter record is keyed on the ISA of the two bench kernels: the new kernels live in a header of their own
    record = json.load(open(os.path.join(ROOT, bench.COUNTER_RECORD)))
    ident = bench.loaded_kernel_identity()
    assert "error" not in ident, ident
    for which in ("predictor", "corrector"):
        assert ident[which]["isa_sha16"] == record["kernels"][which]["isa_sha16"], which


def test_oracle_backed_run_simulation_keeps_the_host_gathers(dam_break_2d_mdbc, monkeypatch):
    """The oracle has no column entry points: with it RunSimulation gathers on the host exactly as before, whatever SPHMI_COLUMNS says."""
    from oracle.oracle import Oracle
    from sphexample_amd import simulation
    p, s = dam_break_2d_mdbc
    host_gather = simulation.permute_passive_fields
    calls = {"n": 0}

    def counted(*a, **kw):
        calls["n"] += 1
        return host_gather(*a, **kw)

    monkeypatch.setattr(simulation, "permute_passive_fields", counted)
    got = {}
    for switch in (None, "0"):
        if switch is None:
            monkeypatch.delenv("SPHMI_COLUMNS", raising=False)
        else:
            monkeypatch.setenv("SPHMI_COLUMNS", switch)
        calls["n"] = 0
        meta = copy.deepcopy(s.SimMetaData)
        meta.SimulationTime, meta.OutputTimes = 0.002, 0.001
        q = p.copy()
        q.ChunkID[:] = q.ID * 3 + 1
        snaps = []
        simulation.RunSimulation(SimGeometry=None, SimMetaData=meta, SimConstants=s.SimConstants, SimKernel=s.SimKernel, SimLogger=None,
                                 SimParticles=q, SimViscosity=s.SimViscosity, SimDensityDiffusion=s.SimDensityDiffusion, backend_factory=Oracle,
                                 on_output=lambda m, pp: snaps.append({k: getattr(pp, k).copy() for k in simulation.PASSIVE_FIELDS + ("ID",)}))
        assert len(snaps) >= 3 and calls["n"] == len(snaps) - 1
        for sn in snaps:
            np.testing.assert_array_equal(sn["ChunkID"], sn["ID"] * 3 + 1)
        got[switch] = snaps
    for a, b in zip(got[None], got["0"]):
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
