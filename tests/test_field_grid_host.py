"""Host side of the lattice sampler (sphmi_sample_grid, csrc/sphmi_field_grid.h): the prototype and its binding, the helpers of
sphexample_amd/fields.py, the RunSimulation plumbing with a stand-in backend, and what the built code object says about the
kernel.  No GPU."""
import copy
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from sphexample_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "sphmi.h")).read()


def _prototype(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", _header(), re.S)
    assert m, f"{name} is not declared in include/sphmi.h"
    args = []
    for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(","):
        a = " ".join(a.split())
        star = "*" if "*" in a else ""
        args.append(" ".join(a.replace("*", " ").split()[:-1]) + star)
    return args


class _Fn:
    argtypes = None

    def __init__(self):
        self.calls = []

    def __call__(self, *a):
        self.calls.append(a)
        return _abi.OK


class _Recorder:
    """Stands in for the library: remembers the argtypes and arguments a Backend method hands over and answers OK."""
    def __init__(self):
        self.fns = {}

    def __getattr__(self, name):
        if name.startswith("sphmi_"):
            return self.fns.setdefault(name, _Fn())
        raise AttributeError(name)


def _backend(dims):
    b = _abi.Backend.__new__(_abi.Backend)
    b._lib, b._p, b._h, b.N, b.D = _Recorder(), "sphmi_", C.c_void_p(), 10, dims
    return b


def test_header_and_binding_agree():
    text = _header()
    assert re.search(r"#define\s+SPHMI_ABI_VERSION\s+5\b", text) and _abi.ABI_VERSION == 5      # append-only: the version stays
    m = re.search(r"#define\s+SPHMI_MAX_GRID_NODES\s+\(1\s*<<\s*(\d+)\)", text)
    assert m and 1 << int(m.group(1)) == _abi.MAX_GRID_NODES == 1 << 24
    assert _prototype("sphmi_sample_grid") == ["sphmi_handle*", "const double*", "const double*", "const int64_t*", "double*", "int64_t*",
                                               "double*", "double*", "double*"]
    b = _backend(3)
    out = b.sample_grid([0.1, 0.2, 0.3], [0.5, 0.25, 0.125], [4, 3, 2])
    fn = b._lib.fns["sphmi_sample_grid"]
    assert fn.argtypes == [C.c_void_p] * 9 and len(fn.calls) == 1 and len(fn.calls[0]) == 9
    # shapes: counts reversed — x fastest — and three velocity components
    assert set(out) == {"weight", "count", "pressure", "density", "velocity"}
    assert out["weight"].shape == out["pressure"].shape == out["density"].shape == out["count"].shape == (2, 3, 4)
    assert out["velocity"].shape == (2, 3, 4, 3) and out["count"].dtype == np.int64 and out["weight"].dtype == np.float64
    assert all(a.flags.c_contiguous for a in out.values())
    # a subset of the fields: the others travel as NULL
    b2 = _backend(2)
    out = b2.sample_grid([0.0, 0.0], [1.0, 1.0], [5, 7], fields=("weight", "velocity"))
    assert set(out) == {"weight", "velocity"} and out["weight"].shape == (7, 5) and out["velocity"].shape == (7, 5, 3)
    call = b2._lib.fns["sphmi_sample_grid"].calls[0]
    assert [a is None for a in call[4:]] == [False, True, True, True, False]
    for bad in (lambda: b2.sample_grid([0.0], [1.0, 1.0], [5, 7]), lambda: b2.sample_grid([0.0, 0.0], [1.0, 1.0], [5, 7], fields=("vorticity",))):
        with pytest.raises(ValueError):
            bad()


def test_grid_nodes_order_and_exact_doubles():
    from sphexample_amd.fields import grid_axes, grid_nodes
    origin, spacing, counts = [0.1, -0.7, 1e-3], [0.3, 0.07, 1.0 / 3.0], [4, 3, 5]
    X = grid_nodes(origin, spacing, counts)
    assert X.shape == (60, 3) and X.dtype == np.float64
    for k in range(5):
        for j in range(3):
            for i in range(4):
                n = i + 4 * (j + 3 * k)                                             # x fastest: the order of VTK image data
                want = [origin[d] + float(idx) * spacing[d] for d, idx in enumerate((i, j, k))]      # one multiply, one add, in doubles
                assert X[n].tolist() == want, (i, j, k)
    assert X[3, 0] == 0.1 + 3.0 * 0.3
    ax = grid_axes(origin, spacing, counts)
    assert [len(a) for a in ax] == counts and all((np.diff(a) > 0).all() for a in ax)
    X2 = grid_nodes([0.5, 0.25], [0.125, 2.0], [3, 2])
    assert X2.tolist() == [[0.5, 0.25], [0.625, 0.25], [0.75, 0.25], [0.5, 2.25], [0.625, 2.25], [0.75, 2.25]]
    # the flattened arrays of sample_grid line up with the rows of grid_nodes
    w = np.arange(6.0).reshape(2, 3)                                               # shaped counts[::-1]
    assert w.reshape(-1)[4] == w[1, 1] and X2[4].tolist() == [0.625, 2.25]
    for bad in (lambda: grid_nodes([0, 0], [1, 0], [2, 2]), lambda: grid_nodes([0, np.nan], [1, 1], [2, 2]), lambda: grid_nodes([0, 0], [1, 1], [2, 0]),
                lambda: grid_nodes([0], [1], [2]), lambda: grid_nodes([0, 0], [1, 1, 1], [2, 2])):
        with pytest.raises(ValueError):
            bad()


def test_surface_height_on_synthetic_columns():
    from sphexample_amd.fields import surface_height
    nz, ny, nx = 11, 2, 3
    origin, spacing = [0.0, 0.0, 0.2], [0.5, 0.5, 0.1]
    z = origin[2] + np.arange(nz) * spacing[2]
    S = np.zeros((nz, ny, nx))
    S[:, 0, 1] = 1.0                                                               # submerged → the top node
    S[:, 0, 2] = np.where(z <= 0.6 + 1e-12, 1.0, 0.0)                              # a crossing between 0.6 and 0.7
    S[:, 1, 0] = np.clip(1.0 - (z - 0.5) / 0.2, 0.0, 1.0)                          # a linear ramp 1 → 0 over [0.5, 0.7]: ½ at 0.6
    S[:, 1, 1] = 0.3                                                               # spray below the threshold everywhere → dry
    eta = surface_height(S, origin, spacing)
    assert eta.shape == (ny, nx)
    assert eta[0, 0] == 0.2 and eta[1, 1] == 0.2 and eta[1, 2] == 0.2              # dry → the base of the lattice
    assert eta[0, 1] == z[-1]
    assert eta[0, 2] == pytest.approx(0.65) and eta[1, 0] == pytest.approx(0.6)
    assert surface_height(S, origin, spacing, threshold=0.25)[1, 0] == pytest.approx(0.65)
    # 2-D: the vertical is y, one height per x
    eta2 = surface_height(S[:, 0, :], [0.0, 0.2], [0.5, 0.1])
    assert eta2.shape == (nx,) and eta2.tolist() == eta[0].tolist()
    for bad in (lambda: surface_height(S[:, 0, 0], [0.2], [0.1]), lambda: surface_height(S, [0.0, 0.2], [0.5, 0.1])):
        with pytest.raises(ValueError):
            bad()


class _StandIn:
    """What RunSimulation asks of a backend, without a device: three steps per advance, a lattice sample that tells which
    state it was taken on."""
    instances = []

    def __init__(self, cfg):
        self.cfg, self.iteration, self.t, self.log = cfg, 0, 0.0, []
        _StandIn.instances.append(self)

    def upload_particles(self, p): self.log.append("upload")
    def set_motions(self, g): pass
    def pin(self, p): pass
    def unpin(self): pass
    def close(self): self.log.append("close")
    def set_clock(self, iteration, t): self.iteration, self.t = iteration, t
    def _has(self, name): return False
    def download_into(self, p): self.log.append(("download", self.iteration))

    def advance(self, t_target):
        self.iteration += 3
        self.t = t_target + 1e-9
        self.log.append(("advance", self.iteration))
        pr = _abi.SphmiProgress()
        pr.iteration, pr.total_time, pr.last_dt, pr.index_counter, pr.steps_done = self.iteration, self.t, 1e-4, 7, 3
        return pr

    def group_forces_enable(self, markers, capacity): self.markers = list(markers)

    def group_forces_read(self):
        return (np.arange(3), np.zeros(3), np.zeros(3), np.zeros((3, len(self.markers), 3)))

    def sample_grid(self, origin, spacing, counts):
        self.log.append(("sample_grid", self.iteration))
        shape = tuple(int(c) for c in counts)[::-1]
        return {"weight": np.full(shape, float(self.iteration)), "count": np.zeros(shape, np.int64), "pressure": np.zeros(shape),
                "density": np.zeros(shape), "velocity": np.zeros(shape + (3,)), "lattice": (tuple(origin), tuple(spacing), tuple(counts))}


def test_run_simulation_hands_the_fields_to_the_callback():
    from conftest import load_dam_break_2d
    from sphexample_amd import simulation
    p, s = load_dam_break_2d()
    lattice = ([0.05, 0.01], [0.1, 0.05], [12, 9])

    def run(**kw):
        meta = copy.deepcopy(s.SimMetaData)
        meta.SimulationTime, meta.OutputTimes = 0.002, 0.001
        got = []
        _StandIn.instances.clear()
        steps = simulation.RunSimulation(SimGeometry=None, SimMetaData=meta, SimConstants=s.SimConstants, SimKernel=s.SimKernel, SimLogger=None,
                                         SimParticles=p.copy(), SimViscosity=s.SimViscosity, SimDensityDiffusion=s.SimDensityDiffusion,
                                         backend_factory=_StandIn, on_output=lambda m, pp, *extra: got.append((m.Iteration, extra)), **kw)
        return steps, got, _StandIn.instances[0]

    steps, got, eng = run(field_grid=lattice)
    assert len(got) == len(steps) + 1 >= 3
    assert got[0] == (0, (None,))                                                  # the call before the first step: nothing to sample yet
    for iteration, extra in got[1:]:
        assert len(extra) == 1 and extra[0]["weight"].shape == (9, 12) and extra[0]["velocity"].shape == (9, 12, 3)
        assert (extra[0]["weight"] == iteration).all()                              # sampled on the state of THIS output
        assert extra[0]["lattice"] == ((0.05, 0.01), (0.1, 0.05), (12, 9))
    # one sample per output, each between the advance and the download of that output
    seq = [e for e in eng.log if isinstance(e, tuple)]
    assert [e[0] for e in seq] == ["advance", "sample_grid", "download"] * len(steps)
    # behind the group forces when those are on; the default changes nothing
    steps2, got2, _ = run(group_forces=[1, 2], field_grid=lattice)
    assert all(len(extra) == 2 for _, extra in got2) and got2[0][1][1] is None
    assert got2[1][1][0][3].shape == (3, 2, 3) and got2[1][1][1]["weight"].shape == (9, 12)
    steps3, got3, eng3 = run()
    assert all(extra == () for _, extra in got3) and not any(e[0] == "sample_grid" for e in eng3.log if isinstance(e, tuple))


def test_the_kernel_is_built_for_gfx950_without_scratch(tmp_path):
    """The library builds with hipcc --offload-arch=gfx950 and exports the entry point; the code object's metadata — read the way
    tests/test_bench_contract.py reads it — shows the four instantiations of k_field_grid without scratch, with LDS for four
    workgroups per compute unit (160 KiB) and registers for four waves per SIMD (512 / 4)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_report
    from sphexample_amd import build
    lib = build.build()
    assert hasattr(C.CDLL(lib), "sphmi_sample_grid")
    co = isa_report.code_object(lib, str(tmp_path))
    meta = isa_report.metadata(co)
    names = isa_report.demangle(list(meta))
    mine = {names[k]: v for k, v in meta.items() if "k_field_grid" in names[k]}
    assert len(mine) == 4, sorted(mine)
    assert {("<float, 2>" in d, "<double, 3>" in d) for d in mine} >= {(True, False), (False, True)}
    for d, v in mine.items():
        assert v["scratch_bytes"] == 0, (d, v)
        assert 4 * v["lds_bytes"] <= 160 * 1024, (d, v)
        assert v["vgprs"] + v["agprs"] <= 128, (d, v)
        assert v["max_flat_workgroup_size"] == 256, (d, v)
    outlined = [d for k, d in isa_report.demangle(list(isa_report.kernels(co))).items() if k not in meta]
    assert not outlined, outlined[:4]
