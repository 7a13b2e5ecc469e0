"""Host side of the neighbour list (sphmi_neighbors_build / _read / _release, csrc/sphmi_neighbor_list.h): the prototypes and
their binding, what the built code object says about the two kernels, the reference enumeration `brute_force_neighbors` pinned on a
regular lattice, the helpers of sphexample_amd/neighbors.py on hand-made CSR, and the RunSimulation plumbing with a stand-in
backend.  No GPU.

    row i lists every row j != i with r^2 = ((dx^2 + dy^2) + dz^2) <= H^2, ascending in j; HALF keeps j > i
"""
import copy
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from sphexample_amd import _abi, neighbors
from test_field_grid_host import _backend, _header, _prototype, _StandIn
from test_particle_fields_host import lattice_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference ------------------------------------------------------------------------------------------------------
def brute_force_neighbors(cfg, pos, targets=None, chunk=128, half=False):
    """Every target row against every row in fp64: (offsets int64 [M + 1], neighbors int32) of the rows `targets` (default: all),
    each list ascending in j.  r^2 is formed per axis, term by term, as the header states it.  Never calls the code under test."""
    X = np.asarray(pos, np.float64)
    N, D = X.shape
    idx = np.arange(N) if targets is None else np.asarray(targets, dtype=np.int64)
    counts, lists = np.zeros(len(idx), np.int64), []
    for a0 in range(0, len(idx), chunk):
        rows = idx[a0:a0 + chunk]
        d = [X[rows, c][:, None] - X[None, :, c] for c in range(D)]                 # x_i - x_j per axis, [m, N]
        r2 = d[0] * d[0] + d[1] * d[1]
        if D == 3:
            r2 = r2 + d[2] * d[2]
        sel = r2 <= cfg.H2
        j = np.arange(N)[None, :]
        sel &= (j > rows[:, None]) if half else (j != rows[:, None])
        a, jj = np.nonzero(sel)                                                     # row-major: per target ascending in j
        counts[a0:a0 + len(rows)] = np.bincount(a, minlength=len(rows))
        lists.append(jj.astype(np.int32))
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return offsets, (np.concatenate(lists) if lists else np.zeros(0, np.int32))


# ---- 1. the prototypes and the binding --------------------------------------------------------------------------------------
def test_header_and_binding_agree():
    text = _header()
    assert re.search(r"#define\s+SPHMI_ABI_VERSION\s+5\b", text) and _abi.ABI_VERSION == 5      # append-only: the version stays
    m = re.search(r"enum\s*\{\s*SPHMI_NEIGHBORS_FULL\s*=\s*(\d+)\s*,\s*SPHMI_NEIGHBORS_HALF\s*=\s*(\d+)\s*\}", text)
    assert m and (int(m.group(1)), int(m.group(2))) == (_abi.NEIGHBORS_FULL, _abi.NEIGHBORS_HALF) == (0, 1)
    assert _prototype("sphmi_neighbors_build") == ["sphmi_handle*", "int32_t", "int64_t*", "int64_t*"]
    assert _prototype("sphmi_neighbors_read") == ["sphmi_handle*", "int64_t*", "int32_t*"]
    assert _prototype("sphmi_neighbors_release") == ["sphmi_handle*"]
    b = _backend(3)
    assert b.has_neighbor_list()
    off, nbr = b.neighbor_list()
    fns = b._lib.fns
    assert fns["sphmi_neighbors_build"].argtypes == [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    assert fns["sphmi_neighbors_read"].argtypes == [C.c_void_p] * 3 and fns["sphmi_neighbors_release"].argtypes == [C.c_void_p]
    assert [len(fns[f"sphmi_neighbors_{k}"].calls) for k in ("build", "read", "release")] == [1, 1, 1]
    assert fns["sphmi_neighbors_build"].calls[0][1] == 0
    assert off.dtype == np.int64 and nbr.dtype == np.int32 and off.shape == (1,) and nbr.shape == (0,)       # (the recorder reports no rows)
    b.neighbor_list(half=True)
    assert fns["sphmi_neighbors_build"].calls[1][1] == 1
    # the pieces for callers who keep the result on the device; either array of a read may be left out
    b.neighbors_build()
    off, nbr = b.neighbors_read(neighbors=False)
    assert nbr is None and off is not None and fns["sphmi_neighbors_read"].calls[-1][2] is None
    off, nbr = b.neighbors_read(offsets=False)
    assert off is None and fns["sphmi_neighbors_read"].calls[-1][1] is None
    b.neighbors_release()
    assert len(fns["sphmi_neighbors_release"].calls) == 3


# ---- 2. the library ----------------------------------------------------------------------------------------------------------
def test_the_kernels_are_built_for_gfx950_without_scratch(tmp_path):
    """The library exports the three entry points; the code object's metadata — read the way tests/test_bench_contract.py reads it —
    shows the four instantiations of k_neighbor_count and of k_neighbor_fill without scratch, with LDS within the budget the header
    states (kNlLdsBytes, four workgroups per compute unit like k_particle_fields) and registers for four waves per SIMD."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_report
    from sphexample_amd import build
    lib = build.build()
    dll = C.CDLL(lib)
    assert all(hasattr(dll, f"sphmi_neighbors_{k}") for k in ("build", "read", "release"))
    src = open(os.path.join(ROOT, "sphexample_amd", "csrc", "sphmi_neighbor_list.h")).read()
    assert re.search(r"kNlLdsBytes = 2 \* \(size_t\)kNlThreads \* kNlRow \* 8 \+ 2 \* \(size_t\)kNlThreads \* 4 \+ 4 \* 6 \* 8 \+ 64;", src)
    assert re.search(r"constexpr int kNlThreads = 256;", src) and re.search(r"constexpr int kNlRow = 4;", src)
    lds = 2 * 256 * 4 * 8 + 2 * 256 * 4 + 4 * 6 * 8 + 64                            # kNlLdsBytes: 32-byte staged rows, half of k_particle_fields'
    budget = {"k_neighbor_count": lds, "k_neighbor_fill": lds}
    assert 4 * lds <= 160 * 1024
    co = isa_report.code_object(lib, str(tmp_path))
    meta = isa_report.metadata(co)
    names = isa_report.demangle(list(meta))
    for kernel, lds in budget.items():
        mine = {names[k]: v for k, v in meta.items() if kernel + "<" in names[k]}
        assert len(mine) == 4, (kernel, sorted(mine))
        assert {("<float, 2>" in d, "<double, 3>" in d) for d in mine} >= {(True, False), (False, True)}
        for d, v in mine.items():
            assert v["scratch_bytes"] == 0, (d, v)
            assert v["lds_bytes"] <= lds, (d, v, lds)
            assert v["vgprs"] + v["agprs"] <= 128, (d, v)
            assert v["max_flat_workgroup_size"] == 256, (d, v)
    scan = {names[k]: v for k, v in meta.items() if "k_nl_" in names[k]}
    assert len(scan) == 3 and all(v["scratch_bytes"] == 0 for v in scan.values()), scan


# ---- 3. the enumeration on a regular lattice ---------------------------------------------------------------------------------
@pytest.mark.parametrize("D,n", [(2, 21), (3, 13)])
def test_the_enumeration_counts_the_lattice_offsets_within_H(D, n):
    """On an n^D lattice the interior rows have as many neighbours as there are integer offsets o != 0 with |o|^2 dp^2 <= H^2,
    counted here from the integers alone (H^2 / dp^2 = 4 · 1.44 · D is not an integer: no offset sits at the cut)."""
    cfg, X, _, _, centre, _, _ = lattice_case(D, n)
    bound = 4 * 1.44 * D                                                            # (H / dp)^2
    reach = int(np.floor(np.sqrt(bound)))
    o = np.stack(np.meshgrid(*[np.arange(-reach, reach + 1)] * D, indexing="ij"), -1).reshape(-1, D)
    q = (o * o).sum(1)
    assert abs(bound - round(bound)) > 1e-3
    want = int(((q <= bound) & (q > 0)).sum())
    assert want == {2: 36, 3: 304}[D]
    off, nbr = brute_force_neighbors(cfg, X)
    cnt = np.diff(off)
    idx = np.stack(np.unravel_index(np.arange(len(X)), (n,) * D), -1)
    interior = ((idx >= reach) & (idx < n - reach)).all(1)
    assert interior[centre] and (cnt[interior] == want).all() and (cnt[~interior] < want).all()
    assert off[0] == 0 and off[-1] == len(nbr) and nbr.dtype == np.int32 and off.dtype == np.int64
    assert neighbors.symmetric(off, nbr)
    i, j = neighbors.pairs(off, nbr)
    assert (i != j).all() and all((np.diff(nbr[off[k]:off[k + 1]]) > 0).all() for k in range(len(X)))
    # the offsets of the centre row's entries are exactly the integer offsets within the bound
    got = np.round((X[nbr[off[centre]:off[centre + 1]]] - X[centre]) / 0.02).astype(int)
    assert sorted(map(tuple, got)) == sorted(map(tuple, o[(q <= bound) & (q > 0)]))
    # a subset of targets is the same rows; HALF is FULL filtered to j > i
    some = [0, centre, len(X) - 1]
    o2, n2 = brute_force_neighbors(cfg, X, targets=some)
    for k, r in enumerate(some):
        np.testing.assert_array_equal(n2[o2[k]:o2[k + 1]], nbr[off[r]:off[r + 1]])
    oh, nh = brute_force_neighbors(cfg, X, half=True)
    np.testing.assert_array_equal(nh, nbr[j > i])
    assert 2 * len(nh) == len(nbr) and not neighbors.symmetric(oh, nh)
    # a coincident row is listed, by both
    X2 = np.concatenate([X, X[centre:centre + 1]])
    o3, n3 = brute_force_neighbors(cfg, X2, targets=[centre, len(X)])
    assert o3[1] == want + 1 and n3[o3[1] - 1] == len(X) and o3[2] - o3[1] == want + 1 and centre in n3[o3[1]:]


# ---- 4. the helpers on hand-made CSR ----------------------------------------------------------------------------------------------
def test_pairs_pair_sum_and_symmetric_on_hand_made_csr():
    #        row 0: 1, 3     row 1: 0     row 2: (none)     row 3: 0     row 4: (none)
    off, nbr = np.array([0, 2, 3, 3, 4, 4]), np.array([1, 3, 0, 0], dtype=np.int32)
    i, j = neighbors.pairs(off, nbr)
    assert i.tolist() == [0, 0, 1, 3] and j.tolist() == [1, 3, 0, 0] and i.dtype == j.dtype == np.int64
    assert neighbors.symmetric(off, nbr)
    s = neighbors.pair_sum(off, np.array([1.0, 2.0, 4.0, 8.0]))
    assert s.tolist() == [3.0, 4.0, 0.0, 8.0, 0.0] and s.dtype == np.float64         # rows without entries: zero, and their neighbours intact
    v = neighbors.pair_sum(off, np.array([[1.0, 10.0], [2.0, 20.0], [4.0, 40.0], [8.0, 80.0]]))
    assert v.tolist() == [[3.0, 30.0], [4.0, 40.0], [0.0, 0.0], [8.0, 80.0], [0.0, 0.0]]
    assert neighbors.pair_sum(off, np.ones(4, dtype=np.int64)).tolist() == [2, 1, 0, 1, 0]      # the row lengths
    assert neighbors.pair_sum(off, np.ones(4, dtype=np.float32)).dtype == np.float64
    # leading and trailing empty rows
    off2 = np.array([0, 0, 0, 2, 2])
    assert neighbors.pair_sum(off2, np.array([5.0, 6.0])).tolist() == [0.0, 0.0, 11.0, 0.0]
    assert neighbors.pairs(off2, np.array([3, 3]))[0].tolist() == [2, 2]
    # not symmetric: a half list, an entry without its mirror
    assert not neighbors.symmetric(np.array([0, 1, 1]), np.array([1]))
    assert not neighbors.symmetric(np.array([0, 1, 2, 2]), np.array([1, 2]))
    assert not neighbors.symmetric(np.array([0, 1]), np.array([7]))                 # an entry that is no row
    # an empty list, and no rows at all
    e_off, e_nbr = np.zeros(4, np.int64), np.zeros(0, np.int32)
    i, j = neighbors.pairs(e_off, e_nbr)
    assert len(i) == len(j) == 0 and neighbors.symmetric(e_off, e_nbr)
    assert neighbors.pair_sum(e_off, np.zeros(0)).tolist() == [0.0, 0.0, 0.0]
    assert neighbors.pair_sum(np.array([0]), np.zeros(0)).shape == (0,) and neighbors.symmetric(np.array([0]), e_nbr)
    for bad in (lambda: neighbors.pairs(np.array([0, 2]), np.array([1])), lambda: neighbors.pair_sum(off, np.ones(3)),
                lambda: neighbors.pairs(np.array([1, 2]), np.array([0, 0])), lambda: neighbors.pairs(np.array([0, 2, 1]), np.array([0]))):
        with pytest.raises(ValueError):
            bad()


# ---- 5. RunSimulation ----------------------------------------------------------------------------------------------------------------
class _ListStandIn(_StandIn):
    def neighbor_list(self, half=False):
        self.log.append(("neighbor_list", self.iteration))
        return np.array([0, 1, 2], dtype=np.int64), np.array([1, 0], dtype=np.int32) + 0 * self.iteration, self.iteration

    def particle_fields(self, fields):
        self.log.append(("particle_fields", self.iteration))
        return {k: np.zeros(2) for k in fields}


def test_run_simulation_hands_the_list_to_the_callback():
    from conftest import load_dam_break_2d
    from sphexample_amd import simulation
    p, s = load_dam_break_2d()

    def run(**kw):
        meta = copy.deepcopy(s.SimMetaData)
        meta.SimulationTime, meta.OutputTimes = 0.002, 0.001
        got = []
        _StandIn.instances.clear()
        steps = simulation.RunSimulation(SimGeometry=None, SimMetaData=meta, SimConstants=s.SimConstants, SimKernel=s.SimKernel, SimLogger=None,
                                         SimParticles=p.copy(), SimViscosity=s.SimViscosity, SimDensityDiffusion=s.SimDensityDiffusion,
                                         backend_factory=_ListStandIn, on_output=lambda m, pp, *extra: got.append((m.Iteration, extra)), **kw)
        return steps, got, _StandIn.instances[0]

    steps, got, eng = run(neighbor_list=True)
    assert len(got) == len(steps) + 1 >= 3
    assert got[0] == (0, (None,))                                                  # the call before the first step: no cell list yet
    for iteration, extra in got[1:]:
        assert len(extra) == 1
        off, nbr, taken_at = extra[0]                                               # what the backend returned, untouched
        assert off.tolist() == [0, 1, 2] and nbr.tolist() == [1, 0] and taken_at == iteration      # built on the rows of THIS output
    seq = [e for e in eng.log if isinstance(e, tuple)]
    assert [e[0] for e in seq] == ["advance", "neighbor_list", "download"] * len(steps)      # no step between the list and the download
    # behind the differential fields when those are on
    _, got2, eng2 = run(particle_fields=("div_r",), neighbor_list=True)
    assert all(len(extra) == 2 for _, extra in got2) and got2[0][1] == (None, None)
    assert set(got2[1][1][0]) == {"div_r"} and got2[1][1][1][0].tolist() == [0, 1, 2]
    assert [e[0] for e in eng2.log if isinstance(e, tuple)][:4] == ["advance", "particle_fields", "neighbor_list", "download"]
    # without the keyword the callback keeps its arguments and nothing is built
    _, got3, eng3 = run()
    assert all(extra == () for _, extra in got3) and not any(e[0] == "neighbor_list" for e in eng3.log if isinstance(e, tuple))
