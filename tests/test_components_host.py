"""Host side of the connected bodies (sphmi_components_build / _read / _release, csrc/sphmi_components.h): the prototypes and their
binding, the Julia shim's calls, the numpy restatement sphexample_amd.components on hand-made graphs and against an independent
connected-components search (scipy's when it imports, else a plain union–find here), the droplet helpers, the RunSimulation
plumbing with a stand-in backend, and what the built code object says about the kernels.  No GPU.

Every comparison is exact: integers and bytes."""
import copy
import ctypes as C
import os
import re
import sys
import types

import numpy as np
import pytest

from sphexample_amd import _abi, components
from test_field_grid_host import _backend, _header, _prototype, _StandIn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the prototypes and the binding ------------------------------------------------------------------------------------------
def test_header_and_binding_agree():
    text = _header()
    assert re.search(r"#define\s+SPHMI_ABI_VERSION\s+5\b", text) and _abi.ABI_VERSION == 5      # append-only: the version stays
    assert _prototype("sphmi_components_build") == ["sphmi_handle*", "double", "uint32_t", "int64_t*", "int64_t*"]
    assert _prototype("sphmi_components_read") == ["sphmi_handle*", "int32_t*", "int32_t*", "int32_t*", "double*"]
    assert _prototype("sphmi_components_release") == ["sphmi_handle*"]
    b = _backend(2)
    b.cfg = types.SimpleNamespace(H=0.25)
    assert b.has_components()
    got = b.components()
    fns = b._lib.fns
    assert fns["sphmi_components_build"].argtypes == [C.c_void_p, C.c_double, C.c_uint32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    assert fns["sphmi_components_read"].argtypes == [C.c_void_p] * 5 and fns["sphmi_components_release"].argtypes == [C.c_void_p]
    assert [len(fns[f"sphmi_components_{k}"].calls) for k in ("build", "read", "release")] == [1, 1, 1]
    assert fns["sphmi_components_build"].calls[0][1:3] == (0.25, 1 << 1)             # link=None is H; the fluid
    assert list(got) == ["label", "first_row", "count", "box"]
    assert [got[k].dtype for k in got] == [np.int32, np.int32, np.int32, np.float64] and got["box"].shape == (0, 6) and got["label"].shape == (0,)
    b.components_build(0.125, types=("Fluid", "Fixed", "Moving"))
    assert fns["sphmi_components_build"].calls[1][1:3] == (0.125, 0b1110)
    b.components_build(0.125, types=(2, "Moving"))
    assert fns["sphmi_components_build"].calls[2][2] == 0b1100
    lab, first, cnt, box = b.components_read(first_row=False, box=False)             # any array of a read may be left out
    assert first is None and box is None and lab is not None and cnt is not None
    assert [a is None for a in fns["sphmi_components_read"].calls[-1][1:]] == [False, True, False, True]
    b.components_release()
    with pytest.raises(RuntimeError, match="did not build"):                        # nothing of this object's is held any more
        b.components_read()
    with pytest.raises(ValueError):
        b.components_build(types=("Water",))


def test_the_julia_shim_calls_match_the_prototypes():
    """_read and _release go through `ccall(` and tests/test_julia_shim.py holds them; the build — the header's only uint32_t
    argument — goes through @ccall and is held here, argument by argument."""
    import test_julia_shim as tj
    calls = {c[0]: c for c in tj.shim_ccalls()}
    assert {"sphmi_components_read", "sphmi_components_release"} <= set(calls)
    m = re.search(r"@ccall\s+LIB\.sphmi_components_build\((.*?)\)::(\w+)\)", tj.shim_text())
    assert m, "components(...) does not call sphmi_components_build"
    jl = [a.split("::")[1].strip() for a in tj._split_top(m.group(1))]
    width = dict(tj.JL_WIDTH, UInt32=("i", 4))
    cls = lambda t: "ptr" if t.startswith(("Ptr{", "Ref{")) else "%s%d" % width[t]      # noqa: E731
    want = {"sphmi_handle*": "ptr", "double": "f8", "uint32_t": "i4", "int64_t*": "ptr"}
    assert m.group(2) == "Cint" and [cls(t) for t in jl] == [want[a] for a in _prototype("sphmi_components_build")]
    assert jl[2] == "UInt32"


# ---- 2. the numpy restatement -------------------------------------------------------------------------------------------------------
def _union_find(n, i, j, sel):
    """A plain union–find, nothing shared with the module: root[x] for selected rows, the minimum of the component."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in zip(i.tolist(), j.tolist()):
        if sel[a] and sel[b]:
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(x) for x in range(n)], dtype=np.int64)


def reference(position, sel, link):
    """(label, first_row, count, box) by enumeration and an independent search; labels canonicalised to ascending first row."""
    X = np.asarray(position, np.float64)
    n, D = X.shape
    sel = np.asarray(sel, bool)
    cut = float(link) * float(link)
    I, J = [], []
    for a in range(0, n, 1024):
        d = X[a:a + 1024, None, :] - X[None, :, :]
        r2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
        if D == 3:
            r2 = r2 + d[..., 2] * d[..., 2]
        ii, jj = np.nonzero(r2 <= cut)
        ii += a
        keep = (jj > ii) & sel[ii] & sel[jj]
        I.append(ii[keep]); J.append(jj[keep])
    I, J = np.concatenate(I), np.concatenate(J)
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        _, comp = connected_components(coo_matrix((np.ones(len(I), np.int8), (I, J)), shape=(n, n)), directed=False)
        first_of = np.full(comp.max(initial=-1) + 1, n, np.int64)
        np.minimum.at(first_of, comp[sel], np.flatnonzero(sel))
        root = first_of[comp]
    except ImportError:
        root = _union_find(n, I, J, sel)
    firsts = np.unique(root[sel])
    label = np.where(sel, np.searchsorted(firsts, root), -1).astype(np.int32)
    count = np.array([(label == c).sum() for c in range(len(firsts))], dtype=np.int32)
    box = np.zeros((len(firsts), 6))
    for c in range(len(firsts)):
        rows = X[label == c]
        box[c, :D], box[c, 3:3 + D] = rows.min(0), rows.max(0)
    return label, firsts.astype(np.int32), count, box


def _same(got, want, what=""):
    for k, w in zip(("label", "first_row", "count", "box"), want):
        assert got[k].dtype == w.dtype and got[k].shape == w.shape, (what, k)
        np.testing.assert_array_equal(got[k], w, err_msg=f"{what} {k}")


def _both(X, sel, link, what):
    """label() and from_pairs() on the module's own links against the reference."""
    X = np.asarray(X, np.float64)
    want = reference(X, sel, link)
    got = components.label(X, sel, link)
    _same(got, want, what)
    i, j = components.links(X, np.ones(len(X), bool), link)                        # ALL links: from_pairs drops the unselected ends
    again = components.from_pairs(len(X), j, i, sel, position=X)                   # (ends swapped: the order of a link does not matter)
    _same(again, want, what + " from_pairs")
    assert components.from_pairs(len(X), i, j, sel)["box"] is None
    return got


def test_hand_made_graphs():
    two = np.zeros((5, 2))
    got = _both(two, np.zeros(5, bool), 1.0, "empty selection")
    assert got["label"].tolist() == [-1] * 5 and len(got["first_row"]) == 0 and got["box"].shape == (0, 6)
    got = _both([[0.3, -0.7, 2.0]], [True], 0.1, "one row")
    assert got["label"].tolist() == [0] and got["count"].tolist() == [1] and got["box"].tolist() == [[0.3, -0.7, 2.0, 0.3, -0.7, 2.0]]
    got = _both([[0.5, 0.5], [9.0, 9.0], [0.5, 0.5]], [True] * 3, 1e-3, "coincident rows")
    assert got["label"].tolist() == [0, 1, 0] and got["first_row"].tolist() == [0, 1] and got["count"].tolist() == [2, 1]
    assert (got["box"][:, [2, 5]] == 0).all() and not np.signbit(got["box"][:, [2, 5]]).any()      # 2-D: exact zeros for z
    # a chain laid out from its far end: row 0 is the LAST particle of the line, so the minimum has to travel through all of it
    n = 40
    chain = np.stack([0.9 * np.arange(n)[::-1], np.zeros(n)], 1)
    order = np.r_[0, np.random.default_rng(3).permutation(np.arange(1, n))]
    got = _both(chain[order], [True] * n, 1.0, "chain")
    assert got["first_row"].tolist() == [0] and got["count"].tolist() == [n] and (got["label"] == 0).all()
    assert got["box"][0].tolist() == [0.0, 0.0, 0.0, 0.9 * (n - 1), 0.0, 0.0]
    # two blobs joined only through rows that are not selected
    blob = np.array([[0.0, 0.0], [0.5, 0.0], [0.0, 0.5]])
    bridge = np.stack([np.arange(1.0, 5.0, 0.8), np.zeros(5)], 1)
    X = np.concatenate([bridge[:2], blob, bridge[2:], blob + [5.0, 0.0]])
    sel = np.array([False] * 2 + [True] * 3 + [False] * 3 + [True] * 3)
    got = _both(X, sel, 0.9, "bridge")
    assert got["label"].tolist() == [-1, -1, 0, 0, 0, -1, -1, -1, 1, 1, 1] and got["first_row"].tolist() == [2, 8]
    assert _both(X, np.ones(len(X), bool), 0.9, "bridge selected")["count"].tolist() == [len(X)]
    for bad in (lambda: components.label(X, sel, 0.0), lambda: components.label(X, sel[:3], 1.0), lambda: components.from_pairs(3, [0], [3]),
                lambda: components.label(X, sel, np.inf), lambda: components.from_pairs(3, [0, 1], [1])):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.parametrize("D", [2, 3])
def test_random_clouds_against_the_independent_search(D):
    """Uniform clouds near the percolation threshold, where sizes spread widely; a third of the rows unselected."""
    rng = np.random.default_rng(11 + D)
    n = 1500
    X = rng.random((n, D))
    link = (4.5 / (n * np.pi)) ** 0.5 if D == 2 else (2.7 / (n * 4.0 / 3.0 * np.pi)) ** (1.0 / 3.0)
    for sel in (np.ones(n, bool), rng.random(n) > 0.33):
        got = _both(X, sel, link, f"cloud {D}-D")
        print(f"{D}-D: {len(got['count'])} components, largest {int(got['count'].max())} of {int(sel.sum())}")
        assert len(got["count"]) > 20 and got["count"].max() > 10 and got["count"].sum() == sel.sum()
    # a negative coordinate, a negative zero and a positive zero in one component: the box is taken on the order-preserving keys
    Y = np.array([[-0.0, 1.0], [0.0, 1.0], [-0.25, 1.0]])
    box = components.label(Y, [True] * 3, 1.0)["box"][0]
    assert box[0] == -0.25 and box[3] == 0.0 and not np.signbit(box[3])


# ---- 3. main body, droplets, the wave front ----------------------------------------------------------------------------------------
def test_helpers_with_one_droplet_ahead_of_the_bulk():
    bulk = np.stack(np.meshgrid(np.arange(4) * 0.1, np.arange(3) * 0.1, indexing="ij"), -1).reshape(-1, 2)      # 12 rows, x up to 0.3
    drop = np.array([[0.9, 0.5], [0.95, 0.5]])
    wall = np.array([[2.0, 0.0]])
    X = np.concatenate([drop[:1], bulk, wall, drop[1:]])
    sel = np.ones(len(X), bool); sel[13] = False
    V = np.zeros_like(X); V[:, 0] = 1.0; V[[0, 14]] = [[3.0, 1.0], [5.0, -1.0]]
    c = components.label(X, sel, 0.11)
    assert c["first_row"].tolist() == [0, 1] and c["count"].tolist() == [2, 12]      # the droplet holds the first row: it is component 0
    assert components.main_body(c["count"]) == 1
    mask = components.main_body_mask(c["label"], c["count"])
    assert mask.tolist() == [False] + [True] * 12 + [False, False]
    assert components.front_position(X, c["label"], c["count"]) == pytest.approx(0.3)
    assert X[sel, 0].max() == 0.95                                                  # … where the box of all the fluid says 0.95
    assert components.front_position(X, c["label"], c["count"], axis=1) == pytest.approx(0.2)
    assert components.front_position(X, c["label"], c["count"], side="min") == 0.0
    t = components.droplet_table(c["label"], c["count"], X, V, m0=0.5)
    assert t["main"] == 1 and t["count"].tolist() == [2, 12] and t["mass"].tolist() == [1.0, 6.0]
    np.testing.assert_allclose(t["centroid"], [[0.925, 0.5], [0.15, 0.1]], rtol=0, atol=1e-15)
    np.testing.assert_allclose(t["momentum"], [[4.0, 0.0], [6.0, 0.0]], rtol=0, atol=1e-15)
    assert components.main_body([3, 7, 7]) == 1                                     # the lowest number among equals
    for bad in (lambda: components.main_body([]), lambda: components.droplet_table(c["label"], c["count"][:1], X, V, 1.0),
                lambda: components.front_position(X, c["label"], c["count"], axis=2), lambda: components.droplet_table(c["label"], c["count"], X, V[:3], 1.0)):
        with pytest.raises(ValueError):
            bad()


# ---- 4. RunSimulation -------------------------------------------------------------------------------------------------------------------
class _BodiesStandIn(_StandIn):
    def isosurface(self, origin, spacing, counts, level=0.5, attributes=False):
        self.log.append(("isosurface", self.iteration))
        return "mesh"

    def components(self, link=None, types=("Fluid",)):
        self.log.append(("components", self.iteration))
        return {"label": np.full(4, self.iteration, np.int32), "asked": (link, tuple(types))}


def test_run_simulation_hands_the_components_to_the_callback():
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
                                         backend_factory=_BodiesStandIn, on_output=lambda m, pp, *extra: got.append((m.Iteration, extra)), **kw)
        return steps, got, _StandIn.instances[0]

    steps, got, eng = run(components=True)
    assert len(got) == len(steps) + 1 >= 3
    assert got[0] == (0, (None,))                                                  # the call before the first step: nothing to label yet
    for iteration, extra in got[1:]:
        assert len(extra) == 1 and (extra[0]["label"] == iteration).all()           # labelled on the state of THIS output
        assert extra[0]["asked"] == (None, ("Fluid",))
    assert [e[0] for e in eng.log if isinstance(e, tuple)] == ["advance", "components", "download"] * len(steps)
    # a link of the caller's; a link and types; behind the mesh when that is on
    _, got2, _ = run(components=0.004)
    assert got2[1][1][0]["asked"] == (0.004, ("Fluid",))
    lattice = ([0.05, 0.01], [0.1, 0.05], [12, 9])
    _, got3, eng3 = run(isosurface=lattice, components=(0.003, ("Fluid", "Moving")))
    assert got3[0][1] == (None, None) and got3[1][1][0] == "mesh" and got3[1][1][1]["asked"] == (0.003, ("Fluid", "Moving"))
    assert [e[0] for e in eng3.log if isinstance(e, tuple)][:4] == ["advance", "isosurface", "components", "download"]
    # without the keyword (or with False) the callback keeps its arguments and nothing is built
    for kw in ({}, {"components": False}, {"components": None}):
        _, got4, eng4 = run(**kw)
        assert all(extra == () for _, extra in got4) and not any(e[0] == "components" for e in eng4.log if isinstance(e, tuple))


# ---- 5. the library ---------------------------------------------------------------------------------------------------------------------
def test_the_kernels_are_built_for_gfx950_without_scratch(tmp_path):
    """The library exports the three entry points; the code object's metadata — read the way tests/test_bench_contract.py reads it —
    shows every kernel of csrc/sphmi_components.h without scratch, the hook once per (precision, dimension) with exactly the LDS
    of k_neighbor_count (nl_walk's, four workgroups per compute unit) and no device function left outside a kernel; the scan
    kernels are the neighbour list's three, not copies."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_report
    from sphexample_amd import build
    assert "sphmi_components.h" in build.HEADERS
    lib = build.build()
    dll = C.CDLL(lib)
    assert all(hasattr(dll, f"sphmi_components_{k}") for k in ("build", "read", "release"))
    co = isa_report.code_object(lib, str(tmp_path))
    meta = isa_report.metadata(co)
    names = isa_report.demangle(list(meta))
    mine = {names[k]: v for k, v in meta.items() if "k_cc_" in names[k]}
    per_kernel = {}
    for d in mine:
        per_kernel.setdefault(re.search(r"k_cc_\w+", d).group(0), []).append(d)
    assert {k: len(v) for k, v in per_kernel.items()} == {"k_cc_init": 1, "k_cc_hook": 4, "k_cc_flatten": 1, "k_cc_label": 1, "k_cc_table_init": 1,
                                                          "k_cc_table": 4, "k_cc_box_decode": 2}, per_kernel
    count_lds = {v["lds_bytes"] for k, v in meta.items() if "k_neighbor_count<" in names[k]}
    assert len(count_lds) == 1
    for d, v in mine.items():
        assert v["scratch_bytes"] == 0, (d, v)
        assert v["max_flat_workgroup_size"] == 256, (d, v)
        if "k_cc_hook" in d:
            assert {v["lds_bytes"]} == count_lds and 4 * v["lds_bytes"] <= 160 * 1024, (d, v)
            assert v["vgprs"] + v["agprs"] <= 128, (d, v)                            # four workgroups of four waves per compute unit
        else:
            assert v["lds_bytes"] == 0, (d, v)
    assert {("float" in d, "2>" in d) for d in per_kernel["k_cc_hook"]} == {(a, b) for a in (True, False) for b in (True, False)}
    assert len([k for k in meta if "k_nl_" in names[k]]) == 3
    outlined = [d for k, d in isa_report.demangle(list(isa_report.kernels(co))).items() if k not in meta]
    assert not outlined, outlined[:4]
    text = re.sub(r"//.*", "", open(os.path.join(ROOT, "sphexample_amd", "csrc", "sphmi_components.h")).read())
    assert "always_inline" in text and "nl_walk<T, D>(A, i, has_row" in text and "__global__ void __launch_bounds__(kNlThreads, 4) k_cc_hook" in text
