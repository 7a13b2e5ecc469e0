"""Host side of the free-surface mesh (sphmi_isosurface_build / _read / _release, csrc/sphmi_isosurface.h, csrc/sphmi_iso_core.h):
the prototypes and their binding; the stand-alone host program tests/host_isosurface/iso_main.cpp — the per-node functions the
kernels call, run in a loop, built with the address and undefined-behaviour sanitizers where their runtime links — against the
numpy restatement sphexample_amd.isosurface.extract, byte for byte; the topology and the bounds of the meshes of analytic fields;
the swap table; the RunSimulation plumbing with a stand-in backend; what the built code object says about the kernels.  No GPU.

Every comparison is exact — bytes, integers — or a bound derived from the lattice."""
import copy
import ctypes as C
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

from sphexample_amd import _abi, isosurface
from test_field_grid_host import _backend, _header, _prototype, _StandIn
from test_step_series_host import SANITIZE, host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sphexample_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "host_isosurface", "iso_main.cpp")
IRR = np.array([0.0318309886, 0.0577215665, 0.0693147181])          # nothing a lattice of spacing 1/11 knows


# ---- 1. the prototypes and the binding --------------------------------------------------------------------------------------
def test_header_and_binding_agree():
    text = _header()
    assert re.search(r"#define\s+SPHMI_ABI_VERSION\s+5\b", text) and _abi.ABI_VERSION == 5      # append-only: the version stays
    assert _prototype("sphmi_isosurface_build") == ["sphmi_handle*", "const double*", "const double*", "const int64_t*", "double", "int64_t*", "int64_t*"]
    assert _prototype("sphmi_isosurface_read") == ["sphmi_handle*", "double*", "int32_t*", "double*", "double*"]
    assert _prototype("sphmi_isosurface_release") == ["sphmi_handle*"]
    b = _backend(3)
    assert b.has_isosurface()
    got = b.isosurface([0.1, 0.2, 0.3], [0.5, 0.25, 0.125], [4, 3, 2])
    fns = b._lib.fns
    assert fns["sphmi_isosurface_build"].argtypes == [C.c_void_p] * 4 + [C.c_double, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    assert fns["sphmi_isosurface_read"].argtypes == [C.c_void_p] * 5 and fns["sphmi_isosurface_release"].argtypes == [C.c_void_p]
    assert [len(fns[f"sphmi_isosurface_{k}"].calls) for k in ("build", "read", "release")] == [1, 1, 1]
    assert fns["sphmi_isosurface_build"].calls[0][4] == 0.5                         # the default level
    assert len(got) == 2 and got[0].shape == (0, 3) and got[0].dtype == np.float64 and got[1].shape == (0, 3) and got[1].dtype == np.int32
    assert [a is None for a in fns["sphmi_isosurface_read"].calls[0][1:]] == [False, False, True, True]      # no attributes asked for
    b2 = _backend(2)
    v, e, p, u = b2.isosurface([0.0, 0.0], [1.0, 1.0], [5, 7], level=0.25, attributes=True)
    assert b2._lib.fns["sphmi_isosurface_build"].calls[0][4] == 0.25
    assert v.shape == (0, 3) and e.shape == (0, 2) and p.shape == (0,) and u.shape == (0, 3)
    assert not any(a is None for a in b2._lib.fns["sphmi_isosurface_read"].calls[0][1:])
    # the pieces, for callers who keep the mesh on the device; any array of a read may be left out
    b2.isosurface_build([0.0, 0.0], [1.0, 1.0], [5, 7])
    v, e, p, u = b2.isosurface_read(vertices=False, pressure=True)
    assert v is None and u is None and e is not None and p is not None
    b2.isosurface_release()
    with pytest.raises(ValueError):
        b2.isosurface_build([0.0], [1.0, 1.0], [5, 7])


# ---- 2. the host program against the numpy restatement ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def iso_main(tmp_path_factory):
    cxx = host_compiler()
    exe = str(tmp_path_factory.mktemp("iso") / "iso_main")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I", CSRC, MAIN, "-o", exe]
    for extra in (SANITIZE + ("-static-libasan", "-static-libubsan"), SANITIZE, ()):
        built = subprocess.run(base + list(extra), capture_output=True, text=True)
        if built.returncode == 0:
            break
    assert built.returncode == 0, built.stderr
    print("sanitizers:", " ".join(extra) or "none")
    return exe


def test_the_core_header_is_host_only():
    text = open(os.path.join(CSRC, "sphmi_iso_core.h")).read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert not [i for i in includes if "hip" in i or i.startswith('"')], includes
    main = [ln.split()[1] for ln in open(MAIN).read().splitlines() if ln.startswith("#include")]
    assert [i for i in main if i.startswith('"')] == ['"sphmi_iso_core.h"']
    kernels = open(os.path.join(CSRC, "sphmi_isosurface.h")).read()
    assert '#include "sphmi_iso_core.h"' in kernels and '#include "sphmi_neighbor_list.h"' not in kernels
    assert "k_nl_" not in re.sub(r"//.*", "", kernels)                              # the scan kernels are used, not copied


def _nodes(counts, origin, spacing):
    from sphexample_amd.fields import grid_nodes
    return grid_nodes(origin, spacing, counts)


def _ramp(signed_distance, width):
    """1 in the fluid, 1/2 where the distance is 0, 0 in air — and EXACT zeros beyond the ramp, as the sampler's empty space."""
    return np.clip(0.5 + signed_distance / width, 0.0, 1.0)


def _lattice(D, n=12):
    counts = (n,) * D
    return counts, IRR[:D] - 0.5, np.full(D, 1.0 / (n - 1)) * np.array([1.0, 1.03, 0.97])[:D]


SPHERE_R, TORUS_R, TORUS_r, CIRCLE_R = 0.33, 0.29, 0.13, 0.31
PLANE_N, PLANE_C = np.array([0.31, 0.47, 0.83]), 0.6180339887


def _field(name):
    """name → (counts, origin, spacing, level, S [nodes])."""
    if name in ("sphere", "torus", "plane", "at_level"):
        counts, origin, spacing = _lattice(3)
        X = _nodes(counts, origin, spacing)
        if name == "torus":
            S = _ramp(TORUS_r - np.sqrt((np.sqrt(X[:, 0] ** 2 + X[:, 1] ** 2) - TORUS_R) ** 2 + X[:, 2] ** 2), 0.11)
        elif name == "plane":
            XL = X.astype(np.longdouble)                                            # the samples rounded ONCE: half an ulp each
            S = (np.longdouble(PLANE_C) - (XL * PLANE_N.astype(np.longdouble)).sum(1)).astype(np.float64)
        else:
            S = _ramp(SPHERE_R - np.sqrt((X ** 2).sum(1)), 0.11)
        if name == "at_level":
            k = int(np.argmin(np.abs(np.sqrt((X ** 2).sum(1)) - SPHERE_R)))          # the node nearest the surface: interior to the lattice
            S[k] = 0.5
        return counts, origin, spacing, 0.5, S
    if name == "circle":
        counts, origin, spacing = _lattice(2)
        X = _nodes(counts, origin, spacing)
        return counts, origin, spacing, 0.5, _ramp(CIRCLE_R - np.sqrt((X ** 2).sum(1)), 0.11)
    if name in ("one_cell_3d", "one_cell_2d"):
        D = 3 if name.endswith("3d") else 2
        counts, origin, spacing = (2,) * D, IRR[:D], np.array([0.07, 0.05, 0.09])[:D]
        S = np.array([0.9, 0.7, 0.2, 0.6, 0.1, 0.55, 0.0, 0.3])[:2 ** D]
        return counts, origin, spacing, 0.5, S
    if name == "flat":                                                              # a count of 1 along y: no cells
        counts, origin, spacing = (12, 1, 12), IRR - np.array([0.5, 0.0, 0.5]), np.full(3, 1.0 / 11)      # the plane y = const runs through the sphere
        X = _nodes(counts, origin, spacing)
        return counts, origin, spacing, 0.5, _ramp(SPHERE_R - np.sqrt((X ** 2).sum(1)), 0.11)
    raise KeyError(name)


def _sums(counts, origin, spacing, S):
    """The raw sums a sampler would leave next to S: n (exact zeros where S is zero), SP, Srho, Sv of smooth fields."""
    X = np.zeros((S.size, 3))
    X[:, :len(counts)] = _nodes(counts, origin, spacing)
    n = np.where(S > 0, np.ceil(np.abs(S) * 20.0), 0.0)
    P = 9810.0 * (0.7 - X[:, -1 if len(counts) == 3 else 1]) + 13.0 * X[:, 0]
    V = np.stack([0.3 + X[:, 1], -X[:, 0] * 1.7, 0.1 * X[:, 2] + X[:, 0] * X[:, 1]], 1)
    return np.stack([S, S * P, S * 1000.0, S * V[:, 0], S * V[:, 1], S * V[:, 2], n])


def _means(sums):
    S, n = sums[0], sums[6]
    some = (n > 0) & (S > 0)
    with np.errstate(all="ignore"):
        mean = lambda a: np.where(some, a / S, 0.0)                                 # noqa: E731 — one IEEE division, as the library's
        return mean(sums[1]), np.stack([mean(sums[3]), mean(sums[4]), mean(sums[5])], 1), n.astype(np.int64)


def _run_host(exe, tmp_path, counts, origin, spacing, level, sums):
    D = len(counts)
    c3, o3, s3 = list(counts) + [1] * (3 - D), list(origin) + [0.0] * (3 - D), list(spacing) + [1.0] * (3 - D)
    src, dst = str(tmp_path / "lattice.bin"), str(tmp_path / "mesh.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<4q", D, *c3) + struct.pack("<7d", *o3, *s3, level) + np.ascontiguousarray(sums, dtype=np.float64).tobytes())
    run = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip().splitlines()[-1] == "ok", run.stdout + run.stderr
    assert not run.stderr.strip(), run.stderr                                       # a sanitizer report would be here
    raw = open(dst, "rb").read()
    nv, ne, dims = struct.unpack("<3q", raw[:24])
    assert dims == D
    at = 24
    out = []
    for shape, dtype in (((nv, 3), np.float64), ((ne, D), np.int32), ((nv,), np.float64), ((nv, 3), np.float64)):
        size = int(np.prod(shape)) * np.dtype(dtype).itemsize
        out.append(np.frombuffer(raw[at:at + size], dtype=dtype).reshape(shape))
        at += size
    assert at == len(raw)
    return out


_MESHES = {}


def _both(name, exe, tmp_path):
    """(host program's mesh, numpy's mesh, the field) of a named case, each computed once."""
    if name not in _MESHES:
        counts, origin, spacing, level, S = _field(name)
        sums = _sums(counts, origin, spacing, S)
        P, V, n = _means(sums)
        shape = tuple(counts)[::-1]
        ref = isosurface.extract(S.reshape(shape), origin, spacing, level, pressure=P.reshape(shape), velocity=V.reshape(shape + (3,)), count=n.reshape(shape))
        got = _run_host(exe, tmp_path, counts, origin, spacing, level, sums)
        _MESHES[name] = (got, ref, (counts, origin, spacing, level, S, n))
    return _MESHES[name]


CASES = ("sphere", "torus", "circle", "plane", "one_cell_3d", "one_cell_2d", "flat", "at_level")


@pytest.mark.parametrize("name", CASES)
def test_host_program_equals_the_numpy_restatement(name, iso_main, tmp_path):
    got, ref, (counts, origin, spacing, level, S, n) = _both(name, iso_main, tmp_path)
    D = len(counts)
    print(f"{name}: lattice {counts}, {len(ref[0])} vertices, {len(ref[1])} elements")
    assert ref[0].dtype == np.float64 and ref[1].dtype == np.int32 and ref[0].shape[1] == 3 and ref[1].shape[1] == D
    for a, b, what in zip(got, ref, ("vertices", "elements", "pressure", "velocity")):
        assert a.shape == b.shape and a.dtype == b.dtype, what
        assert a.tobytes() == b.tobytes(), what
    if D == 2:
        assert (ref[0][:, 2] == 0).all() and not np.signbit(ref[0][:, 2]).any()
    if name == "flat":
        assert len(ref[0]) == 0 and len(ref[1]) == 0 and (S >= level).any() and (S < level).any()
    else:
        assert len(ref[0]) > 0 and len(ref[1]) > 0 and ref[1].min() == 0 and ref[1].max() == len(ref[0]) - 1
    if name in ("sphere", "torus", "circle"):
        # the rule for ends without rows is exercised: crossing edges whose low end is an exact zero of S (n == 0)
        plain = isosurface.extract(S.reshape(tuple(counts)[::-1]), origin, spacing, level, pressure=_means(_sums(counts, origin, spacing, S))[0].reshape(tuple(counts)[::-1]))
        assert (plain[2] != ref[2]).sum() > 10
    if name == "at_level":
        X = _nodes(counts, origin, spacing)
        k = int(np.flatnonzero(S == 0.5)[0])
        idx = np.unravel_index(k, tuple(counts)[::-1])[::-1]
        assert all(0 < i < c - 1 for i, c in zip(idx, counts))                      # an interior node
        at_node = (ref[0] == X[k]).all(1)
        assert at_node.sum() >= 2                                                   # t = 0 vertices: the node counts as inside
        sphere = _both("sphere", iso_main, tmp_path)[1]
        assert len(ref[0]) != len(sphere[0]) or ref[0].tobytes() != sphere[0].tobytes()


# ---- 3. topology and bounds ---------------------------------------------------------------------------------------------------
def _euler(elements):
    E = np.asarray(elements, np.int64)
    edges = np.sort(np.concatenate([E[:, [0, 1]], E[:, [1, 2]], E[:, [2, 0]]]), axis=1)
    return len(np.unique(E)) - len(np.unique(edges, axis=0)) + len(E)


def _cells_holding_an_element(counts, origin, spacing, vertices, elements):
    """The number of lattice cells that hold (the centroid of) an element."""
    c = np.asarray(vertices)[np.asarray(elements)].mean(1)[:, :len(counts)]
    ijk = np.floor((c - origin) / spacing).astype(np.int64)
    return len(np.unique(ijk, axis=0))


@pytest.mark.parametrize("name,chi,volume", [("sphere", 2, 4.0 / 3.0 * np.pi * SPHERE_R ** 3), ("torus", 0, 2.0 * np.pi ** 2 * TORUS_R * TORUS_r ** 2)])
def test_closed_surfaces_3d(name, chi, volume, iso_main, tmp_path):
    _, (v, e, _, _), (counts, origin, spacing, _, _, _) = _both(name, iso_main, tmp_path)
    assert isosurface.is_closed(v, e)
    assert _euler(e) == chi
    vol = isosurface.enclosed_volume(v, e)
    bound = _cells_holding_an_element(counts, origin, spacing, v, e) * float(np.prod(spacing))
    print(f"{name}: volume {vol:.6f} against {volume:.6f}, bound {bound:.6f}; area {isosurface.surface_area(v, e):.6f}")
    assert vol > 0 and abs(vol - volume) <= bound
    tri = v[e]
    assert (np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1) > 0).all()      # no degenerate triangle here


def test_circle_is_one_counter_clockwise_loop(iso_main, tmp_path):
    _, (v, e, _, _), (counts, origin, spacing, _, _, _) = _both("circle", iso_main, tmp_path)
    assert isosurface.is_closed(v, e)
    nxt = np.zeros(len(v), np.int64)
    nxt[e[:, 0]] = e[:, 1]
    k, seen = int(e[0, 0]), 0
    while True:
        k, seen = int(nxt[k]), seen + 1
        if k == e[0, 0] or seen > len(e):
            break
    assert seen == len(e) == len(v)                                                 # ONE loop
    area = isosurface.enclosed_volume(v, e)
    bound = _cells_holding_an_element(counts, origin, spacing, v, e) * float(np.prod(spacing))
    assert area > 0 and abs(area - np.pi * CIRCLE_R ** 2) <= bound                  # counter-clockwise: the inside to the left
    assert abs(isosurface.surface_area(v, e) - 2 * np.pi * CIRCLE_R) < 0.1 * 2 * np.pi * CIRCLE_R


def test_plane(iso_main, tmp_path):
    _, (v, e, _, _), _ = _both("plane", iso_main, tmp_path)
    assert len(e) > 100
    # S = c - n·x: the surface is n·x = c - level, the outside (S < level) on the side n points to
    res = (v.astype(np.longdouble) * PLANE_N.astype(np.longdouble)).sum(1) - (np.longdouble(PLANE_C) - np.longdouble(0.5))
    worst = float(np.abs(res).max() / np.spacing(abs(PLANE_C)))
    print(f"plane: {len(v)} vertices, worst residual {worst:.2f} ulp of |c|")
    assert worst <= 8.0
    tri = v[e]
    normal = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert (normal @ PLANE_N > 0).all()
    assert not isosurface.is_closed(v, e)                                           # it leaves through the sides of the lattice


def test_measures_on_hand_made_meshes():
    # the unit tetrahedron, outward normals
    v = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    e = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=np.int32)
    assert isosurface.is_closed(v, e) and isosurface.enclosed_volume(v, e) == pytest.approx(1.0 / 6.0)
    assert isosurface.surface_area(v, e) == pytest.approx(1.5 + 0.5 * np.sqrt(3.0))
    assert isosurface.enclosed_volume(v, e[:, [0, 2, 1]]) == pytest.approx(-1.0 / 6.0)
    assert not isosurface.is_closed(v, e[:3])
    flipped = e.copy(); flipped[3] = flipped[3, [0, 2, 1]]
    assert not isosurface.is_closed(v, flipped)                                     # a directed edge twice
    # the unit square, counter-clockwise
    q = np.array([[0.0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]])
    s = np.array([[0, 1], [1, 2], [2, 3], [3, 0]], dtype=np.int32)
    assert isosurface.is_closed(q, s) and isosurface.enclosed_volume(q, s) == 1.0 and isosurface.surface_area(q, s) == 4.0
    assert isosurface.enclosed_volume(q, s[:, ::-1]) == -1.0 and not isosurface.is_closed(q, s[:3])
    for bad in (lambda: isosurface.surface_area(q[:, :2], s), lambda: isosurface.is_closed(q, np.array([[0, 9]]))):
        with pytest.raises(ValueError):
            bad()


# ---- 4. the swap table -----------------------------------------------------------------------------------------------------------
def test_swap_table(iso_main):
    run = subprocess.run([iso_main, "--table"], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and not run.stderr.strip(), run.stdout + run.stderr
    rows = {2: {}, 3: {}}
    for ln in run.stdout.strip().splitlines():
        f = ln.split()
        D, s, perm, inside, count, swapped = int(f[0]), int(f[1]), tuple(int(ch) for ch in f[2]), int(f[3]), int(f[4]), int(f[5])
        assert len(f) == 6 + count * D
        rows[D][(perm, inside)] = (s, count, swapped, f[6:])
    for D, simplices, sets in ((2, 2, 8), (3, 6, 16)):
        want = isosurface.swap_table(D)
        assert len(rows[D]) == len(want) == simplices * sets
        perms = sorted({k[0] for k in rows[D]})
        assert [rows[D][(p, 0)][0] for p in perms] == list(range(simplices))         # simplices in the lexicographic order of the permutation
        some = 0
        for key, swapped in want.items():
            perm, inside = key
            elems, _ = isosurface._simplex_elements(D, perm, {k for k in range(D + 1) if (inside >> k) & 1})
            s, count, got, verts = rows[D][key]
            assert (count, got) == (len(elems), swapped), key
            some += bool(swapped)
            # … and the edges themselves: owner corner and slot of every element vertex
            masks = isosurface._corner_masks(perm)
            flat = [f"{masks[min(p, q)]}:{(masks[max(p, q)] ^ masks[min(p, q)]) - 1}" for el in elems for p, q in el]
            assert verts == flat, key
        assert 0 < some < len(want)


# ---- 5. RunSimulation ----------------------------------------------------------------------------------------------------------------
class _MeshStandIn(_StandIn):
    def isosurface(self, origin, spacing, counts, level=0.5, attributes=False):
        self.log.append(("isosurface", self.iteration))
        return np.full((2, 3), float(self.iteration)), np.array([[0, 1]], dtype=np.int32), (tuple(origin), tuple(spacing), tuple(counts), level)


def test_run_simulation_hands_the_mesh_to_the_callback():
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
                                         backend_factory=_MeshStandIn, on_output=lambda m, pp, *extra: got.append((m.Iteration, extra)), **kw)
        return steps, got, _StandIn.instances[0]

    steps, got, eng = run(isosurface=lattice)
    assert len(got) == len(steps) + 1 >= 3
    assert got[0] == (0, (None,))                                                  # the call before the first step: nothing to extract yet
    for iteration, extra in got[1:]:
        assert len(extra) == 1
        v, e, asked = extra[0]                                                      # what the backend returned, untouched
        assert (v == iteration).all() and e.tolist() == [[0, 1]]                    # extracted on the state of THIS output
        assert asked == ((0.05, 0.01), (0.1, 0.05), (12, 9), 0.5)
    seq = [e for e in eng.log if isinstance(e, tuple)]
    assert [e[0] for e in seq] == ["advance", "isosurface", "download"] * len(steps)
    # a level of the caller's; behind the field grid when that is on
    _, got2, eng2 = run(field_grid=lattice, isosurface=lattice + (0.35,))
    assert all(len(extra) == 2 for _, extra in got2) and got2[0][1] == (None, None)
    assert got2[1][1][0]["weight"].shape == (9, 12) and got2[1][1][1][2][3] == 0.35
    assert [e[0] for e in eng2.log if isinstance(e, tuple)][:4] == ["advance", "sample_grid", "isosurface", "download"]
    # without the keyword the callback keeps its arguments and nothing is extracted
    _, got3, eng3 = run()
    assert all(extra == () for _, extra in got3) and not any(e[0] == "isosurface" for e in eng3.log if isinstance(e, tuple))


# ---- 6. the library ----------------------------------------------------------------------------------------------------------
def test_the_kernels_are_built_for_gfx950_without_scratch(tmp_path):
    """The library exports the three entry points; the code object's metadata — read the way tests/test_bench_contract.py reads it —
    shows k_iso_classify, k_iso_vertices and k_iso_elements once per dimension, without scratch and without LDS (plain global
    loads), one workgroup of 256 lanes; the scan kernels are the neighbour list's three, not copies."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_report
    from sphexample_amd import build
    lib = build.build()
    dll = C.CDLL(lib)
    assert all(hasattr(dll, f"sphmi_isosurface_{k}") for k in ("build", "read", "release"))
    co = isa_report.code_object(lib, str(tmp_path))
    meta = isa_report.metadata(co)
    names = isa_report.demangle(list(meta))
    for kernel in ("k_iso_classify", "k_iso_vertices", "k_iso_elements"):
        mine = {names[k]: v for k, v in meta.items() if kernel + "<" in names[k]}
        assert len(mine) == 2 and {("<2>" in d, "<3>" in d) for d in mine} == {(True, False), (False, True)}, (kernel, sorted(mine))
        for d, v in mine.items():
            assert v["scratch_bytes"] == 0, (d, v)
            assert v["lds_bytes"] == 0, (d, v)
            assert v["vgprs"] + v["agprs"] <= 128, (d, v)
            assert v["max_flat_workgroup_size"] == 256, (d, v)
    assert len([k for k in meta if "k_nl_" in names[k]]) == 3
