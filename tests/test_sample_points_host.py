"""Host side of the point-cloud sampler (sphmi_sample_points, csrc/sphmi_point_cloud.h): the prototype, its export and its bindings;
the helpers of sphexample_amd/fields.py (segment, triangle_centroids, surface_load) on closed meshes with known loads; the plan —
point → cell → block, points → tiles — compiled for the host with the address and undefined-behaviour sanitizers
(tests/host_points/points_main.cpp, a program of its own) against a numpy restatement; the RunSimulation plumbing with a stand-in
backend; and what the built code object says about the kernels.  No GPU."""
import copy
import ctypes as C
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

from sphexample_amd import _abi
from test_field_grid_host import _StandIn, _backend, _prototype
from test_step_series_host import CSRC, SANITIZE, host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "host_points", "points_main.cpp")


# ---- the symbol -----------------------------------------------------------------------------------------------------------------
def test_header_library_and_bindings_agree():
    text = open(os.path.join(ROOT, "include", "sphmi.h")).read()
    assert re.search(r"#define\s+SPHMI_ABI_VERSION\s+5\b", text) and _abi.ABI_VERSION == 5      # append-only: the version stays
    m = re.search(r"#define\s+SPHMI_MAX_SAMPLE_POINTS\s+\(1\s*<<\s*(\d+)\)", text)
    assert m and 1 << int(m.group(1)) == _abi.MAX_SAMPLE_POINTS == 1 << 24
    proto = _prototype("sphmi_sample_points")
    assert proto == ["sphmi_handle*", "int64_t", "const double*", "double*", "int64_t*", "double*", "double*", "double*"]
    from sphexample_amd.engine import load_library
    assert hasattr(load_library(), "sphmi_sample_points")
    # the binding: the header's arity, the caller's order, a leading axis of n
    b = _backend(3)
    x = np.arange(15.0).reshape(5, 3)
    out = b.sample_points(x)
    fn = b._lib.fns["sphmi_sample_points"]
    assert fn.argtypes == [C.c_void_p, C.c_int64] + [C.c_void_p] * 6 and len(fn.argtypes) == len(proto)
    assert len(fn.calls) == 1 and len(fn.calls[0]) == len(proto) and fn.calls[0][1] == 5
    assert set(out) == {"weight", "count", "pressure", "density", "velocity"}
    assert out["weight"].shape == out["pressure"].shape == out["density"].shape == out["count"].shape == (5,)
    assert out["velocity"].shape == (5, 3) and out["count"].dtype == np.int64 and out["weight"].dtype == np.float64
    b2 = _backend(2)
    out = b2.sample_points(np.zeros((0, 2)), fields=("pressure",))                 # an empty cloud travels as n = 0
    assert set(out) == {"pressure"} and out["pressure"].shape == (0,)
    call = b2._lib.fns["sphmi_sample_points"].calls[0]
    assert call[1] == 0 and [a is None for a in call[3:]] == [True, True, False, True, True]
    for bad in (lambda: b2.sample_points(np.zeros((4, 3))), lambda: b2.sample_points(np.zeros(4)), lambda: b2.sample_points(np.zeros((4, 2)), fields=("vorticity",))):
        with pytest.raises(ValueError):
            bad()


def test_the_julia_shim_binds_the_symbol():
    from test_julia_shim import c_prototypes, shim_ccalls
    calls = [c for c in shim_ccalls() if c[0] == "sphmi_sample_points"]
    assert len(calls) == 1 and len(calls[0][2]) == len(c_prototypes()["sphmi_sample_points"][1]) == 8
    shim = open(os.path.join(ROOT, "julia", "SPHExampleMI355X.jl"), encoding="utf-8").read()
    assert shim.index("function sample_grid(") < shim.index("function sample_points(") < shim.index("function particle_fields(")


# ---- fields.py ------------------------------------------------------------------------------------------------------------------
def _cube(lo=(0.0, 0.0, 0.0), edge=1.0):
    """A cube of 6 faces × 4 triangles round the face centre (every face mirrors the opposite one), counter-clockwise from outside."""
    lo = np.asarray(lo, np.float64)
    corners = np.array([[i, j, k] for k in (0, 1) for j in (0, 1) for i in (0, 1)], np.float64)
    faces = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]      # −z, +z, −y, +y, −x, +x
    verts, tris = [c for c in corners], []
    for f in faces:
        centre = len(verts)
        verts.append(corners[list(f)].mean(0))
        tris += [(f[k], f[(k + 1) % 4], centre) for k in range(4)]
    return lo + edge * np.array(verts), np.array(tris, np.int64)


def test_segment_and_centroids():
    from sphexample_amd.fields import segment, triangle_centroids
    s = segment([0.0, 1.0, 2.0], [1.0, 1.0, 0.0], 5)
    assert s.shape == (5, 3) and s[0].tolist() == [0.0, 1.0, 2.0] and s[-1].tolist() == [1.0, 1.0, 0.0] and s[2].tolist() == [0.5, 1.0, 1.0]
    assert segment([0.25, 0.5], [9.0, 9.0], 1).tolist() == [[0.25, 0.5]] and segment([0, 0], [1, 2], 3).tolist() == [[0, 0], [0.5, 1.0], [1, 2]]
    for bad in (lambda: segment([0, 0], [1, 1, 1], 3), lambda: segment([0, 0], [1, 1], 0), lambda: segment([0], [1], 2)):
        with pytest.raises(ValueError):
            bad()
    v, t = _cube()
    c = triangle_centroids(v, t)
    assert c.shape == (24, 3) and np.allclose(c.mean(0), 0.5)
    assert c[0].tolist() == ((v[0] + v[2] + v[8]) / 3).tolist()
    assert triangle_centroids([[0.0, 0.0], [2.0, 0.0], [2.0, 4.0]], [[0, 1], [1, 2]]).tolist() == [[1.0, 0.0], [2.0, 2.0]]
    for bad in (lambda: triangle_centroids(v, t[:, :2]), lambda: triangle_centroids(v, t + 100), lambda: triangle_centroids(v[:, :2], t)):
        with pytest.raises(ValueError):
            bad()


def test_surface_load_on_closed_meshes():
    from sphexample_amd.fields import surface_load, triangle_centroids
    v, t = _cube(lo=(0.3, -0.2, 0.1))
    # the mesh is closed and its normals point outwards: Σ A n̂ = 0, and the divergence theorem gives the volume
    c = triangle_centroids(v, t)
    assert np.abs(surface_load(v, t, np.ones(len(t)))).max() <= 1e-15
    assert np.abs(surface_load(v, t, np.full(len(t), 101325.0))).max() <= 1e-10      # a uniform pressure: no force
    assert -surface_load(v, t, c[:, 2])[2] == pytest.approx(1.0, abs=1e-14)          # −Σ z A n_z = −V
    # hydrostatic p = ρ g (z0 − z): the buoyancy ρ g V upwards, no moment about the centroid
    rho, g, z0 = 1000.0, 9.81, 2.0
    p = rho * g * (z0 - c[:, 2])
    F, M = surface_load(v, t, p, about=v[:8].mean(0))
    assert np.abs(F[:2]).max() <= 1e-9 and F[2] == pytest.approx(rho * g * 1.0, rel=1e-13)
    assert np.abs(M).max() <= 1e-9
    # about another point the moment is r × F of the resultant through the centroid
    F2, M2 = surface_load(v, t, p, about=[0.0, 0.0, 0.0])
    assert F2.tolist() == F.tolist() and np.allclose(M2, np.cross(v[:8].mean(0), F), rtol=0, atol=1e-9)
    # a scaled cube: V = 8
    v2, _ = _cube(edge=2.0)
    assert surface_load(v2, t, rho * g * (z0 - triangle_centroids(v2, t)[:, 2]))[2] == pytest.approx(rho * g * 8.0, rel=1e-13)
    with pytest.raises(ValueError):
        surface_load(v, t, p[:-1])
    # 2-D: a closed counter-clockwise polygon (an L), force per unit width.  (The left side is cut at y = 1 like the right one, so
    # that the midpoint rule's error in ∮ y p n_x ds — p is linear in y, the integrand quadratic — cancels side against side.)
    poly = np.array([[0.0, 0.0], [2.0, 0.0], [2.0, 1.0], [1.0, 1.0], [1.0, 3.0], [0.0, 3.0], [0.0, 1.0]]) + np.array([0.4, -0.3])
    seg = np.array([[k, (k + 1) % len(poly)] for k in range(len(poly))])
    mid = triangle_centroids(poly, seg)
    area = 2.0 * 1.0 + 1.0 * 2.0
    assert np.abs(surface_load(poly, seg, np.full(len(seg), 5.0))).max() <= 1e-14
    Fp, Mp = surface_load(poly, seg, rho * g * (z0 - mid[:, 1]), about=[0.0, 0.0])
    assert abs(Fp[0]) <= 1e-9 and Fp[1] == pytest.approx(rho * g * area, rel=1e-13) and isinstance(Mp, float)
    # the resultant acts through the centroid of the area: M_z = x_c · F_y (p linear in y only, exact for the midpoint rule in x)
    xc = (2.0 * 1.0 * 1.0 + 1.0 * 2.0 * 0.5) / area + 0.4
    assert Mp == pytest.approx(xc * Fp[1], rel=1e-12)


# ---- the plan, compiled for the host ---------------------------------------------------------------------------------------------
def plan(gmin, npad, dims, H_inv, X):
    """numpy restatement of pc_tiling / pc_plan_point / pc_plan_tiles, with every block handing out its slots in the caller's order."""
    B = 3 if dims == 3 else 6
    gmin3 = np.array([gmin[d] if d < dims else 0 for d in range(3)], np.int64)
    np3 = np.array([npad[d] if d < dims else 1 for d in range(3)], np.int64)
    nb = (np3 + B - 1) // B
    X = np.asarray(X, np.float64).reshape(-1, dims)
    cell = np.zeros((len(X), 3), np.int64)
    with np.errstate(over="ignore"):
        t = np.trunc(np.abs(X) * H_inv + 0.5)
    c = np.where(X < 0.0, -t, t)
    i = (c - gmin3[:dims].astype(np.float64)) + 1.0
    cell[:, :dims] = np.minimum(np.maximum(i, 0.0), (np3[:dims] - 1).astype(np.float64)).astype(np.int64)
    b3 = cell // B
    block = b3[:, 0] + nb[0] * (b3[:, 1] + nb[1] * b3[:, 2])
    blocks = int(nb.prod())
    points = np.bincount(block, minlength=blocks).astype(np.int64)
    tiles = (points + 255) // 256
    first = np.concatenate([[0], np.cumsum(points)])
    order = np.argsort(block, kind="stable")
    slot = np.empty(len(X), np.int64)
    slot[order] = np.arange(len(X))
    desc = [(first[b] + 256 * k, min(256, points[b] - 256 * k)) for b in range(blocks) for k in range(tiles[b])]
    return {"blocks": blocks, "total": int(tiles.sum()), "cell": cell, "block": block, "slot": slot, "points": points, "tiles": tiles,
            "desc": np.array(desc, np.int64).reshape(-1, 2)}


def _clouds():
    """name → (gmin, np, dims, H, points): faces, the outside on each side, 0 / 1 / 256 / 257 points in a block."""
    rng = np.random.default_rng(11)
    out = {}
    for dims, gmin, npad, H in ((3, (-3, 0, 2), (17, 9, 11), 0.04), (2, (5, -7), (40, 23), 0.113)):
        B = 3 if dims == 3 else 6
        g, n = np.array(gmin, np.float64), np.array(npad)
        lo, hi = (g - 1.0) * H, (g + n - 2.0) * H                                  # the centres of padded cells 0 and np − 1
        inside = rng.uniform(lo, hi, (700, dims))
        # exactly on cell faces (c + ½)·H, on one axis and on all, block boundaries among them
        faces = rng.uniform(lo, hi, (60, dims))
        k = np.round(faces[:, 0] / H)
        faces[:, 0] = (k + 0.5) * H
        corners = (np.round(rng.uniform(lo, hi, (20, dims)) / H) + 0.5) * H
        edge_of_block = np.stack([(g + B * m - 1.0 - 0.5) * H for m in range(1, 3)])      # the face between padded cells B·m − 1 and B·m
        # outside on each side, by a cell, by three and by everything
        outside = []
        for d in range(dims):
            for far in (1.7 * H, 3.3 * H, 1e6, 1e300):
                for side in (-1, 1):
                    p = rng.uniform(lo, hi, dims)
                    p[d] = (lo[d] - far) if side < 0 else (hi[d] + far)
                    outside.append(p)
        # 1, 256 and 257 points inside three different blocks (cell centres of the blocks' first cells + a jitter inside that cell)
        crowd = []
        for m, count in enumerate((1, 256, 257)):
            centre = (g + np.array([B * m, B, 0][:dims] if dims == 3 else [B * m, B]) - 1.0) * H
            crowd.append(centre + rng.uniform(-0.4 * H, 0.4 * H, (count, dims)))
        pts = np.concatenate([inside, faces, corners, edge_of_block, np.array(outside)] + crowd)
        out[f"{dims}-D"] = (gmin, npad, dims, H, pts[rng.permutation(len(pts))])
        out[f"{dims}-D crowd alone"] = (gmin, npad, dims, H, np.concatenate(crowd))
        out[f"{dims}-D empty"] = (gmin, npad, dims, H, np.zeros((0, dims)))
    return out


def test_the_plan_compiled_for_the_host_agrees_with_numpy(tmp_path):
    main = [ln.split()[1] for ln in open(MAIN).read().splitlines() if ln.startswith("#include")]
    assert [i for i in main if i.startswith('"')] == ['"sphmi_point_cloud.h"']
    cxx = host_compiler()
    exe = str(tmp_path / "points_main")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I", CSRC, MAIN, "-o", exe]
    for extra in (SANITIZE + ("-static-libasan", "-static-libubsan"), SANITIZE, ()):
        built = subprocess.run(base + list(extra), capture_output=True, text=True)
        if built.returncode == 0:
            break
    assert built.returncode == 0, built.stderr
    print("sanitizers:", " ".join(extra) or "none")
    alone = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert alone.returncode == 0 and alone.stdout.strip().splitlines()[-1] == "ok" and not alone.stderr.strip(), alone.stdout + alone.stderr
    for name, (gmin, npad, dims, H, X) in _clouds().items():
        H_inv = 1.0 / H
        want = plan(gmin, npad, dims, H_inv, X)
        g3 = list(gmin) + [0] * (3 - dims)
        n3 = list(npad) + [1] * (3 - dims)
        src, dst = str(tmp_path / "cloud.bin"), str(tmp_path / "bins.bin")
        with open(src, "wb") as f:
            f.write(struct.pack("<8qd", *g3, *n3, dims, len(X), H_inv) + np.ascontiguousarray(X, np.float64).tobytes())
        run = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=60)
        assert run.returncode == 0, (name, run.stdout + run.stderr)
        assert run.stdout.strip().splitlines()[-1] == "ok", run.stdout
        assert not run.stderr.strip(), run.stderr                                  # a sanitizer report would be here
        raw = np.fromfile(dst, dtype=np.int64)
        n, nb = len(X), want["blocks"]
        assert raw[0] == nb and raw[1] == want["total"], name
        assert len(raw) == 2 + 5 * n + 2 * nb + 2 * want["total"], name
        at = 2
        for key, count, shape in (("cell", 3 * n, (n, 3)), ("block", n, (n,)), ("slot", n, (n,)), ("points", nb, (nb,)), ("tiles", nb, (nb,)),
                                  ("desc", 2 * want["total"], (-1, 2))):
            np.testing.assert_array_equal(raw[at:at + count].reshape(shape), want[key], err_msg=f"{name}: {key}")
            at += count
        # the cases the clouds are there for
        if name.endswith("crowd alone"):
            assert sorted(want["points"][want["points"] > 0].tolist()) == [1, 256, 257] and sorted(want["tiles"][want["tiles"] > 0].tolist()) == [1, 1, 2]
            assert (want["points"] == 0).any() and want["desc"][:, 1].tolist().count(1) == 2      # the lone point and the 257th
        elif name.endswith("empty"):
            assert want["total"] == 0 and len(want["desc"]) == 0
        else:
            cell = want["cell"][:, :dims]
            top = np.array(npad) - 1
            assert all((cell[:, d] == 0).sum() >= 4 and (cell[:, d] == top[d]).sum() >= 4 for d in range(dims)), name      # outside on each side
            # every tile holds points of one block, every point sits in exactly one tile
            owner = np.empty(n, np.int64)
            owner[want["slot"]] = want["block"]
            seen = np.zeros(n, np.int64)
            for first, count in want["desc"]:
                assert 1 <= count <= 256 and len(set(owner[first:first + count].tolist())) == 1
                seen[first:first + count] += 1
            assert (seen == 1).all()


# ---- RunSimulation --------------------------------------------------------------------------------------------------------------
class _CloudStandIn(_StandIn):
    def sample_points(self, positions):
        self.log.append(("sample_points", self.iteration))
        n = len(positions)
        return {"weight": np.full(n, float(self.iteration)), "count": np.zeros(n, np.int64), "pressure": np.zeros(n), "density": np.zeros(n),
                "velocity": np.zeros((n, 3)), "positions": np.array(positions)}


def test_run_simulation_hands_the_cloud_to_the_callback():
    from conftest import load_dam_break_2d
    from sphexample_amd import simulation
    p, s = load_dam_break_2d()
    cloud = [[0.1, 0.2], [0.3, 0.4], [0.5, 0.6]]

    def run(**kw):
        meta = copy.deepcopy(s.SimMetaData)
        meta.SimulationTime, meta.OutputTimes = 0.002, 0.001
        got = []
        _StandIn.instances.clear()
        steps = simulation.RunSimulation(SimGeometry=None, SimMetaData=meta, SimConstants=s.SimConstants, SimKernel=s.SimKernel, SimLogger=None,
                                         SimParticles=p.copy(), SimViscosity=s.SimViscosity, SimDensityDiffusion=s.SimDensityDiffusion,
                                         backend_factory=_CloudStandIn, on_output=lambda m, pp, *extra: got.append((m.Iteration, extra)), **kw)
        return steps, got, _StandIn.instances[0]

    steps, got, eng = run(sample_points=cloud)
    assert len(got) == len(steps) + 1 >= 3 and got[0] == (0, (None,))              # the call before the first step: nothing to sample yet
    for iteration, extra in got[1:]:
        assert len(extra) == 1 and extra[0]["weight"].shape == (3,) and extra[0]["velocity"].shape == (3, 3)
        assert (extra[0]["weight"] == iteration).all() and extra[0]["positions"].tolist() == cloud      # on the state of THIS output
    seq = [e for e in eng.log if isinstance(e, tuple)]
    assert [e[0] for e in seq] == ["advance", "sample_points", "download"] * len(steps)
    # behind the field grid when both are on; the default leaves the callback's arguments as they were
    _, got2, _ = run(field_grid=([0.05, 0.01], [0.1, 0.05], [4, 3]), sample_points=cloud)
    assert all(len(extra) == 2 for _, extra in got2) and got2[1][1][0]["weight"].shape == (3, 4) and got2[1][1][1]["weight"].shape == (3,)
    _, got3, eng3 = run()
    assert all(extra == () for _, extra in got3) and not any(e[0] == "sample_points" for e in eng3.log if isinstance(e, tuple))


# ---- the code object ------------------------------------------------------------------------------------------------------------
def test_the_kernels_are_built_for_gfx950_without_scratch(tmp_path):
    """The code object's metadata — read the way tests/test_bench_contract.py reads it — shows the four instantiations of
    k_point_cloud without scratch, with no more LDS and registers than k_field_grid is held to (four workgroups per compute unit,
    four waves per SIMD), and the four kernels of the bin without scratch or LDS."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_report
    from sphexample_amd import build
    lib = build.build()
    assert hasattr(C.CDLL(lib), "sphmi_sample_points")
    co = isa_report.code_object(lib, str(tmp_path))
    meta = isa_report.metadata(co)
    names = isa_report.demangle(list(meta))
    mine = {names[k]: v for k, v in meta.items() if "k_point_cloud" in names[k]}
    assert len(mine) == 4, sorted(mine)
    assert {("<float, 2>" in d, "<double, 3>" in d) for d in mine} >= {(True, False), (False, True)}
    lattice = {names[k]: v for k, v in meta.items() if "k_field_grid" in names[k]}
    for d, v in mine.items():
        assert v["scratch_bytes"] == 0, (d, v)
        assert v["lds_bytes"] <= max(w["lds_bytes"] for w in lattice.values()) and 4 * v["lds_bytes"] <= 160 * 1024, (d, v)
        assert v["vgprs"] + v["agprs"] <= 128, (d, v)
        assert v["max_flat_workgroup_size"] == 256, (d, v)
    bins = {names[k]: v for k, v in meta.items() if re.search(r"\bk_pc_(count|tiles|scatter|describe)\b", names[k])}
    assert len(bins) == 4, sorted(bins)
    for d, v in bins.items():
        assert v["scratch_bytes"] == 0 and v["lds_bytes"] == 0, (d, v)
