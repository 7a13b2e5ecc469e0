"""The free surface as a mesh, extracted on the device (sphmi_isosurface_build / _read / _release, csrc/sphmi_isosurface.h) — needs a
real MI355X.

The reference is `sphexample_amd.isosurface.extract`, the numpy restatement of the contract in include/sphmi.h (pinned against the
stand-alone host program and on analytic fields in tests/test_isosurface_host.py), applied to what `Backend.sample_grid` returns for
the same lattice with no step in between.  The mesh must be EQUAL to it: vertices, pressure and velocity as bytes, elements as
integers, on fp64 and fp32 handles — the kernels read the very S the sampler delivers and round every operation once.
"""
import ctypes as C

import numpy as np
import pytest

from sphexample_amd import isosurface
from sphexample_amd._abi import ERR_ARGUMENT, ERR_STATE, SphmiError
from test_probes_gpu import _engine, _state, _variant

pytestmark = pytest.mark.gpu

IRR = np.array([0.318309886, 0.577215665, 0.693147181])            # offsets in units of dp: nothing the particle lattice knows
STEPS = {"dam_break_2d": 12, "dam_break_3d_shipped": 6}


def _reference(eng, lattice, level=0.5):
    out = eng.sample_grid(*lattice)
    return isosurface.extract(out["weight"], lattice[0], lattice[1], level, pressure=out["pressure"], velocity=out["velocity"], count=out["count"]), out


def _same(got, ref, what):
    for a, b, name in zip(got, ref, ("vertices", "elements", "pressure", "velocity")):
        assert a.shape == b.shape and a.dtype == b.dtype, (what, name, a.shape, b.shape)
        if name == "elements":
            np.testing.assert_array_equal(a, b, err_msg=f"{what}: {name}")
        else:
            assert a.tobytes() == b.tobytes(), (what, name, int((a != b).sum()))


def _check(eng, lattice, what, level=0.5):
    got = eng.isosurface(*lattice, level=level, attributes=True)
    ref, out = _reference(eng, lattice, level)
    print(f"{what}: lattice {tuple(int(c) for c in lattice[2])}, {len(ref[0])} vertices, {len(ref[1])} elements")
    assert got[0].dtype == np.float64 and got[1].dtype == np.int32 and got[0].shape[1] == 3 and got[1].shape[1] == eng.D
    _same(got, ref, what)
    if eng.D == 2:
        assert (got[0][:, 2] == 0).all() and (got[3][:, 2] == 0).all()
    return got, out


def _lattices(eng, d):
    """The shapes of the issue, from a downloaded state: name → (origin, spacing, counts)."""
    X, T = d["Position"].astype(np.float64), d["Type"]
    D = X.shape[1]
    F = X[T == 1]
    H, dp = eng.cfg.H, eng.cfg.dx
    lo, hi = X.min(0), X.max(0)
    flo, fhi = F.min(0), F.max(0)
    irr = IRR[:D] * dp
    top = np.array([0.5 * (flo[0] + fhi[0]), fhi[1]] if D == 2 else [0.5 * (flo[0] + fhi[0]), 0.5 * (flo[1] + fhi[1]), fhi[2]])      # on the free surface
    ints = lambda *c: np.array(c[:D], dtype=np.int64)                               # noqa: E731
    out = {}
    # one cell, 2^D nodes, across the free surface
    out["one cell"] = (top - 0.6 * dp + 0.1 * irr, np.full(D, 1.3 * dp), np.full(D, 2, dtype=np.int64))
    # a count of 1 along one axis: no cells, an empty mesh (the plane runs through water)
    c = ints(40, 30, 1) if D == 3 else ints(40, 1)
    o = flo - 0.5 * H + irr
    o[D - 1] = 0.5 * (flo[D - 1] + fhi[D - 1])
    out["flat"] = (o, (fhi + 1.0 * H - flo) / np.maximum(c - 1, 1), c)
    # 257 nodes along x: one node past a workgroup of the kernels and past a brick of the sampler
    c = ints(257, 9, 5) if D == 3 else ints(257, 23)
    out["257 along x"] = (flo - 0.4 * H + irr, (fhi + 0.8 * H - flo) / (c - 1), c)
    # 2 048 nodes: one scan tile; 2 049 = 3 · 683: one node past it (3-D: only with a count of 1 — the tile edge with empty counts —
    # so 13^3 = 2 197 stands in there for "past one tile" with elements)
    c = ints(16, 16, 8) if D == 3 else ints(64, 32)
    out["2048 nodes"] = (flo - 0.4 * H + irr, (fhi + 0.8 * H - flo) / (c - 1), c)
    c = ints(683, 3, 1) if D == 3 else ints(683, 3)
    o = flo - 0.4 * H + irr
    o[1] = fhi[1] - 1.5 * dp if D == 2 else 0.5 * (flo[1] + fhi[1])
    sp = (fhi + 0.8 * H - flo) / np.maximum(c - 1, 1)
    sp[1] = 1.1 * dp
    out["2049 nodes"] = (o, sp, c)
    if D == 3:
        c = ints(13, 13, 13)
        out["2197 nodes"] = (flo - 0.4 * H + irr, (fhi + 0.8 * H - flo) / (c - 1), c)
    # several scan tiles
    c = ints(20, 18, 16) if D == 3 else ints(90, 70)
    out["several tiles"] = (flo - 0.5 * H - irr, (fhi + 1.0 * H - flo) / (c - 1), c)
    # overhanging the particles' bounding grid on every side by more than three cells: zeros outside, nothing crosses there
    c = ints(27, 23, 19) if D == 3 else ints(75, 61)
    out["overhang"] = (lo - 3.3 * H - irr, (hi + 6.6 * H - lo) / (c - 1), c)
    # coarser than H: ends without rows next to ends with rows
    o = lo - 1.1 * H + irr
    out["coarse"] = (o, np.full(D, 1.7 * H), np.ceil((hi + 2.0 * H - o) / (1.7 * H)).astype(np.int64) + 1)
    return out


# ---- 1. equals the numpy restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fb", [8, 4])
@pytest.mark.parametrize("case", list(STEPS))
def test_equals_the_restatement(case, fb, request):
    p, s = _state(case, request)
    eng = _engine(p, s, fb)
    assert eng.advance(1e9, max_steps=STEPS[case]).iteration == STEPS[case]
    d = eng.download(("Position", "Type"))
    D, H = eng.D, eng.cfg.H
    for name, lattice in _lattices(eng, d).items():
        got, out = _check(eng, lattice, f"{case} fp{8 * fb} {name}")
        counts = [int(c) for c in lattice[2]]
        nodes = int(np.prod(counts))
        n, w = out["count"].reshape(-1), out["weight"].reshape(-1)
        if name == "one cell":
            assert nodes == 2 ** D and len(got[1]) >= 1
        elif name == "flat":
            assert 1 in counts and (w >= 0.5).any() and (w < 0.5).any() and len(got[0]) == 0 and len(got[1]) == 0
        elif name == "2048 nodes":
            assert nodes == 2048 and len(got[1]) > 0
        elif name == "2049 nodes":
            assert nodes == 2049 and (len(got[1]) > 0 or D == 3)
        elif name == "overhang":
            from sphexample_amd.fields import grid_axes
            X = d["Position"]
            for dim, a in enumerate(grid_axes(*lattice)):
                outside = (a < X[:, dim].min() - 1.6 * H) | (a > X[:, dim].max() + 1.6 * H)
                assert outside[:1].all() and outside[-1:].all() and (np.compress(outside, out["weight"], axis=D - 1 - dim) == 0).all()
            assert len(got[1]) > 0
        elif name == "coarse":
            assert (np.asarray(lattice[1]) > H).all() and len(got[0]) > 0
            # the rule for ends without rows decides vertices here: mixing in the empty end's zero would give other bytes
            mixed = isosurface.extract(out["weight"], lattice[0], lattice[1], 0.5, pressure=out["pressure"])[2]
            assert ((n == 0) & (w == 0)).any() and (mixed != got[2]).any()
        else:
            assert len(got[1]) > 0
    eng.close()


# ---- 2. the level rule --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,fb", [("dam_break_2d", 8), ("dam_break_2d", 4), ("dam_break_3d_shipped", 8), ("dam_break_3d_shipped", 4)])
def test_a_node_exactly_at_the_level_is_inside(case, fb, request):
    from sphexample_amd.fields import grid_nodes
    p, s = _state(case, request)
    eng = _engine(p, s, fb)
    eng.advance(1e9, max_steps=STEPS[case])
    d = eng.download(("Position", "Type"))
    lattice = _lattices(eng, d)["several tiles"]
    out = eng.sample_grid(*lattice, fields=("weight",))
    w = out["weight"]
    interior = np.zeros(w.shape, bool)
    interior[(slice(1, -1),) * eng.D] = True
    wet = np.flatnonzero((interior & (w > 0.3) & (w < 0.9) & (np.roll(w, -1, axis=-1) < w)).reshape(-1))      # … whose +x neighbour lies lower: an edge it owns crosses
    assert len(wet) > 0
    k = int(wet[len(wet) // 2])
    level = float(w.reshape(-1)[k])
    got, _ = _check(eng, lattice, f"{case} fp{8 * fb} level = S[{k}] = {level!r}", level=level)
    node = np.zeros(3)
    node[:eng.D] = grid_nodes(*lattice)[k]
    at_node = (got[0] == node).all(1)
    print(f"vertices at node {k}: {int(at_node.sum())}")
    assert at_node.sum() >= 1                                                      # t = 0: the node counts as inside and owns crossing edges
    eng.close()


# ---- 3. a closed surface ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,fb", [("dam_break_2d", 8), ("dam_break_2d", 4), ("dam_break_3d_shipped", 8), ("dam_break_3d_shipped", 4)])
def test_the_surface_round_the_whole_fluid_is_closed(case, fb, request):
    p, s = _state(case, request)
    eng = _engine(p, s, fb)
    eng.advance(1e9, max_steps=STEPS[case])
    d = eng.download(("Position", "Type"))
    F = d["Position"][d["Type"] == 1].astype(np.float64)
    D, H, dp = eng.D, eng.cfg.H, eng.cfg.dx
    spacing = np.full(D, 1.45 * dp)
    margin = H + 1.5 * spacing                                                     # at least H + one spacing: the outermost nodes see no Fluid row
    origin = F.min(0) - margin - IRR[:D] * dp
    counts = np.ceil((F.max(0) + margin - origin) / spacing).astype(np.int64) + 1
    v, e = eng.isosurface(origin, spacing, counts)
    area, vol = isosurface.surface_area(v, e), isosurface.enclosed_volume(v, e)
    print(f"{case} fp{8 * fb}: lattice {tuple(int(c) for c in counts)}, {len(v)} vertices, {len(e)} elements, area {area:.5f}, volume {vol:.5f}")
    assert len(e) > 100 and isosurface.is_closed(v, e) and vol > 0
    eng.close()


# ---- 4. repeats, and does not disturb -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,fb", [("dam_break_2d", 4), ("dam_break_2d", 8), ("dam_break_3d_shipped", 4)])
def test_repeats_and_does_not_disturb(case, fb, request):
    p, s = _state(case, request)
    markers = sorted(int(m) for m in np.unique(p.GroupMarker))
    F = p.Position[p.Type == 1]
    D = F.shape[1]
    calls = (9, 1, 7)
    runs = []
    for built in (False, True):
        eng = _engine(p, s, fb)
        H = eng.cfg.H
        counts = np.array([41, 37] if D == 2 else [21, 17, 13], dtype=np.int64)
        origin = F.min(0) - 1.2 * H + IRR[:D] * eng.cfg.dx
        lattice = (origin, (F.max(0) + 1.2 * H - origin) / (counts - 1), counts)
        other = (origin + 0.3 * H, lattice[1] * 1.7, np.maximum(counts // 2, 2))
        eng.group_forces_enable(markers, capacity=64)
        eng.probes_enable(F[:: max(len(F) // 8, 1)][:8] + 0.3 * eng.cfg.dx, capacity=64)
        prog, meshes = [], []
        for n in calls:
            q = eng.advance(1e9, max_steps=n)
            prog.append((q.iteration, q.steps_done, q.n_rebuilds, q.index_counter, q.total_time, q.last_dt, q.delta_x))
            if built:
                eng.isosurface_build(*lattice)
                a = eng.isosurface_read(pressure=True, velocity=True)
                eng.isosurface_build(*lattice)                                     # no step in between: the same bytes
                b = eng.isosurface_read(pressure=True, velocity=True)
                _same(b, a, "second build")
                eng.sample_grid(*other)                                            # fg_arena is reused; the mesh has an arena of its own
                _same(eng.isosurface_read(pressure=True, velocity=True), a, "read behind sphmi_sample_grid")
                assert len(a[1]) > 0
                meshes.append(a)
        runs.append((prog, eng.download(), eng.group_forces_read(), eng.probes_read()))
        if built:
            # a download begun before a build completes with the snapshot taken at its begin
            want = eng.download()
            spec = {k: np.zeros_like(want[k]) for k in ("Position", "Velocity", "Acceleration", "Density", "Pressure", "ID", "Type", "GroupMarker", "GhostPoints", "Cells")}
            fbeg = eng._fn("download_begin"); fbeg.argtypes = [C.c_void_p] * 11
            eng._check(fbeg(eng._h, *[spec[k].ctypes.data_as(C.c_void_p) for k in spec]))
            eng.isosurface_build(*lattice)
            mid = eng.isosurface_read(pressure=True, velocity=True)
            eng.download_end()
            for k in spec:
                np.testing.assert_array_equal(spec[k], want[k], err_msg=k)
            _same(mid, meshes[-1], "build inside a download")
        eng.close()
    assert runs[0][0][-1][0] == sum(calls) and runs[0][0] == runs[1][0]            # the progress blocks, n_rebuilds among them
    for k, v in runs[0][1].items():
        assert runs[1][1][k].tobytes() == v.tobytes(), k                            # the final download, byte for byte
    for a, b in zip(runs[0][2], runs[1][2]):
        np.testing.assert_array_equal(a, b)                                         # the group-force series
    assert len(runs[0][3]["iteration"]) == sum(calls)
    for k in runs[0][3]:
        np.testing.assert_array_equal(runs[1][3][k], runs[0][3][k], err_msg=k)      # the probe series


# ---- 5. lifetime and errors ---------------------------------------------------------------------------------------------------
def _refused(call, status, word):
    with pytest.raises(SphmiError) as ei:
        call()
    assert ei.value.status == status and word in str(ei.value), str(ei.value)


def _small_lattice(p):
    """A few dozen nodes round the whole water column: the free surface and the rim along the walls cross it."""
    F = p.Position[p.Type == 1]
    counts = np.array([8, 14], dtype=np.int64)
    origin = F.min(0) - 0.1 - 0.013
    return (origin, (F.max(0) + 0.1 - origin) / (counts - 1), counts)


def test_lifetime(request):
    p, s = _state("dam_break_2d", request)
    lattice = _small_lattice(p)
    eng = _engine(p, s, 8)
    build = lambda: eng.isosurface_build(*lattice)                                  # noqa: E731
    _refused(eng.isosurface_read, ERR_STATE, "no mesh")                             # before any build (and before any step)
    _refused(build, ERR_STATE, "has not executed a step")                           # the text sphmi_sample_grid uses
    with pytest.raises(SphmiError) as ei:
        eng.sample_grid(*lattice)
    assert "has not executed a step since the upload (no cell list, no half-step set)" in str(ei.value)
    assert eng.advance(1e9, max_steps=3).iteration == 3
    _refused(eng.isosurface_read, ERR_STATE, "no mesh")
    nv, ne = build()
    v, e, _, _ = eng.isosurface_read()
    assert v.shape == (nv, 3) and e.shape == (ne, 2) and ne > 0
    assert eng.advance(1e9, max_steps=1).steps_done == 1
    _refused(eng.isosurface_read, ERR_STATE, "stale")                               # rows may have moved
    build()                                                                         # a new build after a stale result serves again
    _same(eng.isosurface_read(pressure=True, velocity=True), _reference(eng, lattice)[0], "after a stale result")
    eng.forces_once()
    _refused(eng.isosurface_read, ERR_STATE, "stale")
    assert eng.advance(1e9, max_steps=1).steps_done == 1
    build()
    eng.upload_particles(p)                                                         # a new particle set
    _refused(eng.isosurface_read, ERR_STATE, "stale")
    _refused(build, ERR_STATE, "has not executed a step")
    _refused(eng.isosurface_read, ERR_STATE, "")                                    # (a refused build leaves nothing to read)
    assert eng.advance(1e9, max_steps=2).steps_done == 2
    build()
    eng.isosurface_release()
    _refused(eng.isosurface_read, ERR_STATE, "no mesh")                             # after release
    eng.isosurface_release()                                                        # releasing nothing is legal
    assert build()[1] == len(eng.isosurface_read()[1])
    assert eng.advance(1e9, max_steps=1).steps_done == 1
    eng.close()


def test_errors(request):
    from sphexample_amd._abi import MAX_GRID_NODES, make_config
    from sphexample_amd.engine import Engine
    p, s = _state("dam_break_2d", request)
    lattice = _small_lattice(p)
    cfg = make_config(len(p), s.SimConstants, s.SimKernel, s.SimMetaData, s.SimViscosity, s.SimDensityDiffusion, device_float_bytes=8, host_float_bytes=8)
    bare = Engine(cfg)
    _refused(lambda: bare.isosurface_build(*lattice), ERR_STATE, "before sphmi_upload")
    bare.upload_particles(p)
    _refused(lambda: bare.isosurface_build(*lattice), ERR_STATE, "has not executed a step")
    assert bare.advance(1e9, max_steps=3).iteration == 3                            # the handle still advances …
    f = bare._fn("isosurface_build")
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    o, sp, c = [np.ascontiguousarray(a, dtype=t) for a, t in zip(lattice, (np.float64, np.float64, np.int64))]
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)                                   # noqa: E731
    nv, ne = C.c_int64(), C.c_int64()
    raw = lambda *a: bare._check(f(bare._h, *a))                                    # noqa: E731
    # everything sphmi_sample_grid reports of a lattice
    _refused(lambda: raw(None, ptr(sp), ptr(c), 0.5, C.byref(nv), C.byref(ne)), ERR_ARGUMENT, "null origin")
    _refused(lambda: raw(ptr(o), None, ptr(c), 0.5, C.byref(nv), C.byref(ne)), ERR_ARGUMENT, "null origin")
    _refused(lambda: raw(ptr(o), ptr(sp), None, 0.5, C.byref(nv), C.byref(ne)), ERR_ARGUMENT, "null origin")
    for bad in ([np.nan, 0.0], [0.0, np.inf], [-np.inf, 0.0]):
        _refused(lambda: bare.isosurface_build(bad, lattice[1], lattice[2]), ERR_ARGUMENT, "non-finite origin")
    for bad in ([0.0, 0.1], [0.1, -0.1], [np.nan, 0.1], [0.1, np.inf]):
        _refused(lambda: bare.isosurface_build(lattice[0], bad, lattice[2]), ERR_ARGUMENT, "spacing")
    for bad in ([0, 4], [4, -1]):
        _refused(lambda: bare.isosurface_build(lattice[0], lattice[1], bad), ERR_ARGUMENT, "count")
    for bad in ([MAX_GRID_NODES, 2], [4097, 4096], [1 << 40, 1 << 40]):
        _refused(lambda: bare.isosurface_build(lattice[0], lattice[1], bad), ERR_ARGUMENT, "SPHMI_MAX_GRID_NODES")
    # the level; the two counts
    for bad in (0.0, -0.5, np.nan, np.inf, -np.inf):
        _refused(lambda: bare.isosurface_build(*lattice, level=bad), ERR_ARGUMENT, "level")
    _refused(lambda: raw(ptr(o), ptr(sp), ptr(c), 0.5, None, C.byref(ne)), ERR_ARGUMENT, "null n_vertices_out")
    _refused(lambda: raw(ptr(o), ptr(sp), ptr(c), 0.5, C.byref(nv), None), ERR_ARGUMENT, "null n_vertices_out")
    _refused(bare.isosurface_read, ERR_STATE, "no mesh")                            # none of the refused builds left a mesh
    raw(ptr(o), ptr(sp), ptr(c), 0.5, C.byref(nv), C.byref(ne))                     # after the argument errors the handle still builds
    assert nv.value > 0 and ne.value > 0
    with pytest.raises(RuntimeError, match="did not build"):                        # the wrapper sizes its arrays from its OWN build
        bare.isosurface_read()
    assert bare.isosurface_build(*lattice) == (nv.value, ne.value)
    _same(bare.isosurface_read(pressure=True, velocity=True), _reference(bare, lattice)[0], "after the argument errors")
    only = bare.isosurface_read(vertices=False, elements=False, velocity=True)      # any pointer may be NULL
    assert only[0] is None and only[1] is None and only[2] is None and only[3].shape == (nv.value, 3)
    assert bare.advance(1e9, max_steps=1).steps_done == 1
    bare.close()
    slabs = _engine(p, s, 8, devices=[0, 0])                                        # two slabs on one GPU
    _refused(lambda: slabs.isosurface_build(*lattice), ERR_STATE, "single-device")
    slabs.advance(1e9, max_steps=3)
    _refused(lambda: slabs.isosurface_build(*lattice), ERR_STATE, "single-device")  # … with a cell list too
    _refused(slabs.isosurface_read, ERR_STATE, "no mesh")
    slabs.isosurface_release()
    assert slabs.advance(1e9, max_steps=2).steps_done == 2
    slabs.close()
    thin = _engine(p, _variant(s, None, 0.9), 8)                                    # H < h
    _refused(lambda: thin.isosurface_build(*lattice), ERR_STATE, "H < h")
    assert thin.advance(1e9, max_steps=1).steps_done == 1
    _refused(lambda: thin.isosurface_build(*lattice), ERR_STATE, "H < h")
    thin.close()


def test_errors_rank_mode(request):
    """A rank-mode handle holds one slab of the rows per process: refused like a multi-device handle, and it goes on advancing.
    (Its own test: bringing up the communicator of a rank-mode handle takes most of the time.)"""
    p, s = _state("dam_break_2d", request)
    from sphexample_amd.engine import rccl_unique_id
    lattice = _small_lattice(p)
    rk = _engine(p, s, 8, rank=0, world=1, unique_id=rccl_unique_id())
    for _ in range(2):                                                              # before the first step, and with a cell list
        with pytest.raises(SphmiError) as ei:
            rk.isosurface_build(*lattice)
        assert ei.value.status == ERR_STATE and "single-device" in str(ei.value) and "rank-mode" in str(ei.value), str(ei.value)
        _refused(rk.isosurface_read, ERR_STATE, "no mesh")
        rk.isosurface_release()
        assert rk.advance(1e9, max_steps=2).steps_done == 2                         # the handle still advances
    rk.close()


# ---- 6. RunSimulation ---------------------------------------------------------------------------------------------------------
def test_run_simulation_hands_the_mesh_to_the_callback(dam_break_2d):
    import copy
    from sphexample_amd import simulation
    p, s = dam_break_2d
    meta = copy.deepcopy(s.SimMetaData)
    meta.SimulationTime, meta.OutputTimes = 0.002, 0.001
    F = p.Position[p.Type == 1]
    lattice = (F.min(0) - 0.15, np.array([0.03, 0.03]), np.ceil((F.max(0) - F.min(0) + 0.3) / 0.03).astype(np.int64) + 1)
    got = []
    steps = simulation.RunSimulation(SimGeometry=None, SimMetaData=meta, SimConstants=s.SimConstants, SimKernel=s.SimKernel, SimLogger=None,
                                     SimParticles=p.copy(), SimViscosity=s.SimViscosity, SimDensityDiffusion=s.SimDensityDiffusion,
                                     isosurface=lattice, on_output=lambda m, pp, mesh: got.append((m.Iteration, mesh)))
    assert len(got) == len(steps) + 1 and got[0][1] is None                        # one mesh per output; none before the first step
    box = float(np.prod(F.max(0) - F.min(0)))
    for _, (v, e) in got[1:]:
        assert e.shape[1] == 2 and isosurface.is_closed(v, e)
        assert 0.5 * box < isosurface.enclosed_volume(v, e) < 1.5 * box             # the water column, give or take its rim
