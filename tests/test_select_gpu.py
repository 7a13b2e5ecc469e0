"""A selected subset of the rows, compacted on the device (sphmi_select_build / _read / _download* / _release, csrc/sphmi_select.h) —
needs a real MI355X.

The reference is `selection.restate` on a full Float64 download taken at the same point — pinned against the C++ predicate and a
row-by-row loop in tests/test_select_host.py; it never calls the code under test — and the full download itself: the rows must be
EQUAL to the restatement and every delivered array equal to ``full[field][rows]`` byte for byte, on fp64 and fp32 handles, with
Float64 and Float32 host arrays, with vectors of dims and of 3 components.  Fixtures: the 2-D dam break (6 881 rows) and the shipped
3-D one (17 446 rows) after 12 steps, so that the sort has moved rows.

Not tested here: SPHMI_ERR_DEVICE (an arena the device cannot hold needs more rows than a test can hold).
"""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest

from sphexample_amd import selection
from sphexample_amd._abi import DOWNLOAD_NAMES, ERR_ARGUMENT, ERR_STATE, SphmiError, SphmiSelection
from sphexample_amd.selection import Selection, every, restate, slab, where
from test_host_float32_gpu import as_float32
from test_probes_gpu import _engine, _state

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = {"dam_break_2d": 6881, "dam_break_3d_shipped": 17446}
STEPS = 12
INF = float("inf")


def _as_float64(p):
    """The same VALUES as `p` (a Float32 SimParticles) in Float64 arrays: both handles start from identical device state."""
    q = p.copy()
    q.FloatType = np.float64
    for k in ("Position", "Velocity", "Acceleration", "Density", "Pressure", "GhostPoints"):
        a = getattr(q, k, None)
        if isinstance(a, np.ndarray) and a.dtype == np.float32:
            setattr(q, k, np.ascontiguousarray(a.astype(np.float64)))
    return q


def _columns(n, seed=4):
    """Three passive columns of row widths 1, 8 and 33 bytes."""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, n).astype(np.uint8), rng.standard_normal(n), rng.integers(0, 256, (n, 33)).astype(np.uint8)]


def _full_columns(eng, cols):
    outs = [np.zeros_like(c) for c in cols]
    eng.download_columns(outs)
    return [o.reshape(len(o), -1).view(np.uint8) for o in outs]


def _specs(full, cfg, dims, seed=1):
    """One selection per clause and one with every clause, built from the Float64 download `full`."""
    n = len(full["Type"])
    rng = np.random.default_rng(seed)
    x = full["Position"]
    H = cfg.H
    mid = [float(np.median(x[:, d])) for d in range(dims)]
    lo1, hi1 = np.full(dims, -INF), np.full(dims, INF)
    lo1[0], hi1[0] = float(np.sort(x[:, 0])[n // 3]), mid[0]                         # lo sits ON a row's coordinate
    lo2, hi2 = np.array(mid) - 3 * H, np.array(mid) + 3 * H
    mask = rng.integers(0, 3, n) == 0
    s2 = selection.speed2(full["Velocity"][:, :dims])
    fluid = full["Type"] == 1
    return {
        "everything": Selection(),
        "fluid": Selection(types=("Fluid",)),
        "fixed": Selection(types=("Fixed",)),
        "slab": slab(dims - 1, mid[dims - 1], H, dims=dims),
        "boxes": Selection(boxes=((lo1, hi1), (lo2, hi2))),
        "marker": Selection(markers=(1,)),
        "every8": every(8),
        "every7_3": every(7, 3),
        "density": Selection(field="Density", field_lo=float(np.median(full["Density"]))),
        "pressure": Selection(field="Pressure", field_lo=float(np.median(full["Pressure"][fluid])), field_hi=float(full["Pressure"].max())),
        "speed2": Selection(types=("Fluid",), field="Speed2", field_lo=0.0, field_hi=float(np.median(s2[fluid]))),
        "mask": where(mask),
        "all": Selection(types=("Fluid", "Fixed"), boxes=((lo1, hi1), (lo2, hi2)), markers=(1, 2), id_stride=2, id_phase=1, field="Density",
                         field_lo=float(np.quantile(full["Density"], 0.2)), field_hi=INF, mask=rng.integers(0, 4, n) != 0),
    }


def _check(eng, spec, full64, full_own, comps, what, cols=None):
    """One build against the restatement and the full download; prints its figures before it asserts.  `full64`: the Float64
    download the clauses read; `full_own`: the full download of `eng` itself with `comps` components, which the arrays equal."""
    want = restate(spec, full64)
    n_rows, kept = eng.select_build(spec)
    rows = eng.select_read()
    print(f"{what}: {n_rows} rows, {kept} selected (restated: {len(want)})")
    assert n_rows == len(full64["Type"]) and kept == len(rows) and rows.dtype == np.int32
    np.testing.assert_array_equal(rows, want)
    got = eng.select_download(components=comps)
    assert set(got) == set(DOWNLOAD_NAMES)
    for k in DOWNLOAD_NAMES:
        ref = full_own[k][rows]
        assert got[k].dtype == ref.dtype and got[k].shape == ref.shape, (what, k, got[k].shape, ref.shape)
        assert got[k].tobytes() == ref.tobytes(), (what, k)
    if cols is not None:
        for c, (g, ref) in enumerate(zip(eng.select_download_columns(), cols)):
            assert g.tobytes() == ref[rows].tobytes(), (what, "column", c)
    eng.select_release()
    return rows


# ---- 1. bit-exact subset, per clause and with all clauses together -----------------------------------------------------------------
@pytest.mark.parametrize("host", [8, 4])
@pytest.mark.parametrize("fb", [8, 4])
@pytest.mark.parametrize("case", list(ROWS))
def test_equals_the_restatement_and_the_full_download(case, fb, host, request):
    p, s = _state(case, request)
    assert len(p) == ROWS[case]
    dims = s.SimMetaData.Dimensions
    wall = None
    if fb == 4 and host == 8:
        # two Fixed rows that differ only in the low word of x: one wall row is moved by 1e-9, far below the fp32 spacing of its record
        fixed = np.flatnonzero(p.Type == 2)
        xs, cnt = np.unique(p.Position[fixed, 0], return_counts=True)
        cnt = np.where(xs > 0.1, cnt, 0)                                              # (a column whose x has fp32 neighbours far coarser than 1e-9)
        col = fixed[p.Position[fixed, 0] == xs[np.argmax(cnt)]]
        wall = (int(col[0]), int(col[1]))
        p.Position[wall[0], 0] += 1e-9
        wall_ids = (int(p.ID[wall[0]]), int(p.ID[wall[1]]))
    if host == 4:
        p = as_float32(p)
        ref = _engine(_as_float64(p), s, fb)                                         # the Float64 view of the same state: what the clauses read
    eng = _engine(p, s, fb)
    cols = _columns(len(p))
    eng.attach_columns(cols)
    assert eng.advance(1e9, max_steps=STEPS).iteration == STEPS
    if host == 4:
        assert ref.advance(1e9, max_steps=STEPS).iteration == STEPS
        full64 = ref.download()
        ref.close()
    else:
        full64 = eng.download()
    assert full64["Position"].dtype == np.float64
    assert (full64["ID"] != p.ID).any()                                             # the sort has moved rows
    full_cols = _full_columns(eng, cols)
    kept = {}
    for comps in (dims, 3):
        own = eng.download(components=comps)
        assert own["Position"].dtype == (np.float64 if host == 8 else np.float32) and own["Position"].shape[1] == comps
        if host == 4:
            for k in ("ID", "Type", "GroupMarker", "Cells"):
                assert own[k].tobytes() == full64[k].tobytes(), k                   # the two handles hold the same rows in the same order
        for name, spec in _specs(full64, eng.cfg, dims).items():
            rows = _check(eng, spec, full64, own, comps, f"{case} fp{8 * fb} host{8 * host} c{comps} {name}", full_cols if comps == dims else None)
            kept[name] = len(rows)
    n = len(p)
    assert kept["everything"] == n and 0 < kept["fixed"] < n and kept["fluid"] + kept["fixed"] == n
    assert all(0 < kept[k] < n for k in ("slab", "boxes", "marker", "every8", "every7_3", "density", "pressure", "speed2", "mask", "all")), kept
    if wall is not None:
        a, b = (int(np.flatnonzero(full64["ID"] == i)[0]) for i in wall_ids)
        xa, xb = float(full64["Position"][a, 0]), float(full64["Position"][b, 0])
        print(f"low-word pair: rows {a}, {b}, x = {xa!r}, {xb!r}")
        assert np.float32(xa) == np.float32(xb) and xa > xb                           # the same record, another low word
        edge = Selection(boxes=((np.array([xa] + [-INF] * (dims - 1)), np.array([INF] * dims)),))      # the edge: between the two rows
        rows = _check(eng, edge, full64, eng.download(), dims, f"{case} edge between two low words")
        assert a in rows and b not in rows
    eng.close()


# ---- 2. sizes where a compaction can go wrong ------------------------------------------------------------------------------------
def _scan_tile():
    src = open(os.path.join(ROOT, "sphexample_amd", "csrc", "sphmi_neighbor_list.h")).read()
    m = re.search(r"constexpr int kNlScanThreads = (\d+), kNlScanItems = (\d+), kNlScanTile = kNlScanThreads \* kNlScanItems;", src)
    return int(m.group(1)) * int(m.group(2))


@pytest.mark.parametrize("fb", [8, 4])
def test_the_sizes_where_a_compaction_can_go_wrong(fb, request):
    p, s = _state("dam_break_2d", request)
    eng = _engine(p, s, fb)
    assert eng.advance(1e9, max_steps=STEPS).iteration == STEPS
    full = eng.download()
    n, tile = len(p), _scan_tile()
    assert tile == 2048 and n > 3 * tile
    rng = np.random.default_rng(8)
    picks = {f"{k} kept": np.sort(rng.choice(n, k, replace=False)) for k in (0, 1, 63, 64, 65)}
    picks["all kept"] = np.arange(n)
    picks["last row alone"] = np.array([n - 1])
    picks["first row alone"] = np.array([0])
    picks["across one tile boundary"] = np.arange(tile - 3, tile + 4)
    picks["the last of a tile and the first of the one after next"] = np.array([tile - 1, 2 * tile])
    picks["a whole tile"] = np.arange(tile, 2 * tile)
    for what, keep in picks.items():
        mask = np.zeros(n, dtype=np.uint8)
        mask[keep] = 1
        rows = _check(eng, where(mask), full, full, 2, f"fp{8 * fb} {what}")
        assert rows.tolist() == keep.tolist()
    eng.close()


# ---- 3. before the first step ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fb", [8, 4])
def test_directly_after_the_upload(fb, request):
    """No cell list and no half-step set yet: the Pressure clause and the Pressure field come from the pre-step branch of the download."""
    p, s = _state("dam_break_2d", request)
    eng = _engine(p, s, fb)
    full = eng.download()
    assert (full["Cells"] == 0).all() and np.array_equal(full["ID"], p.ID)
    fluid = full["Type"] == 1
    spec = Selection(field="Pressure", field_lo=float(np.median(full["Pressure"][fluid])))
    rows = _check(eng, spec, full, full, 2, f"fp{8 * fb} before the first step, pressure")
    assert 0 < len(rows) < len(p)
    _check(eng, slab(1, 0.2, eng.cfg.H, types=("Fluid",)), full, full, 2, f"fp{8 * fb} before the first step, slab")
    assert eng.advance(1e9, max_steps=2).iteration == 2                              # … and the handle goes on
    full = eng.download()
    _check(eng, spec, full, full, 2, f"fp{8 * fb} after two steps, pressure")
    eng.close()


# ---- 4. the held-result contract -------------------------------------------------------------------------------------------------------
def _refused(call, status, text):
    with pytest.raises(SphmiError) as ei:
        call()
    assert ei.value.status == status and text in str(ei.value), str(ei.value)


def test_held_result_contract(request):
    p, s = _state("dam_break_2d", request)
    eng = _engine(p, s, 4)
    assert eng.advance(1e9, max_steps=STEPS).iteration == STEPS
    spec = Selection(types=("Fluid",), id_stride=3, id_phase=2, field="Speed2", field_lo=0.0, field_hi=4.0)
    a = eng.select(spec, columns=False)
    b = eng.select(spec, columns=False)
    assert a[0].tobytes() == b[0].tobytes() and all(a[1][k].tobytes() == b[1][k].tobytes() for k in DOWNLOAD_NAMES) and 0 < len(a[0]) < len(p)
    _refused(eng.select_read, ERR_STATE, "no selection")                           # select() released
    eng.select_build(spec)
    assert eng.advance(1e9, max_steps=1).steps_done == 1
    _refused(eng.select_read, ERR_STATE, "stale")
    _refused(eng.select_download, ERR_STATE, "stale")
    eng.attach_columns(_columns(len(p)))
    _refused(eng.select_download_columns, ERR_STATE, "stale")
    assert eng.select_build(spec)[0] == len(p)                                     # a rebuild works again
    assert len(eng.select_read()) > 0
    eng.select_release()
    _refused(eng.select_read, ERR_STATE, "no selection")
    _refused(eng.select_download, ERR_STATE, "no selection")
    eng.select_release()                                                           # releasing nothing is legal
    n_rows, kept = eng.select_build(spec)
    assert len(eng.select_read()) == kept and eng.select_download(("ID",))["ID"].shape == (kept,)
    eng.attach_columns([])                                                         # detached: a column download has nothing to deliver
    eng._column_widths = [1]
    _refused(eng.select_download_columns, ERR_STATE, "no columns attached")
    eng.forces_once()
    _refused(eng.select_read, ERR_STATE, "stale")
    eng.upload_particles(p)
    _refused(eng.select_read, ERR_STATE, "stale")
    assert eng.select_build(spec)[0] == len(p)
    eng.close()


def test_errors(request):
    from sphexample_amd._abi import make_config
    from sphexample_amd.engine import Engine
    p, s = _state("dam_break_2d", request)
    cfg = make_config(len(p), s.SimConstants, s.SimKernel, s.SimMetaData, s.SimViscosity, s.SimDensityDiffusion, device_float_bytes=8, host_float_bytes=8)
    bare = Engine(cfg)
    _refused(lambda: bare.select_build(Selection()), ERR_STATE, "before sphmi_upload")
    _refused(bare.select_read, ERR_STATE, "before sphmi_upload")
    bare.upload_particles(p)
    assert bare.select_build(Selection()) == (len(p), len(p))                       # an upload and nothing more
    f = bare._fn("select_build")
    rows, kept = C.c_int64(), C.c_int64()
    lo, hi = np.zeros((1, 2)), np.ones((1, 2))
    mk = np.array([1], dtype=np.uint64)
    nan = float("nan")

    def sel(**kw):
        d = dict(type_mask=7, n_boxes=0, box_lo=None, box_hi=None, n_markers=0, markers=None, id_stride=1, id_phase=0, field=0, field_lo=-INF,
                 field_hi=INF, row_mask=None)
        d.update(kw)
        return SphmiSelection(**d)

    def build(s_, kept_=kept):
        return lambda: bare._check(f(bare._h, None if s_ is None else C.byref(s_), C.byref(rows), None if kept_ is None else C.byref(kept_)))
    bad_lo = np.array([[nan, 0.0]])
    for what, call in {
        "null selection": build(None), "null n_selected_out": build(sel(), None),
        "type_mask": build(sel(type_mask=0)), "type_mask ": build(sel(type_mask=8)), "type_mask  ": build(sel(type_mask=1 << 31)),
        "n_boxes": build(sel(n_boxes=-1)), "n_boxes ": build(sel(n_boxes=17, box_lo=lo.ctypes.data, box_hi=hi.ctypes.data)),
        "box_lo or box_hi": build(sel(n_boxes=1, box_lo=None, box_hi=hi.ctypes.data)), "box_lo or box_hi ": build(sel(n_boxes=1, box_lo=lo.ctypes.data)),
        "n_markers": build(sel(n_markers=-2)), "n_markers ": build(sel(n_markers=17, markers=mk.ctypes.data)),
        "markers without a table": build(sel(n_markers=1)),
        "id_stride": build(sel(id_stride=0)), "id_stride ": build(sel(id_stride=-4)),
        "id_phase": build(sel(id_stride=4, id_phase=4)), "id_phase ": build(sel(id_stride=4, id_phase=-1)), "id_phase  ": build(sel(id_stride=1, id_phase=1)),
        "unknown field": build(sel(field=4)), "unknown field ": build(sel(field=-1)),
        "NaN field bound": build(sel(field=1, field_lo=nan)), "NaN field bound ": build(sel(field=3, field_hi=nan)),
        "NaN box bound": build(sel(n_boxes=1, box_lo=bad_lo.ctypes.data, box_hi=hi.ctypes.data)),
        "NaN box bound ": build(sel(n_boxes=1, box_lo=lo.ctypes.data, box_hi=bad_lo.ctypes.data)),
    }.items():
        _refused(call, ERR_ARGUMENT, what.strip())
    assert len(bare.select_read()) == len(p)                                       # the arguments are judged first: the result before stays
    bare.select_release()
    bare._check(f(bare._h, C.byref(sel(n_boxes=1, box_lo=lo.ctypes.data, box_hi=hi.ctypes.data)), None, C.byref(kept)))      # n_rows_out may be NULL
    assert 0 < kept.value < len(p)
    with pytest.raises(RuntimeError, match="did not build"):                       # the wrapper sizes its arrays from its OWN build
        bare.select_read()
    assert bare.advance(1e9, max_steps=2).steps_done == 2                           # … and the handle still advances
    bare.close()
    slabs = _engine(p, s, 8, devices=[0, 0])                                       # two slabs on one GPU
    _refused(lambda: slabs.select_build(Selection()), ERR_STATE, "single-device")
    slabs.advance(1e9, max_steps=3)
    _refused(lambda: slabs.select_build(every(2)), ERR_STATE, "single-device")
    _refused(slabs.select_read, ERR_STATE, "no selection")
    slabs.select_release()
    assert slabs.advance(1e9, max_steps=2).steps_done == 2
    slabs.close()


# ---- 5. what a selection leaves alone --------------------------------------------------------------------------------------------------
def test_a_pending_download_survives(request):
    p, s = _state("dam_break_3d_shipped", request)
    eng = _engine(p, s, 4)
    assert eng.advance(1e9, max_steps=STEPS).iteration == STEPS
    plain = eng.download()
    n, D = len(p), 3
    out = {k: np.full_like(plain[k], 7) for k in DOWNLOAD_NAMES}
    eng._check(eng._fn("download_begin")(eng._h, *[out[k].ctypes.data_as(C.c_void_p) for k in DOWNLOAD_NAMES]))
    rows, got = eng.select(Selection(types=("Fluid",), id_stride=2))               # build, read, download, release — between begin and end
    _, everything = eng.select(Selection())                                        # as large as the pending snapshot itself
    eng.download_end()
    for k in DOWNLOAD_NAMES:
        assert out[k].tobytes() == plain[k].tobytes(), k
        assert got[k].tobytes() == plain[k][rows].tobytes() and everything[k].tobytes() == plain[k].tobytes(), k
    assert 0 < len(rows) < n and D == eng.D
    eng.close()


def test_nothing_else_moves(request):
    p, s = _state("dam_break_2d", request)
    a, b = _engine(p, s, 4), _engine(p, s, 4)
    for eng in (a, b):
        assert eng.advance(1e9, max_steps=STEPS).iteration == STEPS
    n_rows, n_pairs = a.neighbors_build()
    off0, nbr0 = a.neighbors_read()
    mask = np.random.default_rng(3).integers(0, 2, len(p))
    rows, _ = a.select(Selection(types=("Fluid",), boxes=((np.array([0.0, 0.0]), np.array([1.0, 0.3])),), id_stride=2, field="Pressure", field_lo=0.0,
                                 mask=mask), columns=False)
    assert len(rows) > 0
    off1, nbr1 = a.neighbors_read()                                                 # held across the selection: still readable, the same bytes
    assert off1.tobytes() == off0.tobytes() and nbr1.tobytes() == nbr0.tobytes() and len(nbr1) == n_pairs
    a.neighbors_release()
    for eng in (a, b):
        assert eng.advance(1e9, max_steps=STEPS).steps_done == STEPS
    da, db = a.download(), b.download()
    for k in DOWNLOAD_NAMES:
        assert da[k].tobytes() == db[k].tobytes(), k                                # advance, select, advance == advance, advance
    a.close(); b.close()


# ---- 6. RunSimulation ------------------------------------------------------------------------------------------------------------------
def test_run_simulation_delivers_the_subset_with_every_output(request):
    from sphexample_amd import simulation
    p0, s = request.getfixturevalue("dam_break_2d")
    p = p0.copy()
    meta = copy.deepcopy(s.SimMetaData)
    meta.SimulationTime, meta.OutputTimes = 0.003, 0.001
    H = s.SimKernel.H
    spec = slab(1, 0.1, 4 * H, types=("Fluid",), id_stride=2)
    seen = []

    def on_output(m, pp, subset):
        rows, got = subset
        # the first call hands over the particles as the CALLER holds them, before any download: what the engine does not take from
        # them (Pressure) or returns as record + low word (Position, Density) is compared from the first download on
        names = ("ID", "Type", "GroupMarker") if not seen else ("Position", "Velocity", "Density", "Pressure", "ID", "Type", "GroupMarker")
        full = {k: np.array(getattr(pp, k)) for k in names}
        if seen:
            np.testing.assert_array_equal(rows, restate(spec, full))
        assert rows.dtype == np.int32 and (np.diff(rows) > 0).all()
        for k, v in full.items():
            assert got[k].tobytes() == v[rows].tobytes(), (m.Iteration, k)
        seen.append((m.Iteration, len(rows)))

    steps = simulation.RunSimulation(SimGeometry=None, SimMetaData=meta, SimConstants=s.SimConstants, SimKernel=s.SimKernel, SimLogger=None,
                                     SimParticles=p, SimViscosity=s.SimViscosity, SimDensityDiffusion=s.SimDensityDiffusion, on_output=on_output,
                                     output_select=spec)
    print(seen)
    assert len(seen) == len(steps) + 1 >= 4 and seen[0][0] == 0 and all(0 < k < len(p) for _, k in seen)
