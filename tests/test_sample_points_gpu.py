"""Pressure, density, velocity and fill sampled at arbitrary points (sphmi_sample_points, csrc/sphmi_point_cloud.h) — needs a real
MI355X.

Per point the sums are the probes' and the lattice's (tests/test_probes_gpu.py, tests/test_field_grid_gpu.py): over the Fluid rows j
with |x_p - x_j|^2 <= H^2 on the state sphmi_download delivers now, w_j = (m0 / rho_j) W(|x_p - x_j|), n = rows, S = sum w_j, SP,
Srho, Sv.  The reference is the same `brute_force_probes`, an O(M·N) numpy enumeration that never calls the code under test, fed
the cloud and a download taken right after the call.

Bars (the project's for a single evaluation, as in tests/test_probes_gpu.py): 1e-10 of the field maximum on every raw sum on fp64
handles, 2e-4 on fp32 handles; n equal at every point except — fp32 handles — points where the reference itself shows a Fluid row
within 1e-6·H of the cut, at most 2 % of the points, and the reference alone must stay inside that cap: the clouds come from a
seeded generator and are shifted by offsets incommensurate with the particle lattice.  Against the lattice kernel on the nodes of
a lattice: n equal with no exception, raw sums within 1e-12 — the project's bar between two fp64 evaluations of one sum — on fp64
AND fp32 handles (both kernels read the same staged doubles).  Slab handles against the one-device handle: 1e-9 / 1e-5.  What a
point reads must not depend on the other points of the call: np.array_equal on every output.
"""
import ctypes as C

import numpy as np
import pytest

from test_probes_gpu import FIELDS, _check_against, _engine, _raw, _state, brute_force_probes

pytestmark = pytest.mark.gpu

IRR = np.array([0.318309886, 0.577215665, 0.693147181])            # offsets in units of dp: nothing the particle lattice knows
OUTPUTS = ("weight", "count", "pressure", "density", "velocity")
BLOCK = {2: 6, 3: 3}                                               # cells of a block per axis (pc_block_cells)


def _as_series(out):
    """The dict of sample_points as ONE sample of a probe series: [1, n(, 3)] — what _raw and _check_against take."""
    return {k: v[None] for k, v in out.items()}


def _check_cloud(eng, pts, fb, what):
    """Sample, download right after, enumerate.  Returns (out, ref, download)."""
    out = eng.sample_points(pts)
    d = eng.download(FIELDS)
    assert set(out) == set(OUTPUTS) and out["weight"].shape == (len(pts),) and out["velocity"].shape == (len(pts), 3) and out["count"].dtype == np.int64
    ref = brute_force_probes(eng.cfg, pts, d["Position"], d["Velocity"], d["Density"], d["Pressure"], d["Type"])
    r = _as_series(out)
    _check_against(ref, _raw(r, 0), r, fb, what, k=0)
    if eng.D == 2:
        assert (out["velocity"][:, 2] == 0).all()
    return out, ref, d


def _same_bits(a, b, what, rows=None):
    for k in OUTPUTS:
        x = a[k] if rows is None else a[k][rows]
        assert np.array_equal(x, b[k]), (what, k, int((x != b[k]).sum()))


def _one_cell(F, H, rng, count, k=None):
    """`count` points inside the ONE cell (|x/H − c| < ½ per axis) that holds a Fluid row: inside one block."""
    c = np.round(F[len(F) // 2 if k is None else k] / H)
    pts = (c + rng.uniform(-0.45, 0.45, (count, F.shape[1]))) * H
    assert len(np.unique(np.round(pts / H), axis=0)) == 1
    return pts


def _cloud(d, cfg, seed=7, uniform=500):
    """The parts of the issue, from a downloaded state.  Returns (points [M, D], slices by part)."""
    rng = np.random.default_rng(seed)
    X, T = d["Position"].astype(np.float64), d["Type"]
    D = X.shape[1]
    F = X[T == 1]
    H, dp = cfg.H, cfg.dx
    lo, hi = X.min(0), X.max(0)
    flo, fhi = F.min(0), F.max(0)
    irr = IRR[:D] * dp
    parts, pts = {}, []

    def add(name, a):
        a = np.asarray(a, np.float64).reshape(-1, D)
        at = sum(len(x) for x in pts)
        parts[name] = slice(at, at + len(a))
        pts.append(a)
    add("uniform", rng.uniform(flo, fhi, (uniform, D)) + irr)
    add("cluster", _one_cell(F, H, rng, 600))                                      # three tiles of one block
    out = []
    for dim in range(D):
        for far in (3.3 * H, 7.0 * H, 100.0, 1e6):
            for side in (-1, 1):
                p = rng.uniform(flo, fhi, D)
                p[dim] = lo[dim] - far if side < 0 else hi[dim] + far
                out.append(p)
    out.append(lo - 3.3 * H); out.append(hi + 3.3 * H)
    add("outside", out)
    # exactly ON cell faces: B + 1 consecutive faces per axis through the fluid — whatever the origin of the grid, one of them is
    # a face between two blocks — and cell corners
    faces = []
    c0 = np.round(0.5 * (flo + fhi) / H)
    for dim in range(D):
        for k in range(BLOCK[D] + 1):
            p = rng.uniform(flo, fhi, (3, D)) + irr
            p[:, dim] = (c0[dim] - 3 + k + 0.5) * H                               # cell c covers |x/H - c| <= 1/2 (map_floor rounds)
            faces.append(p)
    faces.append((np.round(F[rng.choice(len(F), 6, replace=False)] / H) + 0.5) * H)
    add("faces", np.concatenate(faces))
    add("on_particle", F[rng.choice(len(F), 12, replace=False)])                   # r = 0
    above = F.mean(0); above[-1] = fhi[-1] + 6.0 * H
    add("above", above)
    return np.concatenate(pts), parts


CASES = {  # name → (fixture, steps)
    "dam_break_2d": ("dam_break_2d", 30),
    "dam_break_3d_shipped": ("dam_break_3d_shipped", 12),
    "moving_square": ("moving_square", 25),                        # k < 2: H + h spans five cells per axis
}


# ---- 1. equals the enumeration ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fb", [8, 4])
@pytest.mark.parametrize("case", list(CASES))
def test_equals_brute_force(case, fb, request):
    fixture, K = CASES[case]
    p, s = _state(fixture, request)
    eng = _engine(p, s, fb)
    eng.advance(1e9, max_steps=K)
    d0 = eng.download(FIELDS)
    H = eng.cfg.H
    if case == "moving_square":
        assert eng.cfg.h * 2 > H * (1 + 1e-9)                                      # k < 2
    pts, parts = _cloud(d0, eng.cfg)
    perm = np.random.default_rng(3).permutation(len(pts))
    pts = pts[perm]                                                                # (the parts interleaved: the order is the caller's)
    inv = np.empty(len(pts), np.int64); inv[perm] = np.arange(len(pts))            # where a point of the parts' order went
    out, ref, d = _check_cloud(eng, pts, fb, f"{case} cloud of {len(pts)}")
    part = lambda name, a: a[inv[parts[name]]]                                     # noqa: E731
    # every part is present and is what it says
    assert (part("uniform", ref["n"]) > 0).sum() > 100
    assert parts["cluster"].stop - parts["cluster"].start == 600 and (part("cluster", ref["n"]) > 0).all()
    X = d["Position"].astype(np.float64)
    o = part("outside", pts)
    assert len(o) >= 4 * 2 * eng.D and ((o < X.min(0) - 3 * H) | (o > X.max(0) + 3 * H)).any(1).all()
    for dim in range(eng.D):
        assert (o[:, dim] < X[:, dim].min() - 3 * H).any() and (o[:, dim] > X[:, dim].max() + 3 * H).any()
    for k in OUTPUTS:
        assert (part("outside", out[k]) == 0).all(), k                             # exact zeros in every output
    f = part("faces", pts)
    on_face = np.abs(f / H - np.floor(f / H) - 0.5) < 1e-9
    assert on_face.any(1).all() and on_face.all(1).sum() >= 6 and (part("faces", ref["n"]) > 0).sum() > 10
    for dim in range(eng.D):
        assert len(np.unique(np.round(f[on_face[:, dim], dim] / H - 0.5))) >= BLOCK[eng.D] + 1      # a block boundary among them
    F = X[d["Type"] == 1]
    q = part("on_particle", pts)
    assert all((np.abs(F - x).max(1) == 0).any() for x in q) and (part("on_particle", ref["n"]) > 0).all()
    assert part("above", ref["n"]).tolist() == [0] and part("above", out["weight"]).tolist() == [0.0]
    eng.close()


# ---- 2. tile edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,fb", [("dam_break_2d", 8), ("dam_break_2d", 4), ("dam_break_3d_shipped", 4)])
def test_tile_edges(case, fb, request):
    """1, 255, 256, 257 and 513 points inside one block — one tile with one lane, a tile one short of full, a full one, a full one
    and a lane, two and a lane — and 257 copies of one point."""
    fixture, K = CASES[case]
    p, s = _state(fixture, request)
    eng = _engine(p, s, fb)
    eng.advance(1e9, max_steps=K)
    d0 = eng.download(FIELDS)
    F = d0["Position"][d0["Type"] == 1].astype(np.float64)
    rng = np.random.default_rng(17)
    for count in (1, 255, 256, 257, 513):
        pts = _one_cell(F, eng.cfg.H, rng, count)
        out, ref, _ = _check_cloud(eng, pts, fb, f"{case} {count} points in one block")
        assert (ref["n"] > 0).all()
    one = _one_cell(F, eng.cfg.H, rng, 1) + 0.1 * IRR[:eng.D] * eng.cfg.dx
    out, ref, _ = _check_cloud(eng, np.repeat(one, 257, axis=0), fb, f"{case} 257 copies of one point")
    assert ref["n"][0] > 0 and out["weight"][0] > 0
    for k in OUTPUTS:
        assert (out[k] == out[k][0]).all(), k                                      # every copy: the same bits
    _same_bits(eng.sample_points(one), {k: v[:1] for k, v in out.items()}, "a copy against the point alone")
    eng.close()


# ---- 3. independent of company and order, bitwise -----------------------------------------------------------------------------
@pytest.mark.parametrize("case,fb", [("dam_break_2d", 8), ("dam_break_2d", 4), ("dam_break_3d_shipped", 8), ("dam_break_3d_shipped", 4)])
def test_independent_of_company_and_order(case, fb, request):
    fixture, K = CASES[case]
    p, s = _state(fixture, request)
    eng = _engine(p, s, fb)
    eng.advance(1e9, max_steps=K)
    pts, parts = _cloud(eng.download(FIELDS), eng.cfg, seed=23, uniform=4300)
    assert 4900 <= len(pts) <= 5200
    full = eng.sample_points(pts)
    assert (full["count"] > 0).sum() > 1000 and (full["count"] == 0).sum() > 10
    _same_bits(eng.sample_points(pts), full, "the same call twice")
    perm = np.random.default_rng(29).permutation(len(pts))
    shuffled = eng.sample_points(pts[perm])
    _same_bits(full, shuffled, "the cloud shuffled", rows=perm)                    # shuffled[i] belongs to pts[perm[i]]
    _same_bits(full, eng.sample_points(pts[:100]), "the first 100 points alone", rows=slice(0, 100))
    for i in np.random.default_rng(31).choice(len(pts), 10, replace=False):
        _same_bits(full, eng.sample_points(pts[i:i + 1]), f"point {i} in a call of its own", rows=slice(i, i + 1))
    inside = int(np.flatnonzero(full["count"] > 0)[0])
    _same_bits(full, eng.sample_points(pts[inside:inside + 1]), "a point inside the fluid in a call of its own", rows=slice(inside, inside + 1))
    eng.close()


# ---- 4. agrees with the lattice -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,fb", [("dam_break_2d", 8), ("dam_break_2d", 4), ("dam_break_3d_shipped", 8), ("dam_break_3d_shipped", 4), ("moving_square", 8)])
def test_agrees_with_the_lattice(case, fb, request):
    from sphexample_amd.fields import grid_nodes
    p, s = _state(case, request)
    eng = _engine(p, s, fb)
    F = p.Position[p.Type == 1]
    D, H = eng.D, eng.cfg.H
    counts = np.array([32, 32] if D == 2 else [16, 8, 8], dtype=np.int64)
    origin = F.min(0) - 0.8 * H + IRR[:D] * eng.cfg.dx
    lattice = (origin, (F.max(0) + 0.8 * H - origin) / (counts - 1), counts)
    nodes = grid_nodes(*lattice)
    assert len(nodes) == 1024
    eng.advance(1e9, max_steps=25 if D == 2 else 10)
    grid = eng.sample_grid(*lattice)
    cloud = eng.sample_points(nodes)
    gr = _raw({k: v.reshape((1, -1) + v.shape[D:]) for k, v in grid.items()}, 0)
    pc = _raw(_as_series(cloud), 0)
    np.testing.assert_array_equal(pc["n"], gr["n"])                                # the same r² arithmetic: no exception
    assert (gr["n"] > 0).sum() > 100
    figures = {q: np.abs(pc[q] - gr[q]).max() / np.abs(gr[q]).max() for q in ("S", "SP", "Srho", "Sv")}
    identical = all(np.array_equal(cloud[k].reshape(-1), grid[k].reshape(-1)) for k in OUTPUTS)
    print(f"{case} fp{8 * fb}: cloud against lattice, " + ", ".join(f"{q} {v:.3g}" for q, v in figures.items()) + f" (bar 1e-12); bit-identical: {identical}")
    for q, v in figures.items():
        assert v <= 1e-12, (q, v)
    # the two kernels stage the same doubles and walk them in the same order with the same arithmetic: measured bit-identical on
    # an MI355X in all five cases (profiles/sample_points.md), and held to it
    assert identical
    eng.close()


# ---- 5. stale lists -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fb", [8, 4])
def test_stale_lists(fb, request):
    """A fresh handle stopped after j steps (max_steps), for every j up to K: calls right behind a Δx-triggered rebuild and calls
    far behind one, where rows have drifted out of the cell `cstart` files them under."""
    p, s = _state("dam_break_2d", request)
    K = 110
    pts = None
    history = []
    for j in range(1, K + 1):
        eng = _engine(p, s, fb)
        if pts is None:
            F = p.Position[p.Type == 1].astype(np.float64)
            H = eng.cfg.H
            rng = np.random.default_rng(41)
            pts = rng.uniform(F.min(0) - 1.3 * H, F.max(0) + 1.3 * H, (260, 2)) + IRR[:2] * eng.cfg.dx
            pts[::5, 0] = (np.round(pts[::5, 0] / H) + 0.5) * H                    # every fifth on a cell face
        pr = eng.advance(1e9, max_steps=j)
        assert pr.iteration == j
        history.append(pr.n_rebuilds)
        _check_cloud(eng, pts, fb, f"step {j} (rebuilds so far {pr.n_rebuilds})")
        eng.close()
    rebuilt_before = [1] + [j for j in range(2, K + 1) if history[j - 1] > history[j - 2]]
    since = [j - max(b for b in rebuilt_before if b <= j) for j in range(1, K + 1)]
    print(f"fp{8 * fb}: rebuilds before steps {rebuilt_before}; longest stretch without one {max(since) + 1} steps")
    assert len(rebuilt_before) >= 2, "no Δx-triggered rebuild within the horizon"
    assert max(since) >= 10, "no checked call lies 10 steps behind the last rebuild"
    assert any(b > 1 for b in rebuilt_before)                                      # a checked call follows a Δx-triggered rebuild directly


# ---- 6. slabs in one handle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("case,fb,axis", [("dam_break_2d", 8, 0), ("dam_break_2d", 4, 0), ("dam_break_2d", 8, 1), ("dam_break_3d_shipped", 4, 0), ("dam_break_3d_shipped", 8, 1)])
def test_slabs_in_one_handle(case, fb, axis, world, request):
    """Every slab bins and samples the whole cloud over the rows it owns, the handle adds the raw sums in slab order.  Some points lie
    ON the first cut (the face between two slabs' cell columns), others 0.3·H to either side: a ghost copy that counted would
    double their sums, a skipped owner halve them.  The cloud is unsorted: entry p must stay the caller's point p."""
    p, s = _state(case, request)
    K = 60 if case == "dam_break_2d" else 20
    ref, dd = _engine(p, s, fb), _engine(p, s, fb, devices=[0] * world, slab_axis=axis)
    pr, pd = ref.advance(1e9, max_steps=K), dd.advance(1e9, max_steps=K)
    assert (pd.iteration, pd.steps_done, pd.n_rebuilds) == (pr.iteration, pr.steps_done, pr.n_rebuilds)
    info = dd.multi_info()
    assert info.world == world and info.n_local == world and info.axis == axis
    cfg = ref.cfg
    H, D = cfg.H, ref.D
    d0 = ref.download(FIELDS)
    F = d0["Position"][d0["Type"] == 1].astype(np.float64)
    cuts = [(c - 0.5) * H for c in info.cuts[:world - 1]]                          # cell column c covers |x/H - c| <= 1/2
    rng = np.random.default_rng(53)
    lo, hi = F.min(0) - 0.9 * H, F.max(0) + 0.9 * H
    pts = [rng.uniform(lo, hi, (500, D)) + IRR[:D] * cfg.dx]
    for xc in cuts:
        for shift in (0.0, -0.3 * H, 0.3 * H):
            q = rng.uniform(lo, hi, (30, D)) + IRR[:D] * cfg.dx
            q[:, axis] = xc + shift
            pts.append(q)
    pts = np.concatenate(pts)
    pts = pts[rng.permutation(len(pts))]
    one, refsum, _ = _check_cloud(ref, pts, fb, f"{case} one device")
    got = dd.sample_points(pts)
    ga, gb = _raw(_as_series(got), 0), _raw(_as_series(one), 0)
    tol = 1e-9 if fb == 8 else 1e-5
    figures = {q: np.abs(ga[q] - gb[q]).max() / np.abs(gb[q]).max() for q in ("S", "SP", "Srho", "Sv")}
    differ = ga["n"] != gb["n"]
    print(f"{case} fp{8 * fb} {world} slabs axis {axis}: {len(pts)} points, n differs at {int(differ.sum())}, near the cut {int(refsum['near'].sum())}; "
          + ", ".join(f"{q} {v:.3g}" for q, v in figures.items()) + f" (bar {tol:g})")
    assert not (differ & ~refsum["near"]).any() and differ.sum() <= 0.02 * len(differ)
    for q, v in figures.items():
        assert v <= tol, (q, v, tol)
    at_cut = np.abs(pts[:, axis] - cuts[0]) <= 0.3 * H + 1e-12
    assert at_cut.sum() >= 90 and (one["count"][at_cut] > 0).any()                 # points on and next to the cut lie in water
    _same_bits(dd.sample_points(pts), got, "slab order: the same bits every time")
    ref.close(); dd.close()


# ---- 7. does not disturb ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,fb", [("dam_break_2d", 4), ("dam_break_3d_shipped", 8)])
def test_does_not_disturb(case, fb, request):
    p, s = _state(case, request)
    F = p.Position[p.Type == 1]
    D = F.shape[1]
    calls = (40, 1, 33, 7) if D == 2 else (12, 1, 9)
    runs = []
    for sampled in (False, True):
        eng = _engine(p, s, fb)
        H = eng.cfg.H
        counts = np.array([21, 17] if D == 2 else [11, 9, 7], dtype=np.int64)
        origin = F.min(0) - 1.2 * H + IRR[:D] * eng.cfg.dx
        lattice = (origin, (F.max(0) + 1.2 * H - origin) / (counts - 1), counts)
        pts = np.random.default_rng(61).uniform(F.min(0) - 2 * H, F.max(0) + 2 * H, (900, D))
        probes = F[:: max(len(F) // 24, 1)][:24] + 0.3 * eng.cfg.dx
        eng.probes_enable(probes, capacity=200)
        prog, clouds = [], []
        for n in calls:
            q = eng.advance(1e9, max_steps=n)
            prog.append((q.iteration, q.steps_done, q.n_rebuilds, q.index_counter, q.total_time, q.last_dt, q.delta_x))
            if sampled:
                before = eng.sample_grid(*lattice)
                a = eng.sample_points(pts)
                after = eng.sample_grid(*lattice)
                for k in before:
                    np.testing.assert_array_equal(after[k], before[k], err_msg=k)  # the lattice's arena and result are its own
                part = eng.sample_points(pts, fields=("pressure",))                # … whichever fields are asked for
                np.testing.assert_array_equal(part["pressure"], a["pressure"])
                clouds.append(a)
        runs.append((prog, eng.download(), eng.probes_read(), clouds))
        if sampled:
            # a download begun before the call completes with the snapshot taken at its begin
            want = eng.download()
            spec = {k: np.zeros_like(want[k]) for k in ("Position", "Velocity", "Acceleration", "Density", "Pressure", "ID", "Type", "GroupMarker", "GhostPoints", "Cells")}
            fbeg = eng._fn("download_begin"); fbeg.argtypes = [C.c_void_p] * 11
            eng._check(fbeg(eng._h, *[spec[k].ctypes.data_as(C.c_void_p) for k in spec]))
            mid = eng.sample_points(pts)
            eng.advance(1e9, max_steps=3)
            eng.sample_points(pts)
            eng.download_end()
            for k in spec:
                np.testing.assert_array_equal(spec[k], want[k], err_msg=k)
            _same_bits(mid, clouds[-1], "the call saw the state of before the three steps")
        eng.close()
    assert runs[0][0] == runs[1][0]                                                # the progress blocks
    for k, v in runs[0][1].items():
        np.testing.assert_array_equal(runs[1][1][k], v, err_msg=k)                  # the downloads, bit for bit
    assert len(runs[0][2]["iteration"]) == sum(calls)
    for k in runs[0][2]:
        np.testing.assert_array_equal(runs[1][2][k], runs[0][2][k], err_msg=k)      # the probe series
    assert all(np.abs(c["weight"]).max() > 0.5 for c in runs[1][3])


# ---- 8. edges and errors ------------------------------------------------------------------------------------------------------
def test_edges(request):
    from sphexample_amd._abi import ERR_ARGUMENT, ERR_STATE, MAX_SAMPLE_POINTS, OK, SphmiError, make_config
    from sphexample_amd.engine import Engine, rccl_unique_id
    from test_probes_gpu import _variant
    p, s = _state("dam_break_2d", request)
    F = p.Position[p.Type == 1].astype(np.float64)
    pts = F[:: max(len(F) // 40, 1)][:40] + 0.013
    assert len(pts) == 40

    def status(e, x):
        with pytest.raises(SphmiError) as ei:
            e.sample_points(x)
        return ei.value.status, str(ei.value)
    cfg = make_config(len(p), s.SimConstants, s.SimKernel, s.SimMetaData, s.SimViscosity, s.SimDensityDiffusion, device_float_bytes=8, host_float_bytes=8)
    bare = Engine(cfg)
    assert status(bare, pts)[0] == ERR_STATE                                       # before the upload
    bare.close()
    eng = _engine(p, s, 8)
    assert status(eng, pts)[0] == ERR_STATE                                        # uploaded, no step yet: no cell list, no half-step set
    eng.advance(1e9, max_steps=5)
    ok = eng.sample_points(pts)
    assert ok["weight"].max() > 0.5
    # arguments
    f = eng._fn("sample_points"); f.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 6
    x = np.ascontiguousarray(pts)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)                                   # noqa: E731
    assert f(eng._h, len(x), None, *[None] * 5) == ERR_ARGUMENT                    # null positions with n_points > 0
    assert f(eng._h, -1, ptr(x), *[None] * 5) == ERR_ARGUMENT
    assert f(eng._h, MAX_SAMPLE_POINTS + 1, ptr(x), *[None] * 5) == ERR_ARGUMENT   # (refused before a coordinate is read)
    assert f(eng._h, 0, None, *[None] * 5) == OK and f(eng._h, 0, ptr(x), *[None] * 5) == OK      # n_points == 0 does nothing
    assert eng.sample_points(np.zeros((0, 2)))["velocity"].shape == (0, 3)
    assert f(eng._h, len(x), ptr(x), *[None] * 5) == OK                            # every output NULL
    for bad, where in ((np.nan, (17, 0)), (np.inf, (3, 1)), (-np.inf, (39, 1))):
        y = x.copy(); y[where] = bad
        if where[0] < 30:
            y[30, 1] = np.nan                                                      # a later one does not change the answer: the FIRST is named
        st, text = status(eng, y)
        assert st == ERR_ARGUMENT and f"point {where[0]}" in text, text
    for k in ok:
        np.testing.assert_array_equal(eng.sample_points(pts)[k], ok[k], err_msg=k)  # after refused calls: the same bits
    assert eng.advance(1e9, max_steps=2).steps_done == 2                           # … and the handle still steps
    # a new particle set: ERR_STATE until a step has run
    eng.upload_particles(p)
    assert status(eng, pts)[0] == ERR_STATE
    eng.advance(1e9, max_steps=1)
    assert eng.sample_points(pts)["weight"].max() > 0.5
    # handles with H < h
    thin = _engine(p, _variant(s, None, 0.9), 8)
    st, text = status(thin, pts)
    assert st == ERR_STATE and "H < h" in text
    thin.close()
    # rank-mode handles: one slab of the rows per process
    rk = _engine(p, s, 8, rank=0, world=1, unique_id=rccl_unique_id())
    st, text = status(rk, pts)
    assert st == ERR_STATE and "rank-mode" in text
    eng.close(); rk.close()


# ---- 9. RunSimulation ---------------------------------------------------------------------------------------------------------
def test_run_simulation_hands_the_cloud_to_the_callback(dam_break_2d):
    import copy
    from sphexample_amd import simulation
    from sphexample_amd.fields import segment
    p, s = dam_break_2d
    F = p.Position[p.Type == 1].astype(np.float64)
    line = segment(F.min(0) + 0.011, [F[:, 0].max() - 0.011, F[:, 1].max() + 0.3], 9)      # from the bottom of the column into the air above it

    def run(**kw):
        meta = copy.deepcopy(s.SimMetaData)
        meta.SimulationTime, meta.OutputTimes = 0.002, 0.001
        got = []
        steps = simulation.RunSimulation(SimGeometry=None, SimMetaData=meta, SimConstants=s.SimConstants, SimKernel=s.SimKernel, SimLogger=None,
                                         SimParticles=p.copy(), SimViscosity=s.SimViscosity, SimDensityDiffusion=s.SimDensityDiffusion,
                                         on_output=lambda m, pp, *extra: got.append((m.Iteration, extra)), **kw)
        return steps, got
    steps, got = run(sample_points=line)
    assert len(got) == len(steps) + 1 and got[0][1] == (None,)                     # one cloud per output; none before the first step
    for iteration, extra in got[1:]:
        (f,) = extra
        assert f["weight"].shape == f["pressure"].shape == f["density"].shape == f["count"].shape == (9,) and f["velocity"].shape == (9, 3)
        assert (f["weight"][1:5] > 0.5).all() and (f["count"][:5] > 0).all() and f["weight"][-1] == 0 and (f["pressure"][1:5] != 0).any()
    _, plain = run()
    assert len(plain) == len(got) and all(extra == () for _, extra in plain)       # the default: the callback's arguments as they were
