"""Pressure, density, velocity and fill sampled on a regular lattice (sphmi_sample_grid, csrc/sphmi_field_grid.h) — needs a real
MI355X.

Per node the sums are the probes' (tests/test_probes_gpu.py): over the Fluid rows j with |x_n - x_j|^2 <= H^2 on the state
sphmi_download delivers now, w_j = (m0 / rho_j) W(|x_n - x_j|), n = rows, S = sum w_j, SP, Srho, Sv.  The reference is the same
`brute_force_probes`, an O(M·N) numpy enumeration that never calls the code under test, fed the node coordinates of
`sphexample_amd.fields.grid_nodes` and a download taken right after the call.

Bars (the project's for a single evaluation, as in tests/test_probes_gpu.py): 1e-10 of the field maximum on every raw sum on fp64
handles, 2e-4 on fp32 handles; n equal at every node except — fp32 handles — nodes where the reference itself shows a Fluid row
within 1e-6·H of the cut, at most 2 % of the nodes, and the reference alone must stay inside that cap: the lattice origins are
incommensurate with the particle lattice.  Against the probe kernel: n equal with no exception, raw sums within 1e-12 (fp64).
Slab handles against the one-device handle: 1e-9 / 1e-5.
"""
import ctypes as C

import numpy as np
import pytest

from test_probes_gpu import FIELDS, _check_against, _engine, _raw, _state, _variant, brute_force_probes

pytestmark = pytest.mark.gpu

IRR = np.array([0.318309886, 0.577215665, 0.693147181])            # offsets in units of dp: nothing the particle lattice knows


def _as_series(out, dims):
    """The dict of sample_grid as ONE sample of a probe series: [1, nodes(, 3)] — what _raw and _check_against take."""
    return {k: v.reshape((1, -1) + v.shape[dims:]) for k, v in out.items()}


def _check_lattice(eng, lattice, fb, what, subset=None, fields=None):
    """Sample, download right after, enumerate.  Returns (out, ref)."""
    from sphexample_amd.fields import grid_nodes
    D = eng.D
    out = eng.sample_grid(*lattice)
    d = eng.download(FIELDS)
    nodes = grid_nodes(*lattice)
    assert out["weight"].shape == tuple(int(c) for c in lattice[2])[::-1] and out["velocity"].shape == out["weight"].shape + (3,)
    r = _as_series(out, D)
    if subset is not None:
        nodes = nodes[subset]
        r = {k: v[:, subset] for k, v in r.items()}
    ref = brute_force_probes(eng.cfg, nodes, d["Position"], d["Velocity"], d["Density"], d["Pressure"], d["Type"])
    _check_against(ref, _raw(r, 0), r, fb, what, k=0)
    if D == 2:
        assert (out["velocity"][..., 2] == 0).all()
    return out, ref, d


def _lattices(d, cfg):
    """The shapes of the issue, from a downloaded state: name → (origin, spacing, counts)."""
    X, T = d["Position"].astype(np.float64), d["Type"]
    D = X.shape[1]
    F = X[T == 1]
    H, dp = cfg.H, cfg.dx
    lo, hi = X.min(0), X.max(0)
    flo, fhi = F.min(0), F.max(0)
    irr = IRR[:D] * dp
    out = {}

    def span(a, b, s, cap):
        s = np.maximum(np.asarray(s, np.float64), (b - a) / (np.asarray(cap) - 1))          # coarsen where the count would pass the cap
        return a, s, np.ceil((b - a) / s).astype(np.int64) + 1             # the last node lies at or beyond b
    cap = 72 if D == 2 else 17
    # overhanging the particles' bounding grid on every side by more than three cells
    out["overhang"] = span(lo - 3.3 * H - irr, hi + 3.3 * H, np.full(D, 0.41 * H), np.full(D, cap))
    # anisotropic, over the fluid
    out["anisotropic"] = span(flo - 0.5 * H + irr, fhi + 0.5 * H, np.array([0.31, 1.27, 0.53])[:D] * H, np.full(D, cap))
    # spacing > H: bricks spanning several cells
    out["coarse"] = span(lo - 1.1 * H + irr, hi + 2.0 * H, np.full(D, 1.7 * H), np.full(D, 1000))
    # spacing < H/8: a brick inside one cell; at the top corner of the fluid, where the free surface is
    n_fine = 44 if D == 2 else 13
    fine = H / 9.3
    out["fine"] = (fhi - 0.6 * n_fine * fine + irr, np.full(D, fine), np.full(D, n_fine, dtype=np.int64))
    # a slice: one count = 1 (3-D: the plane y = const through the fluid; 2-D: a row)
    o, s, c = span(flo - H + irr, fhi + H, np.full(D, 0.23 * H), np.full(D, 90 if D == 2 else 60))
    o[1] = 0.5 * (flo[1] + fhi[1]) + irr[1]; c[1] = 1
    out["slice"] = (o, s, c)
    # a single node, in the fluid
    out["single"] = (F[len(F) // 2] + 0.37 * irr, np.full(D, 0.1 * H), np.ones(D, dtype=np.int64))
    return out


CASES = {  # name → (fixture, steps, kernel variant)
    "dam_break_2d": ("dam_break_2d", 30, None),
    "dam_break_3d_shipped": ("dam_break_3d_shipped", 12, None),
    "moving_square": ("moving_square", 25, None),                  # k < 2: H + h spans five cells per axis
    "cubic_spline": ("dam_break_2d", 20, "cubic"),
}


# ---- 1. equals the enumeration ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fb", [8, 4])
@pytest.mark.parametrize("case", list(CASES))
def test_equals_brute_force(case, fb, request):
    fixture, K, kernel = CASES[case]
    p, s = _state(fixture, request)
    if kernel:
        s = _variant(s, kernel, None)
    eng = _engine(p, s, fb)
    eng.advance(1e9, max_steps=K)
    d0 = eng.download(FIELDS)
    F = d0["Position"][d0["Type"] == 1]
    for name, lattice in _lattices(d0, eng.cfg).items():
        out, ref, d = _check_lattice(eng, lattice, fb, f"{case} {name} {tuple(int(c) for c in lattice[2])}")
        nodes_n = int(np.prod(lattice[2]))
        if name == "overhang":
            # nodes outside the particles' bounding grid read exact zeros, on every side
            from sphexample_amd.fields import grid_axes
            lo, hi = d["Position"].min(0) - 1.6 * eng.cfg.H, d["Position"].max(0) + 1.6 * eng.cfg.H
            for dim, a in enumerate(grid_axes(*lattice)):
                assert (a < lo[dim]).sum() >= 1 and (a > hi[dim]).sum() >= 1, (name, dim)
                axis = eng.D - 1 - dim
                for side in (a < lo[dim], a > hi[dim]):
                    for k in ("weight", "count", "pressure", "density", "velocity"):
                        assert (np.compress(side, out[k], axis=axis) == 0).all(), (name, dim, k)
            assert (ref["n"] > 0).sum() > 20
        if name == "fine":
            assert (lattice[1] < eng.cfg.H / 8).all() and (ref["n"] > 0).sum() > 0.2 * nodes_n and (ref["n"] == 0).any()
        if name == "coarse":
            assert (lattice[1] > eng.cfg.H).all() and (ref["n"] > 0).sum() >= 3
        if name == "slice":
            assert 1 in [int(c) for c in lattice[2]] and (ref["S"] > 0.5).any()
        if name == "single":
            assert nodes_n == 1 and ref["n"][0] > 0 and out["weight"].reshape(-1)[0] > 0.1
    eng.close()


@pytest.mark.parametrize("fb", [4, 8])
def test_a_million_nodes(fb, request):
    """The 3-D Dp 0.02 case under a lattice of 1.06 M nodes over the whole tank: a fixed pseudo-random subset of 4 096 nodes against
    the enumeration, and every node farther than H from the box round the Fluid rows exactly zero."""
    from sphexample_amd.fields import grid_nodes
    p, s = _state("dam_break_3d_shipped", request)
    eng = _engine(p, s, fb)
    eng.advance(1e9, max_steps=12)
    d0 = eng.download(FIELDS)
    X = d0["Position"]
    H, dp = eng.cfg.H, eng.cfg.dx
    counts = np.array([160, 66, 100], dtype=np.int64)
    origin = X.min(0) - 0.7 * H - IRR * dp
    spacing = (X.max(0) + 1.3 * H - origin) / (counts - 1)
    lattice = (origin, spacing, counts)
    assert np.prod(counts) >= 10 ** 6
    subset = np.sort(np.random.default_rng(20240229).choice(int(np.prod(counts)), 4096, replace=False))
    out, ref, d = _check_lattice(eng, lattice, fb, f"1.06 M nodes, subset of {len(subset)}", subset=subset)
    assert (ref["n"] > 0).sum() > 300 and (ref["n"] == 0).sum() > 300
    F = d["Position"][d["Type"] == 1].astype(np.float64)
    nodes = grid_nodes(*lattice)
    far = ((nodes < F.min(0) - H * (1 + 1e-9)) | (nodes > F.max(0) + H * (1 + 1e-9))).any(1)
    assert far.sum() > 10 ** 5
    for k in ("weight", "count", "pressure", "density"):
        assert (out[k].reshape(-1)[far] == 0).all(), k
    assert (out["velocity"].reshape(-1, 3)[far] == 0).all()
    assert (out["count"].reshape(-1)[~far] > 0).sum() > 10 ** 4
    eng.close()


# ---- 2. stale lists -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fb", [8, 4])
def test_stale_lists(fb, request):
    """A fresh handle stopped after j steps (max_steps), for every j up to K: calls right behind a Δx-triggered rebuild and calls
    far behind one, where rows have drifted out of the cell `cstart` files them under."""
    p, s = _state("dam_break_2d", request)
    K = 110
    lattice = None
    history = []
    for j in range(1, K + 1):
        eng = _engine(p, s, fb)
        if lattice is None:
            F = p.Position[p.Type == 1]
            H = eng.cfg.H
            origin = F.min(0) - 1.3 * H + IRR[:2] * eng.cfg.dx
            counts = np.array([19, 17], dtype=np.int64)
            lattice = (origin, (F.max(0) + 1.3 * H - origin) / (counts - 1), counts)
        pr = eng.advance(1e9, max_steps=j)
        assert pr.iteration == j
        history.append(pr.n_rebuilds)
        _check_lattice(eng, lattice, fb, f"step {j} (rebuilds so far {pr.n_rebuilds})")
        eng.close()
    rebuilt_before = [1] + [j for j in range(2, K + 1) if history[j - 1] > history[j - 2]]
    since = [j - max(b for b in rebuilt_before if b <= j) for j in range(1, K + 1)]
    print(f"fp{8 * fb}: rebuilds before steps {rebuilt_before}; longest stretch without one {max(since) + 1} steps")
    assert len(rebuilt_before) >= 2, "no Δx-triggered rebuild within the horizon"
    assert max(since) >= 10, "no checked call lies 10 steps behind the last rebuild"
    assert any(b > 1 for b in rebuilt_before)                                      # a checked call follows a Δx-triggered rebuild directly


# ---- 3. agrees with the probes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,fb", [("dam_break_2d", 8), ("dam_break_2d", 4), ("dam_break_3d_shipped", 8), ("dam_break_3d_shipped", 4), ("moving_square", 8)])
def test_agrees_with_the_probes(case, fb, request):
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
    eng.probes_enable(nodes, capacity=4)
    eng.advance(1e9, max_steps=25 if D == 2 else 10)
    pr = _raw(eng.probes_read())
    gr = _raw(_as_series(eng.sample_grid(*lattice), D), 0)
    np.testing.assert_array_equal(gr["n"], pr["n"])                                # the same r² arithmetic: no exception
    assert (pr["n"] > 0).sum() > 100
    tol = 1e-12 if fb == 8 else 2e-4
    figures = {q: np.abs(gr[q] - pr[q]).max() / np.abs(pr[q]).max() for q in ("S", "SP", "Srho", "Sv")}
    print(f"{case} fp{8 * fb}: lattice against probes, " + ", ".join(f"{q} {v:.3g}" for q, v in figures.items()) + f" (bar {tol:g})")
    for q, v in figures.items():
        assert v <= tol, (q, v, tol)
    eng.close()


# ---- 4. does not disturb, and repeats -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,fb", [("dam_break_2d", 4), ("dam_break_2d", 8), ("dam_break_3d_shipped", 4), ("still_wedge", 8)])
def test_does_not_disturb_and_repeats(case, fb, request):
    p, s = _state(case, request, vel=1.0 if case == "still_wedge" else 3.0)
    markers = sorted(int(m) for m in np.unique(p.GroupMarker))
    F = p.Position[p.Type == 1]
    D = F.shape[1]
    calls = (40, 1, 33, 7)
    runs = []
    for sampled in (False, True):
        eng = _engine(p, s, fb)
        H = eng.cfg.H
        counts = np.array([41, 37] if D == 2 else [21, 17, 13], dtype=np.int64)
        origin = F.min(0) - 1.2 * H + IRR[:D] * eng.cfg.dx
        lattice = (origin, (F.max(0) + 1.2 * H - origin) / (counts - 1), counts)
        probes = F[:: max(len(F) // 24, 1)][:24] + 0.3 * eng.cfg.dx
        eng.group_forces_enable(markers, capacity=200)
        eng.probes_enable(probes, capacity=200)
        prog, fields = [], []
        for n in calls:
            q = eng.advance(1e9, max_steps=n)
            prog.append((q.iteration, q.steps_done, q.n_rebuilds, q.index_counter, q.total_time, q.last_dt, q.delta_x))
            if sampled:
                a = eng.sample_grid(*lattice)
                b = eng.sample_grid(*lattice)                                      # no step in between: the same bits
                for k in a:
                    np.testing.assert_array_equal(a[k], b[k], err_msg=k)
                part = eng.sample_grid(*lattice, fields=("pressure",))             # … whichever fields are asked for
                np.testing.assert_array_equal(part["pressure"], a["pressure"])
                fields.append(a)
        runs.append((prog, eng.download(), eng.group_forces_read(), eng.probes_read(), fields))
        if sampled:
            # a download begun before the call completes with the snapshot taken at its begin
            want = eng.download()
            spec = {k: np.zeros_like(want[k]) for k in ("Position", "Velocity", "Acceleration", "Density", "Pressure", "ID", "Type", "GroupMarker", "GhostPoints", "Cells")}
            fbeg = eng._fn("download_begin"); fbeg.argtypes = [C.c_void_p] * 11
            eng._check(fbeg(eng._h, *[spec[k].ctypes.data_as(C.c_void_p) for k in spec]))
            mid = eng.sample_grid(*lattice)
            eng.advance(1e9, max_steps=3)
            eng.sample_grid(*lattice)
            eng.download_end()
            for k in spec:
                np.testing.assert_array_equal(spec[k], want[k], err_msg=k)
            for k in mid:
                np.testing.assert_array_equal(mid[k], fields[-1][k], err_msg=k)    # … and the call saw the state of before the three steps
        eng.close()
    assert runs[0][0][-1][2] >= len(calls)
    assert runs[0][0] == runs[1][0]                                                # the progress blocks
    for k, v in runs[0][1].items():
        np.testing.assert_array_equal(runs[1][1][k], v, err_msg=k)                  # the downloads, bit for bit
    for a, b in zip(runs[0][2], runs[1][2]):
        np.testing.assert_array_equal(a, b)                                         # the group-force series
    assert len(runs[0][3]["iteration"]) == sum(calls)
    for k in runs[0][3]:
        np.testing.assert_array_equal(runs[1][3][k], runs[0][3][k], err_msg=k)      # the probe series
    assert all(np.abs(f["weight"]).max() > 0.5 for f in runs[1][4])


# ---- 5. slabs in one handle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("case,fb,axis", [("dam_break_2d", 8, 0), ("dam_break_2d", 4, 0), ("dam_break_2d", 8, 1), ("dam_break_3d_shipped", 4, 0), ("dam_break_3d_shipped", 8, 1)])
def test_slabs_in_one_handle(case, fb, axis, world, request):
    """Every slab samples the whole lattice over the rows it owns, the handle adds the raw sums in slab order.  One node plane lies
    ON the first cut (the face between two slabs' cell columns), its neighbours 0.3·H to either side: a ghost copy that counted
    would double their sums, a skipped owner halve them."""
    from sphexample_amd.fields import grid_axes
    p, s = _state(case, request)
    K = 60 if case == "dam_break_2d" else 20
    ref, dd = _engine(p, s, fb), _engine(p, s, fb, devices=[0] * world, slab_axis=axis)
    pr, pd = ref.advance(1e9, max_steps=K), dd.advance(1e9, max_steps=K)
    assert (pd.iteration, pd.steps_done, pd.n_rebuilds) == (pr.iteration, pr.steps_done, pr.n_rebuilds)
    info = dd.multi_info()
    assert info.world == world and info.n_local == world and info.axis == axis
    assert sum(info.n_live[:world]) > len(p)                                       # ghost copies are held
    cfg = ref.cfg
    H, D = cfg.H, ref.D
    d0 = ref.download(FIELDS)
    F = d0["Position"][d0["Type"] == 1].astype(np.float64)
    cuts = [(c - 0.5) * H for c in info.cuts[:world - 1]]                          # cell column c covers |x/H - c| <= 1/2
    spacing = np.full(D, 0.47 * H); spacing[axis] = 0.3 * H
    origin = F.min(0) - 0.9 * H + IRR[:D] * cfg.dx
    origin[axis] = min(origin[axis], cuts[0] - 0.9 * H)
    m = int(np.ceil((cuts[0] - origin[axis]) / spacing[axis]))
    origin[axis] = cuts[0] - m * spacing[axis]                                     # node plane m on the first cut (to a rounding)
    counts = np.minimum(np.floor((F.max(0) + 0.9 * H - origin) / spacing).astype(np.int64) + 1, 70 if D == 2 else 16)
    counts[axis] = int(np.floor((max(F[:, axis].max(), cuts[-1]) + 0.9 * H - origin[axis]) / spacing[axis])) + 1
    lattice = (origin, spacing, counts)
    a = grid_axes(*lattice)[axis]
    for xc in cuts:
        assert np.abs(a - xc).min() <= 0.15 * H + 1e-12                            # a node plane on or next to every cut
    assert abs(a[m] - cuts[0]) <= 1e-12
    # the one-device handle against the enumeration, the slab handle against the one-device handle
    one, refsum, _ = _check_lattice(ref, lattice, fb, f"{case} one device")
    got = dd.sample_grid(*lattice)
    ga, gb = _raw(_as_series(got, D), 0), _raw(_as_series(one, D), 0)
    tol = 1e-9 if fb == 8 else 1e-5
    figures = {}
    for q in ("S", "SP", "Srho", "Sv"):
        scale = np.abs(gb[q]).max()
        figures[q] = np.abs(ga[q] - gb[q]).max() / scale
    differ = ga["n"] != gb["n"]
    print(f"{case} fp{8 * fb} {world} slabs axis {axis}: lattice {tuple(int(c) for c in counts)}, n differs at {int(differ.sum())}, near the cut {int(refsum['near'].sum())}; "
          + ", ".join(f"{q} {v:.3g}" for q, v in figures.items()) + f" (bar {tol:g})")
    assert not (differ & ~refsum["near"]).any() and differ.sum() <= 0.02 * len(differ)
    for q, v in figures.items():
        assert v <= tol, (q, v, tol)
    planes = np.flatnonzero(np.min(np.abs(a[:, None] - np.array(cuts)[None, :]), axis=1) <= 0.3 * H + 1e-12)
    assert m in planes and (np.take(one["count"], planes, axis=D - 1 - axis) > 0).any()      # planes on and next to the cuts run through water
    again = dd.sample_grid(*lattice)
    for k in got:
        np.testing.assert_array_equal(again[k], got[k], err_msg=k)                  # slab order: the same bits every time
    ref.close(); dd.close()


# ---- 6. edges and errors ------------------------------------------------------------------------------------------------------
def test_edges(request):
    from sphexample_amd._abi import ERR_ARGUMENT, ERR_DEVICE, ERR_STATE, MAX_GRID_NODES, OK, SphmiError, make_config
    from sphexample_amd.engine import Engine, rccl_unique_id
    p, s = _state("dam_break_2d", request)
    F = p.Position[p.Type == 1]
    lattice = (F.min(0) + 0.013, np.array([0.05, 0.04]), np.array([6, 5], dtype=np.int64))

    def status(e, *lat, **kw):
        with pytest.raises(SphmiError) as ei:
            e.sample_grid(*lat, **kw)
        return ei.value.status
    cfg = make_config(len(p), s.SimConstants, s.SimKernel, s.SimMetaData, s.SimViscosity, s.SimDensityDiffusion, device_float_bytes=8, host_float_bytes=8)
    bare = Engine(cfg)
    assert status(bare, *lattice) == ERR_STATE                                     # before the upload
    bare.close()
    eng = _engine(p, s, 8)
    assert status(eng, *lattice) == ERR_STATE                                      # uploaded, no step yet: no cell list, no half-step set
    eng.advance(1e9, max_steps=5)
    ok = eng.sample_grid(*lattice)
    assert ok["weight"].max() > 0.5
    # arguments
    f = eng._fn("sample_grid"); f.argtypes = [C.c_void_p] * 9
    o, sp, c = [np.ascontiguousarray(a, dtype=t) for a, t in zip(lattice, (np.float64, np.float64, np.int64))]
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)                                   # noqa: E731
    assert f(eng._h, None, ptr(sp), ptr(c), *[None] * 5) == ERR_ARGUMENT
    assert f(eng._h, ptr(o), None, ptr(c), *[None] * 5) == ERR_ARGUMENT
    assert f(eng._h, ptr(o), ptr(sp), None, *[None] * 5) == ERR_ARGUMENT
    assert f(eng._h, ptr(o), ptr(sp), ptr(c), *[None] * 5) == OK                   # every output NULL
    for bad in ([np.nan, 0.0], [0.0, np.inf], [-np.inf, 0.0]):
        assert status(eng, bad, lattice[1], lattice[2]) == ERR_ARGUMENT            # non-finite origin
    for bad in ([0.0, 0.1], [0.1, -0.1], [np.nan, 0.1], [0.1, np.inf]):
        assert status(eng, lattice[0], bad, lattice[2]) == ERR_ARGUMENT            # spacing not finite and positive
    for bad in ([0, 4], [4, -1], [MAX_GRID_NODES, 2], [4097, 4096], [1 << 40, 1 << 40]):
        assert status(eng, lattice[0], lattice[1], bad) == ERR_ARGUMENT            # a count < 1, a product above the cap
    # the product exactly at the cap passes the argument check (the arena: 7 doubles per node, 0.94 GB)
    big = np.array([4096, 4096], dtype=np.int64)
    assert int(np.prod(big)) == MAX_GRID_NODES
    rc = f(eng._h, ptr(o), ptr(np.array([1e-4, 1e-4])), ptr(big), *[None] * 5)
    if rc == ERR_DEVICE:
        pytest.skip("the device cannot hold the arena of 2^24 nodes: " + (eng._fn("last_error")(eng._h) or b"").decode())
    assert rc == OK
    w = eng.sample_grid(lattice[0], [1e-4, 1e-4], big, fields=("count",))["count"]
    assert w.shape == (4096, 4096) and w.max() > 0
    again = eng.sample_grid(*lattice)                                              # a small lattice behind the big one, in the grown arena
    for k in ok:
        np.testing.assert_array_equal(again[k], ok[k], err_msg=k)
    # a new particle set: ERR_STATE until a step has run
    eng.upload_particles(p)
    assert status(eng, *lattice) == ERR_STATE
    eng.advance(1e9, max_steps=1)
    assert eng.sample_grid(*lattice)["weight"].max() > 0.5
    # handles with H < h
    thin = _engine(p, _variant(s, None, 0.9), 8)
    with pytest.raises(SphmiError) as ei:
        thin.sample_grid(*lattice)
    assert ei.value.status == ERR_STATE and "H < h" in str(ei.value)
    thin.close()
    # rank-mode handles: one slab of the rows per process
    rk = _engine(p, s, 8, rank=0, world=1, unique_id=rccl_unique_id())
    with pytest.raises(SphmiError) as ei:
        rk.sample_grid(*lattice)
    assert ei.value.status == ERR_STATE and "rank-mode" in str(ei.value)
    eng.close(); rk.close()


# ---- 7. the free-surface height -----------------------------------------------------------------------------------------------
def test_surface_height_of_the_generated_reservoir():
    """3-D generator case, a few steps in: over the reservoir the height read off the lattice lies within 1.5·dp of the column's
    top layer (the bound of test_probes_gpu.py::test_generator_disables_and_serves_a_gauge); over the dry floor it is the base."""
    from sphexample_amd._abi import ERR_STATE, SphmiError
    from sphexample_amd.cases import setup_dam_break_3d
    from sphexample_amd.engine import make_generated_dam_break_engine
    from sphexample_amd.fields import grid_axes, surface_height
    dp = 0.02
    eng = make_generated_dam_break_engine(dp, setup_dam_break_3d(dp), device_float_bytes=4)
    d = eng.download(FIELDS)
    F = d["Position"][d["Type"] == 1]
    H = eng.cfg.H
    origin = np.array([F[:, 0].min() + 0.31 * dp, F[:, 1].min() + 0.57 * dp, F[:, 2].min()])
    spacing = np.array([1.7 * dp, 1.9 * dp, dp / 2])
    counts = np.array([int(1.2 / spacing[0]), int((F[:, 1].max() - F[:, 1].min()) / spacing[1]), int(2 * (F[:, 2].max() - F[:, 2].min()) / spacing[2])], dtype=np.int64)
    with pytest.raises(SphmiError) as ei:                                          # the generator leaves no cell list either
        eng.sample_grid(origin, spacing, counts)
    assert ei.value.status == ERR_STATE
    eng.advance(1e9, max_steps=3)
    out = eng.sample_grid(origin, spacing, counts, fields=("weight",))
    eta = surface_height(out["weight"], origin, spacing)
    assert eta.shape == (counts[1], counts[0])
    now = eng.download(("Position", "Type"))
    Fn = now["Position"][now["Type"] == 1]
    top = Fn[:, 2].max()
    x, y, z = grid_axes(origin, spacing, counts)
    wet = (x <= Fn[:, 0].max() - H)[None, :] & ((y >= Fn[:, 1].min() + H) & (y <= Fn[:, 1].max() - H))[:, None]
    dry = np.broadcast_to((x >= Fn[:, 0].max() + 2 * H)[None, :], eta.shape)
    print(f"surface height: {int(wet.sum())} columns over the reservoir, eta in [{eta[wet].min()}, {eta[wet].max()}], top particle {top}; {int(dry.sum())} dry columns")
    assert wet.sum() > 50 and dry.sum() > 50
    assert (np.abs(eta[wet] - top) <= 1.5 * dp).all()
    assert (eta[dry] == z[0]).all()
    eng.close()


# ---- 8. RunSimulation ---------------------------------------------------------------------------------------------------------
def test_run_simulation_hands_the_fields_to_the_callback(dam_break_2d):
    import copy
    from sphexample_amd import simulation
    from sphexample_amd.fields import grid_nodes
    p, s = dam_break_2d
    meta = copy.deepcopy(s.SimMetaData)
    meta.SimulationTime, meta.OutputTimes = 0.002, 0.001
    F = p.Position[p.Type == 1]
    lattice = (F.min(0) + 0.011, (F.max(0) - F.min(0)) / 7 * np.array([1.0, 2.0]), np.array([8, 9], dtype=np.int64))       # the upper half is air
    got = []
    steps = simulation.RunSimulation(SimGeometry=None, SimMetaData=meta, SimConstants=s.SimConstants, SimKernel=s.SimKernel, SimLogger=None,
                                     SimParticles=p.copy(), SimViscosity=s.SimViscosity, SimDensityDiffusion=s.SimDensityDiffusion,
                                     field_grid=lattice, probes=F[:2], on_output=lambda m, pp, pr, f: got.append((m.Iteration, pr, f)))
    assert len(got) == len(steps) + 1 and got[0][2] is None                        # one field set per output; none before the first step
    nodes = grid_nodes(*lattice)
    inside = ((nodes > F.min(0) + 0.05) & (nodes < F.max(0) - 0.05)).all(1).reshape(9, 8)
    assert inside.sum() >= 6
    for iteration, pr, f in got[1:]:
        assert int(pr["iteration"][-1]) == iteration                               # behind the probes
        assert f["weight"].shape == f["pressure"].shape == f["density"].shape == f["count"].shape == (9, 8) and f["velocity"].shape == (9, 8, 3)
        assert (f["weight"][inside] > 0.5).all() and (f["count"][inside] > 0).all() and (f["weight"][-1] == 0).all() and (f["pressure"][inside] != 0).any()
