"""Pressure, density and velocity sampled at fixed probe points on every step (sphmi_probes_enable / sphmi_probes_read,
csrc/sphmi_probes.h) — needs a real MI355X.

    over the Fluid rows j with |x_p - x_j|^2 <= H^2 on the state sphmi_download delivers directly after the step:
    w_j = (m0 / rho_j) W(|x_p - x_j|),   n = rows,   S = sum w_j,   SP = sum w_j P_j,   Srho = sum w_j rho_j,   Sv = sum w_j v_j

The reference is `brute_force_probes` below: an O(M·N) numpy enumeration in fp64 written from that definition — the kernel
formulas of src/SPHKernels.jl:75-91, `eos` of tests/bruteforce.py for the cross-check of the delivered Pressure — fed the arrays
sphmi_download returns after the sampled step.  It never calls the code under test (tests/test_probes_host.py pins it to a
closed form).

Bars (the project's bars for a single evaluation, tests/test_engine_gpu.py::test_single_force_evaluation): 1e-10 of the field
maximum on fp64 handles, 2e-4 on fp32 handles, for the raw sums S, S·P, S·rho, S·v over the probe set and for the normalised
values at the probes with S >= 0.5.  n must be equal; on fp32 handles a probe is excused when the reference shows a row
within 1e-6·H of the cut for it, at most 2 % of the probes — and the reference alone must stay inside that cap.

The stock layouts start at rest: the cases run from `perturbed(p, seed=3, vel_scale=3.0)`, which crosses Δx-triggered rebuilds
within tens of steps (asserted from sphmi_progress.n_rebuilds).
"""
import numpy as np
import pytest

from bruteforce import eos
from conftest import perturbed

pytestmark = pytest.mark.gpu

BAR = {8: 1e-10, 4: 2e-4}


# ---- the reference ------------------------------------------------------------------------------------------------------
def kernel_w(cfg, q):
    """W(q) of src/SPHKernels.jl:75-78 (Wendland C2) and :89-92 (CubicSpline); cfg.kernel: 0 / 1 as in include/sphmi.h."""
    q = np.asarray(q, dtype=np.float64)
    if cfg.kernel == 1:
        return cfg.alphaD * ((1 - 1.5 * q ** 2 + 0.75 * q ** 3) * ((0 <= q) & (q <= 1)) + 0.25 * (2 - q) ** 3 * ((1 < q) & (q <= 2)))
    return cfg.alphaD * (1 - q / 2) ** 4 * (2 * q + 1)


def brute_force_probes(cfg, probes, pos, vel, rho, press, typ):
    """Every probe against every row.  Returns n [M], S, SP, Srho [M], Sv [M, 3] and near [M]: a row of the probe lies within
    1e-6·H of the cut."""
    probes, pos, vel = np.asarray(probes, np.float64), np.asarray(pos, np.float64), np.asarray(vel, np.float64)
    M, D = probes.shape
    fluid = np.asarray(typ) == 1
    x, v, r, p = pos[fluid], vel[fluid], np.asarray(rho, np.float64)[fluid], np.asarray(press, np.float64)[fluid]
    out = {"n": np.zeros(M, np.int64), "S": np.zeros(M), "SP": np.zeros(M), "Srho": np.zeros(M), "Sv": np.zeros((M, 3)), "near": np.zeros(M, bool)}
    for k in range(M):
        d = probes[k][None, :] - x
        r2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
        if D == 3:
            r2 = r2 + d[:, 2] * d[:, 2]
        dist = np.sqrt(r2)
        out["near"][k] = (np.abs(dist - cfg.H) <= 1e-6 * cfg.H).any()
        sel = r2 <= cfg.H2
        w = (cfg.m0 / r[sel]) * kernel_w(cfg, dist[sel] * cfg.h_inv)
        out["n"][k] = sel.sum()
        out["S"][k] = w.sum(); out["SP"][k] = (w * p[sel]).sum(); out["Srho"][k] = (w * r[sel]).sum()
        out["Sv"][k, :D] = (w[:, None] * v[sel]).sum(0)
    return out


# ---- helpers --------------------------------------------------------------------------------------------------------------
def _state(case, request, vel=3.0):
    p0, s = request.getfixturevalue(case)
    p = perturbed(p0, seed=3, vel_scale=vel)
    if hasattr(p0, "geometries"):
        p.geometries = p0.geometries
    return p, s


def _engine(p, s, fb, **kw):
    from sphexample_amd.engine import make_engine
    return make_engine(p, s, device_float_bytes=fb, **kw)


FIELDS = ("Position", "Velocity", "Density", "Pressure", "Type")


def _reference(eng, probes, d=None):
    d = d or eng.download(FIELDS)
    return brute_force_probes(eng.cfg, probes, d["Position"], d["Velocity"], d["Density"], d["Pressure"], d["Type"])


def _raw(r, k=-1):
    """The raw sums of sample k of a probes_read(): S, S·P, S·rho, S·v."""
    S = r["weight"][k]
    return {"n": r["count"][k], "S": S, "SP": S * r["pressure"][k], "Srho": S * r["density"][k], "Sv": S[:, None] * r["velocity"][k]}


def _check_against(ref, got, r, fb, what, k=-1):
    """The bars of the module docstring; prints every figure before it asserts."""
    tol = BAR[fb]
    M = len(ref["n"])
    figures = {}
    for q in ("S", "SP", "Srho", "Sv"):
        scale = np.abs(ref[q]).max()
        figures[q] = np.abs(got[q] - ref[q]).max() / scale if scale > 0 else np.abs(got[q]).max()
    inside = ref["S"] >= 0.5
    norm = {"pressure": ref["SP"], "density": ref["Srho"]}
    for q, raw in norm.items():
        want = raw[inside] / ref["S"][inside]
        figures[q] = np.abs(r[q][k][inside] - want).max() / np.abs(want).max() if inside.any() and np.abs(want).max() > 0 else 0.0
    wantv = ref["Sv"][inside] / ref["S"][inside][:, None]
    figures["velocity"] = np.abs(r["velocity"][k][inside] - wantv).max() / np.abs(wantv).max() if inside.any() and np.abs(wantv).max() > 0 else 0.0
    differ = got["n"] != ref["n"]
    print(f"{what} fp{8 * fb}: {M} probes, {int(inside.sum())} with S >= 0.5, n differs at {int(differ.sum())}, near the cut {int(ref['near'].sum())}; "
          + ", ".join(f"{q} {v:.3g}" for q, v in figures.items()) + f" (bar {tol:g})")
    assert ref["near"].sum() <= 0.02 * M, "the probe set itself has too many probes with a row at the cut"
    if fb == 8:
        assert not differ.any(), np.flatnonzero(differ)
    else:
        assert not (differ & ~ref["near"]).any(), np.flatnonzero(differ & ~ref["near"])      # excused only where the reference shows a row at the cut
        assert differ.sum() <= 0.02 * M
    for q, v in figures.items():
        assert v <= tol, (what, q, v, tol)
    empty = ref["n"] == 0
    assert (got["S"][empty] == 0).all() and (got["n"][empty] == 0).all()
    for q in ("pressure", "density"):
        assert (r[q][k][empty] == 0).all()
    assert (r["velocity"][k][empty] == 0).all()


def _probe_set(d, cfg, seed=5):
    """From a downloaded state: inside the fluid, at the free surface, inside a wall, on cell faces, exactly on particles, outside
    the grid, in empty space.  Returns (points [M, D], slices by kind)."""
    rng = np.random.default_rng(seed)
    X, T = d["Position"].astype(np.float64), d["Type"]
    D = X.shape[1]
    F, B = X[T == 1], X[T != 1]
    H, dp = cfg.H, cfg.dx
    kinds = {}
    pts = []

    def add(name, a):
        a = np.asarray(a, np.float64).reshape(-1, D)
        kinds[name] = slice(sum(len(x) for x in pts), sum(len(x) for x in pts) + len(a))
        pts.append(a)
    pick = rng.choice(len(F), 40, replace=False)
    add("fluid", F[pick[:24]] + rng.uniform(-dp, dp, (24, D)))
    add("on_fluid_particle", F[pick[24:36]])
    add("on_wall_particle", B[rng.choice(len(B), 8, replace=False)])
    top = F[np.argsort(F[:, -1])[-8:]].copy(); top[:, -1] += 0.5 * dp
    add("surface", top)
    face = F[pick[36:40]].copy()
    face[:, 0] = (np.round(face[:, 0] / H) + 0.5) * H                               # cell c covers |x/H - c| <= 1/2 (map_floor rounds): a face
    allf = (np.round(F[pick[:2]] / H) + 0.5) * H                                   # … and a cell corner
    add("cell_face", np.concatenate([face, allf]))
    lo, hi = X.min(0), X.max(0)
    far = np.array([lo - 100.0, hi + 100.0, lo - 3 * H, hi + 3 * H, np.r_[hi[0] + 1e6, lo[1:]]])
    add("outside_grid", far)
    above = np.tile(F.mean(0), (3, 1)); above[:, -1] = F[:, -1].max() + np.array([1.5, 3.0, 6.0]) * H
    add("empty", above)
    return np.concatenate(pts), kinds


def _variant(s, kernel=None, k=None):
    import dataclasses
    from sphexample_amd import CubicSpline, SPHKernelInstance, WendlandC2
    D = s.SimMetaData.Dimensions
    kern = SPHKernelInstance(D, CubicSpline(0.2) if kernel == "cubic" else WendlandC2(), h=s.SimKernel.h, k=k or s.SimKernel.k)
    return dataclasses.replace(s, SimKernel=kern)


CASES = {  # name → (fixture, steps, kernel variant, k)
    "dam_break_2d": ("dam_break_2d", 30, None, None),
    "dam_break_3d_shipped": ("dam_break_3d_shipped", 12, None, None),
    "moving_square": ("moving_square", 25, None, None),
    "dam_break_2d_mdbc": ("dam_break_2d_mdbc", 20, None, None),
    "cubic_spline": ("dam_break_2d", 20, "cubic", None),
    "cubic_spline_k1.5": ("dam_break_2d", 20, "cubic", 1.5),
}


# ---- 1. the last sample equals brute force -------------------------------------------------------------------------------
@pytest.mark.parametrize("fb", [8, 4])
@pytest.mark.parametrize("case", list(CASES))
def test_last_sample_equals_brute_force(case, fb, request):
    fixture, K, kernel, k = CASES[case]
    p, s = _state(fixture, request, vel=1.0 if fixture == "dam_break_2d_mdbc" else 3.0)
    if kernel or k:
        s = _variant(s, kernel, k)
    # a first run tells where the particles are after K steps: probes ON particles, at the surface, on the faces of occupied cells
    scout = _engine(p, s, fb)
    scout.advance(1e9, max_steps=K)
    d0 = scout.download()
    scout.close()
    probes, kinds = _probe_set(d0, scout.cfg)
    eng = _engine(p, s, fb)
    eng.probes_enable(probes, capacity=K + 4)
    pr = eng.advance(1e9, max_steps=K)
    assert pr.iteration == K
    r = eng.probes_read()
    assert len(r["iteration"]) == K and eng.probes_dropped == 0 and r["weight"].shape == (K, len(probes)) and r["velocity"].shape == (K, len(probes), 3)
    assert (int(r["iteration"][-1]), float(r["time"][-1]), float(r["dt"][-1])) == (pr.iteration, pr.total_time, pr.last_dt)
    d = eng.download()
    for f in d0:
        np.testing.assert_array_equal(d[f], d0[f], err_msg=f)                       # the sampled run IS the scouted run
    # the Pressure the download delivers is Pressure!(rho) of the half step: the same order of magnitude as eos(Density), not the same values
    fluid = d["Type"] == 1
    assert np.abs(d["Pressure"][fluid]).max() <= 10 * max(np.abs(eos(eng.cfg, d["Density"][fluid])).max(), 1.0)
    ref, got = _reference(eng, probes, d), _raw(r)
    _check_against(ref, got, r, fb, case)
    # the kinds are what they say
    assert (ref["n"][kinds["fluid"]] > 0).all() and (ref["S"][kinds["fluid"]] > 0.1).any()
    assert (ref["n"][kinds["on_fluid_particle"]] > 0).all()
    assert (ref["n"][kinds["outside_grid"]] == 0).all() and (ref["n"][kinds["empty"]] == 0).all()
    assert (got["S"][kinds["outside_grid"]] == 0).all() and (got["S"][kinds["empty"]] == 0).all()
    s_surface = ref["S"][kinds["surface"]]
    assert (s_surface > 0).all() and s_surface.min() < 0.8, s_surface
    if p.Position.shape[1] == 2:
        assert (r["velocity"][:, :, 2] == 0).all()
    eng.close()


# ---- 2. stale lists, and 3. every executed step ---------------------------------------------------------------------------
def _lattice_probes(p, cfg, n=12):
    """A fixed set over the water column and where it will flow: a lattice of points, every third column moved onto a cell face."""
    F = p.Position[p.Type == 1]
    lo, hi = F.min(0) - cfg.H, F.max(0) + cfg.H
    ax = [np.linspace(lo[d], hi[d], n) for d in range(F.shape[1])]
    ax[0][::3] = (np.round(ax[0][::3] / cfg.H) + 0.5) * cfg.H
    ax[-1][1::3] = (np.round(ax[-1][1::3] / cfg.H) + 0.5) * cfg.H
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, F.shape[1])


@pytest.mark.parametrize("fb", [8, 4])
def test_stale_lists(fb, request):
    """Sample j of a fresh handle advanced j steps, for EVERY j up to K, against brute force on that handle's download: steps
    right behind a rebuild and steps far behind one, where rows have drifted out of the cell `cstart` files them under."""
    p, s = _state("dam_break_2d", request)
    K = 110
    probes = None
    history, progress = [], []
    for j in range(1, K + 1):
        eng = _engine(p, s, fb)
        if probes is None:
            probes = _lattice_probes(p, eng.cfg)
        eng.probes_enable(probes, capacity=K)
        pr = eng.advance(1e9, max_steps=j)
        assert pr.iteration == j
        r = eng.probes_read()
        assert len(r["iteration"]) == j
        history.append(pr.n_rebuilds); progress.append((pr.iteration, pr.total_time, pr.last_dt))
        ref = _reference(eng, probes)
        _check_against(ref, _raw(r), r, fb, f"step {j} (rebuilds so far {pr.n_rebuilds})")
        if j == K:
            series = r
        eng.close()
    # where the rebuilds were: the one that opens the call comes before step 1; a later one comes before step j when the count grew from j - 1 to j
    rebuilt_before = [1] + [j for j in range(2, K + 1) if history[j - 1] > history[j - 2]]
    since = [j - max(b for b in rebuilt_before if b <= j) for j in range(1, K + 1)]
    print(f"fp{8 * fb}: rebuilds before steps {rebuilt_before}; longest stretch without one {max(since) + 1} steps")
    assert len(rebuilt_before) >= 2, "no Δx-triggered rebuild within the horizon"
    assert max(since) >= 10, "no checked step lies 10 steps behind the last rebuild"
    assert any(b > 1 for b in rebuilt_before)                                      # a checked step follows a Δx-triggered rebuild directly
    # 3.: the series of the K-step call holds every step once, in order, with the clock sphmi_progress reports step by step
    np.testing.assert_array_equal(series["iteration"], np.arange(1, K + 1))
    for j in range(1, K + 1):
        assert (int(series["iteration"][j - 1]), float(series["time"][j - 1]), float(series["dt"][j - 1])) == progress[j - 1], j


@pytest.mark.parametrize("case,fb", [("dam_break_2d", 4), ("dam_break_2d", 8), ("moving_square", 0), ("still_wedge", 0), ("dam_break_3d_shipped", 4)])
def test_every_executed_step_across_calls(case, fb, request):
    """Several sphmi_advance calls (output intervals), batches cut by rebuilds, capacity overflow; handles whose step control is a
    launch of its own (moving bodies, mDBC: fp64 by the library's policy)."""
    p, s = _state(case, request, vel=1.0 if case == "still_wedge" else 3.0)
    probes = _lattice_probes(p, _engine(p, s, fb).cfg, n=5)
    eng, small = _engine(p, s, fb), _engine(p, s, fb)
    eng.probes_enable(probes, capacity=1000)
    small.probes_enable(probes, capacity=50)
    calls = [5, 1, 33, 40, 2] if case != "dam_break_3d_shipped" else [5, 1, 20]
    total = sum(calls)
    its, ts, dts, prs = [], [], [], []
    for n in calls:
        pr = eng.advance(1e9, max_steps=n)
        q = small.advance(1e9, max_steps=n)
        assert (q.iteration, q.total_time, q.last_dt) == (pr.iteration, pr.total_time, pr.last_dt)
        r = eng.probes_read()
        assert len(r["iteration"]) == n == pr.steps_done
        assert (int(r["iteration"][-1]), float(r["time"][-1]), float(r["dt"][-1])) == (pr.iteration, pr.total_time, pr.last_dt)
        its.append(r["iteration"]); ts.append(r["time"]); dts.append(r["dt"]); prs.append(r)
    it, t, dt = np.concatenate(its), np.concatenate(ts), np.concatenate(dts)
    np.testing.assert_array_equal(it, np.arange(1, total + 1))                     # no sample for a cancelled step, none twice for a re-queued one
    assert (dt > 0).all()
    np.testing.assert_array_equal(t[1:], t[:-1] + dt[1:])                          # TotalTime += dt, as the control does it
    assert pr.n_rebuilds >= len(calls)                                             # every call opens with one (test_stale_lists crosses the Δx-triggered ones)
    # the last sample is the state the handle holds
    ref = _reference(eng, probes)
    _check_against(ref, _raw(prs[-1]), prs[-1], eng.device_float_bytes, f"{case} after {total} steps in {len(calls)} calls")
    # capacity overflow: the newest 50 stay, the others are counted
    import ctypes as C
    f = small._fn("probes_read")
    n_wait, n_drop = C.c_int64(), C.c_int64()
    assert f(small._h, 0, *[None] * 8, C.byref(n_wait), C.byref(n_drop)) == 0      # capacity 0 asks …
    assert n_wait.value == min(total, 50) and n_drop.value == max(total - 50, 0)
    rs = small.probes_read()                                                      # … and clears nothing
    assert len(rs["iteration"]) == min(total, 50) and small.probes_dropped == max(total - 50, 0)
    np.testing.assert_array_equal(rs["iteration"], it[-len(rs["iteration"]):])
    allw = np.concatenate([r["weight"] for r in prs]); allp = np.concatenate([r["pressure"] for r in prs])
    np.testing.assert_array_equal(rs["weight"], allw[-len(rs["iteration"]):]); np.testing.assert_array_equal(rs["pressure"], allp[-len(rs["iteration"]):])
    small.advance(1e9, max_steps=2)
    assert len(small.probes_read()["iteration"]) == 2 and small.probes_dropped == 0
    eng.close(); small.close()


# ---- 4. sampling does not disturb the run ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,fb", [("dam_break_2d", 4), ("dam_break_2d", 8), ("dam_break_3d_shipped", 4), ("still_wedge", 8)])
def test_sampling_does_not_disturb_the_run(case, fb, request):
    p, s = _state(case, request)
    K = 100
    markers = sorted(int(m) for m in np.unique(p.GroupMarker))
    probes = _lattice_probes(p, _engine(p, s, fb).cfg, n=6)
    runs = []
    for sampled in (False, True, True):
        eng = _engine(p, s, fb)
        eng.group_forces_enable(markers, capacity=K)
        if sampled:
            eng.probes_enable(probes, capacity=K)
        prs = [eng.advance(1e9, max_steps=n) for n in (K - 7, 7)]
        prog = [(q.iteration, q.steps_done, q.n_rebuilds, q.index_counter, q.total_time, q.last_dt, q.delta_x) for q in prs]
        runs.append((prog, eng.download(), eng.group_forces_read(), eng.probes_read() if sampled else None))
        eng.close()
    assert runs[0][0][-1][2] >= 3
    assert runs[0][0] == runs[1][0] == runs[2][0]
    for k, v in runs[0][1].items():
        np.testing.assert_array_equal(runs[1][1][k], v, err_msg=k)                  # the final state, bit for bit
    for a, b in zip(runs[0][2], runs[1][2]):
        np.testing.assert_array_equal(a, b)                                         # the group-force series, bit for bit
    assert len(runs[1][3]["iteration"]) == K and np.abs(runs[1][3]["weight"]).max() > 0
    for k in runs[1][3]:
        np.testing.assert_array_equal(runs[1][3][k], runs[2][3][k], err_msg=k)      # two sampled runs: the same bits


# ---- 5. slabs in one handle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("case,fb,axis", [("dam_break_2d", 8, 0), ("dam_break_2d", 4, 0), ("dam_break_2d", 8, 1), ("dam_break_3d_shipped", 4, 0), ("dam_break_3d_shipped", 8, 1)])
def test_slabs_in_one_handle(case, fb, axis, world, request):
    """Every slab sums the rows it owns for every probe, the handle adds the raw sums.  Probes sit ON the cuts (the face between
    two slabs' cell columns) and within H of them: a ghost copy that counted would double their sums, a skipped owner halve them."""
    p, s = _state(case, request)
    K = 60 if case == "dam_break_2d" else 20
    scout = _engine(p, s, fb, devices=[0] * world, slab_axis=axis)
    scout.advance(1e9, max_steps=K)
    info = scout.multi_info()
    assert info.world == world and info.n_local == world and info.axis == axis
    cfg = scout.cfg
    d0 = scout.download(FIELDS)
    scout.close()
    probes = _lattice_probes(p, cfg, n=7 if case == "dam_break_2d" else 5)
    F = d0["Position"][d0["Type"] == 1]
    on_cut = []
    for c in info.cuts[:world - 1]:
        xc = (c - 0.5) * cfg.H                                                     # cell column c covers |x/H - c| <= 1/2
        near = F[np.argsort(np.abs(F[:, axis] - xc))[:6]].copy()
        for off in (0.0, 0.0, -0.3 * cfg.H, 0.3 * cfg.H, -0.9 * cfg.H, 0.9 * cfg.H):
            q = near[len(on_cut) % 6].copy(); q[axis] = xc + off
            on_cut.append(q)
    probes = np.concatenate([probes, np.array(on_cut)])
    ref, dd = _engine(p, s, fb), _engine(p, s, fb, devices=[0] * world, slab_axis=axis)
    for e in (ref, dd):
        e.probes_enable(probes, capacity=K)
    pr, pd = ref.advance(1e9, max_steps=K), dd.advance(1e9, max_steps=K)
    assert (pd.iteration, pd.steps_done, pd.n_rebuilds) == (pr.iteration, pr.steps_done, pr.n_rebuilds)
    assert sum(dd.multi_info().n_live[:world]) > len(p)                            # ghost copies are held
    rr, rd = ref.probes_read(), dd.probes_read()
    np.testing.assert_array_equal(rd["iteration"], rr["iteration"])
    assert len(rd["iteration"]) == K
    # the slab handle's last sample against ITS OWN download: nothing counted twice, nothing lost
    own = _reference(dd, probes)
    _check_against(own, _raw(rd), rd, fb, f"{case} {world} slabs along axis {axis}, own download")
    assert (own["n"][-len(on_cut):] > 0).any()
    # … and the whole series against the one-device handle's, at the slab tests' bars
    tol = 1e-9 if fb == 8 else 1e-5
    for k in range(K):
        a, b = _raw(rd, k), _raw(rr, k)
        for q in ("S", "SP", "Srho", "Sv"):
            scale = np.abs(b[q]).max()
            err = np.abs(a[q] - b[q]).max() / scale if scale > 0 else np.abs(a[q]).max()
            assert err <= tol, (k, q, err)
    print(f"{case} fp{8 * fb} {world} slabs axis {axis}: series within {tol:g} of the one-device handle over {K} steps, {len(on_cut)} probes on or near the cuts")
    ref.close(); dd.close()


# ---- 6. edges and errors ---------------------------------------------------------------------------------------------------------
def test_edges(dam_break_2d, request):
    import ctypes as C
    from sphexample_amd._abi import ERR_ARGUMENT, ERR_STATE, SphmiError, make_config
    from sphexample_amd.engine import Engine, rccl_unique_id
    p, s = _state("dam_break_2d", request)
    cfg = make_config(len(p), s.SimConstants, s.SimKernel, s.SimMetaData, s.SimViscosity, s.SimDensityDiffusion, device_float_bytes=8, host_float_bytes=8)
    bare = Engine(cfg)                                                             # before the upload
    for call in (lambda: bare.probes_enable([[0.1, 0.1]], capacity=4), bare.probes_read):
        with pytest.raises(SphmiError) as ei:
            call()
        assert ei.value.status == ERR_STATE
    bare.close()
    eng = _engine(p, s, 8)
    with pytest.raises(SphmiError) as ei:                                          # read while disabled
        eng.probes_read()
    assert ei.value.status == ERR_STATE
    one = p.Position[p.Type == 1].mean(0)[None, :]                                 # the middle of the water column
    for bad in (np.zeros((1025, 2)), np.array([[0.1, np.nan]]), np.array([[np.inf, 0.1]])):
        with pytest.raises(SphmiError) as ei:
            eng.probes_enable(bad, capacity=4)
        assert ei.value.status == ERR_ARGUMENT
    with pytest.raises(SphmiError) as ei:
        eng.probes_enable(one, capacity=0)
    assert ei.value.status == ERR_ARGUMENT
    fe = eng._fn("probes_enable"); fe.argtypes = None
    assert fe(eng._h, C.c_int32(2), None, C.c_int64(4)) == ERR_ARGUMENT            # null table
    assert fe(eng._h, C.c_int32(-1), one.ctypes.data_as(C.c_void_p), C.c_int64(4)) == ERR_ARGUMENT
    eng.probes_enable(one, capacity=8)
    fr = eng._fn("probes_read")
    fr.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 10
    assert fr(eng._h, 4, *[None] * 8, None, None) == ERR_ARGUMENT                  # null n_out
    n = C.c_int64()
    assert fr(eng._h, -1, *[None] * 8, C.byref(n), None) == ERR_ARGUMENT
    # n_probes = 1, every output pointer NULL but one
    eng.advance(1e9, max_steps=5)
    w = np.zeros((8, 1))
    assert fr(eng._h, 8, None, None, None, w.ctypes.data_as(C.c_void_p), None, None, None, None, C.byref(n), None) == 0 and n.value == 5
    assert (w[:5] > 0.5).all()                                                     # a point inside the water column
    assert len(eng.probes_read()["iteration"]) == 0                                # the read cleared
    # n_probes = 1024, against brute force
    rng = np.random.default_rng(11)
    F = p.Position[p.Type == 1]
    many = F[rng.integers(0, len(F), 1024)] + rng.uniform(-0.05, 0.05, (1024, 2))
    eng.probes_enable(many, capacity=8)                                            # re-enable replaces the set and drops the series
    eng.advance(1e9, max_steps=3)
    r = eng.probes_read()
    assert r["weight"].shape == (3, 1024)
    _check_against(_reference(eng, many), _raw(r), r, 8, "1024 probes")
    # n_probes = 0 disables and drops the series
    eng.advance(1e9, max_steps=2)
    eng.probes_enable(np.zeros((0, 2)), capacity=1)
    with pytest.raises(SphmiError) as ei:
        eng.probes_read()
    assert ei.value.status == ERR_STATE
    # sphmi_forces_once records nothing; group forces beside the probes
    eng.probes_enable(one, capacity=8)
    eng.group_forces_enable([1, 2], capacity=8)
    eng.forces_once()
    assert len(eng.probes_read()["iteration"]) == 0
    eng.advance(1e9, max_steps=4)
    assert len(eng.probes_read()["iteration"]) == 4 and len(eng.group_forces_read()[0]) == 4
    # the upload disables
    eng.upload_particles(p)
    with pytest.raises(SphmiError) as ei:
        eng.probes_read()
    assert ei.value.status == ERR_STATE
    eng.advance(1e9, max_steps=3)
    # rank-mode handles: one slab of the rows per process
    rk = _engine(p, s, 8, rank=0, world=1, unique_id=rccl_unique_id())
    for call in (lambda: rk.probes_enable(one, capacity=4), rk.probes_read):
        with pytest.raises(SphmiError) as ei:
            call()
        assert ei.value.status == ERR_STATE
    eng.close(); rk.close()


def test_generator_disables_and_serves_a_gauge():
    """The device-side generator disables like the upload; on the generated lattice at rest a gauge column through the water
    reads the still-water level (0.3 m deep reservoir of the 3-D dam break) to within a particle spacing or so."""
    from sphexample_amd._abi import ERR_STATE, SphmiError
    from sphexample_amd.cases import setup_dam_break_3d
    from sphexample_amd.engine import make_generated_dam_break_engine
    from sphexample_amd.probes import gauge_column, water_level
    dp = 0.02
    eng = make_generated_dam_break_engine(dp, setup_dam_break_3d(dp), device_float_bytes=4)
    d = eng.download(FIELDS)
    F = d["Position"][d["Type"] == 1]
    base = np.array([F[:, 0].mean(), F[:, 1].mean(), F[:, 2].min()])
    col = gauge_column(base, base + [0, 0, 2 * (F[:, 2].max() - F[:, 2].min())], dp / 2)
    eng.probes_enable(col, capacity=16)
    eng.advance(1e9, max_steps=3)
    r = eng.probes_read()
    _check_against(_reference(eng, col), _raw(r), r, 4, "gauge column, generated lattice")
    level = water_level(col[:, 2], r["weight"])
    top = eng.download(("Position", "Type"))
    top = top["Position"][top["Type"] == 1][:, 2].max()
    print(f"gauge: level {level} top particle {top}")
    assert level.shape == (3,) and (np.abs(level - top) <= 1.5 * dp).all()
    eng._lib.sphmi_generate_dam_break_3d.argtypes = [__import__("ctypes").c_void_p, __import__("ctypes").c_double]
    eng._check(eng._lib.sphmi_generate_dam_break_3d(eng._h, dp))
    with pytest.raises(SphmiError) as ei:
        eng.probes_read()
    assert ei.value.status == ERR_STATE
    eng.close()


def test_run_simulation_hands_the_samples_to_the_callback(dam_break_2d):
    import copy
    from sphexample_amd import simulation
    p, s = dam_break_2d
    meta = copy.deepcopy(s.SimMetaData)
    meta.SimulationTime, meta.OutputTimes = 0.002, 0.001
    F = p.Position[p.Type == 1]
    points = np.array([F.mean(0), F.max(0) + 1.0])
    got = []
    meta2 = copy.deepcopy(meta)                                                    # (RunSimulation advances the clock of the one it is given)
    steps = simulation.RunSimulation(SimGeometry=None, SimMetaData=meta, SimConstants=s.SimConstants, SimKernel=s.SimKernel, SimLogger=None,
                                     SimParticles=p.copy(), SimViscosity=s.SimViscosity, SimDensityDiffusion=s.SimDensityDiffusion,
                                     probes=points, on_output=lambda m, pp, r: got.append((m.Iteration, m.TotalTime, r)))
    assert len(got) == len(steps) + 1 and len(got[0][2]["iteration"]) == 0
    its = np.concatenate([r["iteration"] for _, _, r in got])
    np.testing.assert_array_equal(its, np.arange(1, got[-1][0] + 1))               # every step of the run, once, in order
    for iteration, time, r in got[1:]:
        assert r["weight"].shape[1:] == (2,) and int(r["iteration"][-1]) == iteration and float(r["time"][-1]) == time
        assert (r["weight"][:, 0] > 0.5).all() and (r["weight"][:, 1] == 0).all() and (r["pressure"][:, 0] != 0).any()
    # with group forces as well: the forces first, then the probes
    both = []
    simulation.RunSimulation(SimGeometry=None, SimMetaData=meta2, SimConstants=s.SimConstants, SimKernel=s.SimKernel, SimLogger=None,
                             SimParticles=p.copy(), SimViscosity=s.SimViscosity, SimDensityDiffusion=s.SimDensityDiffusion,
                             group_forces=[1, 2], probes=points, on_output=lambda m, pp, f, r: both.append((f, r)))
    assert len(both) == len(got) and all(len(f[0]) == len(r["iteration"]) for f, r in both)
