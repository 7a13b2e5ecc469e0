"""Tracers: chosen particles followed and massless drifters advected on the device at every step (sphmi_tracers_enable /
sphmi_tracers_read, csrc/sphmi_tracers.h) — needs a real MI355X.

    tracked particle s, record k:   { x[3], v[3], rho, P } = the row of that particle in the download directly after step k, bit for bit
    drifter p, record k:            { X[3], S, SP, Srho, Sv[3], n }: the probes' raw sums at X on the state after step k, X the position
                                    BEFORE the move;  then  X += (Sv / S) * dt  where S >= min_weight, else the drifter stays

References: the per-step downloads themselves, followed through sphmi_download_permutation (tracked particles);
`brute_force_probes` of tests/test_probes_gpu.py, the O(M·N) enumeration the probes are held to, at the probes' bars
BAR = {8: 1e-10, 4: 2e-4} relative to the largest value (drifter sums): counts equal on fp64 handles, on fp32 handles excused only
where the reference itself shows a row within 1e-6·H of the cut, for at most 2 % of the drifters — and the reference alone stays
inside that cap, checked with `sphexample_amd.tracers.step` on the CPU; `sphexample_amd.tracers.move`, the update rule in numpy
with one rounding per operation (the move, bit for bit).

The cases run from `perturbed(p, seed=3, vel_scale=3.0)` like the probes' (rebuilds fall inside tens of steps): dam_break_2d 30
steps, dam_break_3d_shipped 12, moving_square 25, fp64 and fp32 handles.  72 tracked rows (70 drawn over the types present plus the
first and the last row) and 70 drifters: both kinds cross a workgroup boundary of their kernel and leave the last workgroup partly
filled.

"A drifter has travelled further than H": within the step counts above no point of the flow can — a step moves a row by about
CFL·h·|v|/c0, a few thousandths of h, and a rebuild is asked for once rows have moved about h/4 — so that assertion sits in a case
of its own, `test_a_drifter_crosses_cells`: the 2-D dam break streaming at 6 m/s for 400 steps, where the drifters cover 2 H and
more and the candidate cells change under them several times while every move stays exact.
"""
import numpy as np
import pytest

from test_probes_gpu import BAR, _engine, _probe_set, _state, brute_force_probes

pytestmark = pytest.mark.gpu

CASES = {"dam_break_2d": 30, "dam_break_3d_shipped": 12, "moving_square": 25}
FIELDS = ("Position", "Velocity", "Density", "Pressure", "Type")
MIN_WEIGHT = 0.5


def _tracked_rows(p, seed=7):
    """70 rows drawn over the types present (Fluid, Fixed, Moving) in equal shares, plus the first and the last row."""
    rng = np.random.default_rng(seed)
    types = [t for t in (1, 2, 3) if (p.Type == t).any()]
    rows = {0, len(p) - 1}
    share = 70 // len(types)
    for j, t in enumerate(types):
        pool = np.setdiff1d(np.flatnonzero(p.Type == t), list(rows))
        want = share if j else 70 - share * (len(types) - 1)
        rows |= set(int(r) for r in rng.choice(pool, min(want, len(pool)), replace=False))
    rows = np.array(sorted(rows), dtype=np.int64)
    rng.shuffle(rows)                                                              # slots in no particular order
    return rows


def _drifter_set(d, cfg):
    """The probes' set on the state `d` (inside the fluid, on fluid and wall particles, at the free surface, on a cell face and a cell
    corner, outside the grid, above the fluid in empty space: 66 points) and four more inside the fluid: 70."""
    pts, kinds = _probe_set(d, cfg)
    rng = np.random.default_rng(23)
    F = d["Position"][d["Type"] == 1].astype(np.float64)
    more = F[rng.choice(len(F), 4, replace=False)] + rng.uniform(-cfg.dx, cfg.dx, (4, F.shape[1]))
    kinds["more_fluid"] = slice(len(pts), len(pts) + 4)
    return np.concatenate([pts, more]), kinds


def _pad3(a):
    a = np.asarray(a, dtype=np.float64)
    return a if a.shape[-1] == 3 else np.concatenate([a, np.zeros(a.shape[:-1] + (1,))], -1)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b, what=""):
    np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=what)


def _chain(reads, D, what):
    """The move is exact: X of record k + 1 is `tracers.move` of record k's own position, sums and dt, bit for bit; the current
    position closes the chain.  Returns the joined positions [K + 1, m, 3]."""
    from sphexample_amd import tracers
    path = tracers.pathlines(reads)
    S = np.concatenate([r["drifters"]["sums"][:, :, 0] for r in reads])
    Sv = np.concatenate([r["drifters"]["sums"][:, :, 3:6] for r in reads])
    dt = np.concatenate([r["dt"] for r in reads])
    assert len(path) == len(dt) + 1
    for k in range(len(dt)):
        want = tracers.move(path[k], S[k], Sv[k][:, :D], dt[k], MIN_WEIGHT)       # (2-D: the third column is left alone)
        _same_bits(path[k + 1], want, f"{what}: the move of step {k + 1}")
        stay = ~(S[k] >= MIN_WEIGHT)
        _same_bits(path[k + 1][stay], path[k][stay], f"{what}: a dry drifter moved at step {k + 1}")
    return path


_RUNS = {}


def _run(case, fb, request):
    """One handle per (case, fb), advanced one step at a time with a download and sphmi_download_permutation after each: the
    snapshots, the row of every tracked particle in each, and the series.  Computed once, shared by tests 1 to 3, never changed."""
    if (case, fb) in _RUNS:
        return _RUNS[(case, fb)]
    K = CASES[case]
    p, s = _state(case, request)
    assert p.Position.dtype == np.float64
    scout = _engine(p, s, fb)                                                      # where the rows are after the first step: drifters ON them, on their cells' faces
    scout.advance(1e9, max_steps=1)
    d1 = scout.download(FIELDS)
    cfg = scout.cfg
    scout.close()
    X0, kinds = _drifter_set(d1, cfg)
    rows = _tracked_rows(p)
    assert len(rows) == 72 and len(X0) == 70 and len(np.unique(rows)) == 72
    eng = _engine(p, s, fb)
    eng.tracers_enable(particles=rows, drifters=X0, min_weight=MIN_WEIGHT, capacity=K + 4)
    cur, snaps, where, progress, moved = rows.copy(), [], [], [], 0
    for k in range(K):
        pr = eng.advance(1e9, max_steps=1)
        assert pr.iteration == k + 1
        d = eng.download(FIELDS)
        prev = eng.download_permutation()                                          # row i now was row prev[i] at the call before (the upload order at first)
        inv = np.empty(len(prev), dtype=np.int64); inv[prev] = np.arange(len(prev))
        cur = inv[cur]
        moved += int((prev != np.arange(len(prev))).any())
        snaps.append(d); where.append(cur.copy()); progress.append((pr.iteration, pr.total_time, pr.last_dt, pr.n_rebuilds))
    r = eng.tracers_read()
    eng.close()
    out = dict(K=K, D=p.Position.shape[1], cfg=cfg, fb=fb, rows=rows, X0=X0, kinds=kinds, snaps=snaps, where=where, progress=progress, moved=moved, r=r,
               types=np.asarray(p.Type)[rows])
    _RUNS[(case, fb)] = out
    return out


# ---- 1. tracked particles are the download ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("fb", [8, 4])
@pytest.mark.parametrize("case", list(CASES))
def test_tracked_particles_are_the_download(case, fb, request):
    run = _run(case, fb, request)
    K, r = run["K"], run["r"]
    P = r["particles"]
    assert len(r["iteration"]) == K and r["dropped"] == 0 and P["values"].shape == (K, 72, 8)
    np.testing.assert_array_equal(r["iteration"], np.arange(1, K + 1))
    assert set(run["types"]) == set(np.unique(run["snaps"][0]["Type"]))            # every type present is followed
    for k in range(K):
        d, at = run["snaps"][k], run["where"][k]
        assert (int(r["iteration"][k]), float(r["time"][k]), float(r["dt"][k])) == run["progress"][k][:3]
        np.testing.assert_array_equal(d["Type"][at], run["types"], err_msg=f"step {k + 1}: the followed rows are other particles")
        _same_bits(P["position"][k], _pad3(d["Position"][at]), f"Position, step {k + 1}")
        _same_bits(P["velocity"][k], _pad3(d["Velocity"][at]), f"Velocity, step {k + 1}")
        _same_bits(P["density"][k], d["Density"][at], f"Density, step {k + 1}")
        _same_bits(P["pressure"][k], d["Pressure"][at], f"Pressure, step {k + 1}")
    # across rebuilds that moved rows: the sort permuted at least once, and a tracked row changed its place
    assert run["progress"][-1][3] >= 2 and run["moved"] >= 1, "no rebuild permuted the rows within the horizon"
    assert any((run["where"][k] != run["rows"]).any() for k in range(K))
    assert (P["velocity"][:, run["types"] == 1] != 0).any() and (P["pressure"] != 0).any()
    if run["D"] == 2:
        assert (P["position"][:, :, 2] == 0).all() and (P["velocity"][:, :, 2] == 0).all()


# ---- 2. drifter records are probe samples -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fb", [8, 4])
@pytest.mark.parametrize("case", list(CASES))
def test_drifter_records_are_probe_samples(case, fb, request):
    from sphexample_amd import tracers
    run = _run(case, fb, request)
    K, D, cfg, r, kinds = run["K"], run["D"], run["cfg"], run["r"], run["kinds"]
    Dr = r["drifters"]
    M = Dr["position"].shape[1]
    assert Dr["position"].shape == (K, 70, 3) and Dr["sums"].shape == (K, 70, 7)
    _same_bits(Dr["position"][0], _pad3(run["X0"]), "record 1 is taken at the positions of the enable")
    tol = BAR[fb]
    worst = {q: 0.0 for q in ("S", "SP", "Srho", "Sv")}
    excused = near_most = 0
    for k in range(K):
        d = run["snaps"][k]
        X = Dr["position"][k][:, :D]
        ref = brute_force_probes(cfg, X, d["Position"], d["Velocity"], d["Density"], d["Pressure"], d["Type"])
        # the drifter set keeps the reference alone within the cap: the host restatement of the step, on the CPU
        _, own = tracers.step(X, d, cfg, float(r["dt"][k]), MIN_WEIGHT)
        np.testing.assert_array_equal(own["n"], ref["n"])
        assert own["near"].sum() <= 0.02 * M and ref["near"].sum() <= 0.02 * M, f"step {k + 1}: too many drifters with a row at the cut"
        near_most = max(near_most, int(ref["near"].sum()))
        got = {"n": Dr["sums"][k][:, 6], "S": Dr["sums"][k][:, 0], "SP": Dr["sums"][k][:, 1], "Srho": Dr["sums"][k][:, 2], "Sv": Dr["sums"][k][:, 3:6]}
        differ = got["n"] != ref["n"]
        if fb == 8:
            assert not differ.any(), (k, np.flatnonzero(differ))
        else:
            assert not (differ & ~ref["near"]).any(), (k, np.flatnonzero(differ & ~ref["near"]))
            assert differ.sum() <= 0.02 * M
            excused = max(excused, int(differ.sum()))
        for q in worst:
            scale = np.abs(ref[q]).max()
            err = np.abs(got[q] - ref[q]).max() / scale if scale > 0 else np.abs(got[q]).max()
            worst[q] = max(worst[q], err)
        empty = ref["n"] == 0
        assert (got["S"][empty] == 0).all() and (got["n"][empty] == 0).all() and (got["Sv"][empty] == 0).all()
        if k == 0:                                                                 # the kinds are what they say, at the step they were built for
            assert (ref["n"][kinds["fluid"]] > 0).all() and (ref["n"][kinds["on_fluid_particle"]] > 0).all()
            assert (ref["n"][kinds["outside_grid"]] == 0).all() and (ref["n"][kinds["empty"]] == 0).all()
            surf = ref["S"][kinds["surface"]]
            assert (surf > 0).all() and surf.min() < 0.8, surf
    print(f"{case} fp{8 * fb}: {K} steps x {M} drifters; " + ", ".join(f"{q} {v:.3g}" for q, v in worst.items())
          + f" (bar {tol:g}); near the cut at most {near_most}, counts excused at most {excused}")
    for q, v in worst.items():
        assert v <= tol, (case, q, v, tol)
    # the normalised values are the probes': sums over S, zero where nothing was found
    S = Dr["sums"][:, :, 0]
    some = (Dr["sums"][:, :, 6] > 0) & (S > 0)
    _same_bits(Dr["pressure"][some], Dr["sums"][:, :, 1][some] / S[some])
    _same_bits(Dr["velocity"][some], Dr["sums"][:, :, 3:6][some] / S[some][:, None])
    assert (Dr["pressure"][~some] == 0).all() and (Dr["weight"] == S).all() and (Dr["count"] == Dr["sums"][:, :, 6]).all()


# ---- 3. the move is exact --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fb", [8, 4])
@pytest.mark.parametrize("case", list(CASES))
def test_the_move_is_exact(case, fb, request):
    from sphexample_amd import tracers
    run = _run(case, fb, request)
    r, kinds, D = run["r"], run["kinds"], run["D"]
    path = _chain([r], D, f"{case} fp{8 * fb}")
    assert path.shape == (run["K"] + 1, 70, 3)
    S = r["drifters"]["sums"][:, :, 0]
    wet = S >= MIN_WEIGHT
    assert wet.any() and (~wet).any()
    assert (path[1:][wet] != path[:-1][wet]).any(axis=-1).all()                    # every wet drifter moved at every wet step …
    np.testing.assert_array_equal(tracers.dry(r), ~wet)
    # … and dry ones, empty ones and the ones outside the grid have not moved by a bit over the whole run
    for kind in ("outside_grid", "empty"):
        assert (S[:, kinds[kind]] == 0).all()
        _same_bits(path[:, kinds[kind]], np.broadcast_to(_pad3(run["X0"][kinds[kind]]), path[:, kinds[kind]].shape), kind)
    never = ~wet.any(0)
    assert never.sum() >= 8
    _same_bits(path[-1][never], _pad3(run["X0"])[never])
    if D == 2:
        assert (path[:, :, 2] == 0).all()


def _streaming(request, speed=6.0):
    p, s = _state("dam_break_2d", request, vel=0.5)
    p.Velocity[p.Type == 1, 0] += speed
    return p, s


@pytest.mark.parametrize("fb", [8, 4])
def test_a_drifter_crosses_cells(fb, request):
    """The 2-D dam break streaming along +x, 400 steps in one call: drifters released in the water travel further than H — the
    candidate cells change under them — every move stays exact, and the drifters stay in the water they were released in."""
    p, s = _streaming(request)
    K = 400
    F = p.Position[p.Type == 1]
    rng = np.random.default_rng(31)
    inside = F[(F[:, 0] > F[:, 0].min() + 0.2) & (F[:, 0] < F[:, 0].max() - 0.2) & (F[:, 1] > F[:, 1].min() + 0.2) & (F[:, 1] < F[:, 1].max() - 0.3)]
    X0 = np.concatenate([inside[rng.choice(len(inside), 60, replace=False)] + rng.uniform(-0.01, 0.01, (60, 2)), F.max(0)[None] + [[0.5, 0.5]] * 4 + rng.uniform(0, 0.1, (4, 2))])
    eng = _engine(p, s, fb)
    H = eng.cfg.H
    eng.tracers_enable(drifters=X0, min_weight=MIN_WEIGHT, capacity=K)
    pr = eng.advance(1e9, max_steps=K)
    r = eng.tracers_read()
    assert pr.iteration == K and len(r["iteration"]) == K and pr.n_rebuilds >= 3
    path = _chain([r], 2, f"streaming fp{8 * fb}")
    travel = np.linalg.norm(path[-1] - path[0], axis=1)
    print(f"streaming fp{8 * fb}: {K} steps to t = {pr.total_time:.4g}, {pr.n_rebuilds} rebuilds; travel of the drifters in H: median {np.median(travel[:60]) / H:.3g}, "
          f"max {travel.max() / H:.3g}; wet at the last step {int((r['drifters']['weight'][-1] >= MIN_WEIGHT).sum())} of 64")
    assert (travel > H).any(), "no drifter has travelled further than H: the candidate cells never changed under one"
    assert (travel[:60] > H).sum() >= 30 and (travel[60:] == 0).all()
    # the last record is still a probe sample at the place the drifter has reached
    d = eng.download(FIELDS)
    eng2 = _engine(p, s, fb)
    eng2.tracers_enable(drifters=X0, min_weight=MIN_WEIGHT, capacity=K)
    eng2.advance(1e9, max_steps=K)
    _same_bits(eng2.tracers_read()["drifter_position"], r["drifter_position"], "two identical runs")
    ref = brute_force_probes(eng.cfg, r["drifters"]["position"][-1][:, :2], d["Position"], d["Velocity"], d["Density"], d["Pressure"], d["Type"])
    got = r["drifters"]["sums"][-1]
    assert ref["near"].sum() <= 0.02 * len(X0)
    differ = got[:, 6] != ref["n"]
    assert not (differ & ~ref["near"]).any() and (fb == 4 or not differ.any())
    for q, a in (("S", got[:, 0]), ("SP", got[:, 1]), ("Srho", got[:, 2]), ("Sv", got[:, 3:6])):
        assert np.abs(a - ref[q]).max() <= BAR[fb] * np.abs(ref[q]).max(), q
    assert (ref["S"][:60] >= MIN_WEIGHT).sum() >= 30                                # they went with the water
    eng.close(); eng2.close()


# ---- 4. a full log does not stop a drifter ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,fb", [("dam_break_2d", 4), ("dam_break_2d", 8), ("dam_break_3d_shipped", 4)])
def test_a_full_log_does_not_stop_a_drifter(case, fb, request):
    run = _run(case, fb, request)
    p, s = _state(case, request)
    K = 45 if case == "dam_break_2d" else 14                                       # more than one batch of queued steps in the 2-D case
    ample, small = _engine(p, s, fb), _engine(p, s, fb)
    ample.tracers_enable(particles=run["rows"], drifters=run["X0"], capacity=K + 1)
    small.tracers_enable(particles=run["rows"], drifters=run["X0"], capacity=5)
    pa, ps = ample.advance(1e9, max_steps=K), small.advance(1e9, max_steps=K)
    assert (pa.iteration, pa.total_time) == (ps.iteration, ps.total_time) and pa.iteration == K
    ra, rs = ample.tracers_read(), small.tracers_read()
    assert ra["dropped"] == 0 and len(ra["iteration"]) == K
    assert rs["dropped"] == K - 5 and small.tracers_dropped == K - 5 and len(rs["iteration"]) == 5
    _same_bits(rs["drifter_position"], ra["drifter_position"], "the drifters of the handle whose series overflowed")
    assert (ra["drifter_position"] != _pad3(run["X0"])).any()
    np.testing.assert_array_equal(rs["iteration"], ra["iteration"][-5:])
    _same_bits(rs["drifters"]["position"], ra["drifters"]["position"][-5:]); _same_bits(rs["particles"]["values"], ra["particles"]["values"][-5:])
    _chain([ra], run["D"], f"{case} fp{8 * fb}, one call")
    ample.close(); small.close()


# ---- 5. every executed step, across calls ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,fb", [("dam_break_2d", 4), ("dam_break_2d", 8), ("moving_square", 0), ("dam_break_3d_shipped", 4)])
def test_every_executed_step_across_calls(case, fb, request):
    """Several sphmi_advance calls, a read between some of them only, and a last call bounded by time instead of a step count: the
    steps of its batch queued behind the one that passes t_target are cancelled on the device.  Every executed step once, in order;
    the chain of moves has no gap — a cancelled step that moved a drifter, or a record that was lost, would break it."""
    run = _run(case, fb or 8, request)
    p, s = _state(case, request)
    eng = _engine(p, s, fb)
    eng.tracers_enable(particles=run["rows"], drifters=run["X0"], capacity=1000)
    calls = [5, 1, 33, 40, 2] if case != "dam_break_3d_shipped" else [5, 1, 20]
    read_after = {1, 2, len(calls)}
    reads, expected, total = [], 0, 0
    for c, n in enumerate(calls + [None]):
        if n is None:                                                              # until TotalTime passes t_target: a few steps run, the rest of the batch is cancelled
            pr = eng.advance(pr.total_time + 2.5 * pr.last_dt)
            n = int(pr.steps_done)
            assert 1 <= n <= 8, n
        else:
            pr = eng.advance(1e9, max_steps=n)
            assert pr.steps_done == n
        total += n; expected += n
        assert pr.iteration == total
        if c in read_after:
            r = eng.tracers_read()
            assert len(r["iteration"]) == expected and r["dropped"] == 0
            assert (int(r["iteration"][-1]), float(r["time"][-1]), float(r["dt"][-1])) == (pr.iteration, pr.total_time, pr.last_dt)
            reads.append(r); expected = 0
    it = np.concatenate([r["iteration"] for r in reads]); t = np.concatenate([r["time"] for r in reads]); dt = np.concatenate([r["dt"] for r in reads])
    np.testing.assert_array_equal(it, np.arange(1, total + 1))                     # no record for a cancelled step, none twice for a re-queued one
    assert (dt > 0).all()
    np.testing.assert_array_equal(t[1:], t[:-1] + dt[1:])
    assert pr.n_rebuilds >= len(calls) + 1                                         # every call opens with one
    path = _chain(reads, run["D"], f"{case} across {len(calls)} calls")
    _same_bits(path[0], _pad3(run["X0"]))
    assert len(eng.tracers_read()["iteration"]) == 0                               # the read cleared; the position stays available
    _same_bits(eng.tracers_read()["drifter_position"], path[-1])
    # the last record of the tracked particles is the state the handle holds
    d = eng.download(FIELDS)
    prev = eng.download_permutation()
    inv = np.empty(len(prev), dtype=np.int64); inv[prev] = np.arange(len(prev))
    at = inv[run["rows"]]
    last = reads[-1]["particles"]
    _same_bits(last["position"][-1], _pad3(d["Position"][at])); _same_bits(last["velocity"][-1], _pad3(d["Velocity"][at]))
    _same_bits(last["density"][-1], d["Density"][at]); _same_bits(last["pressure"][-1], d["Pressure"][at])
    eng.close()


# ---- 6. the run is not disturbed ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,fb", [("dam_break_2d", 4), ("dam_break_2d", 8), ("dam_break_3d_shipped", 4)])
def test_the_run_is_not_disturbed(case, fb, request):
    run = _run(case, fb, request)
    p, s = _state(case, request)
    K = 60 if case == "dam_break_2d" else 16
    runs = []
    for traced in (False, True, True):
        eng = _engine(p, s, fb)
        if traced:
            eng.tracers_enable(particles=run["rows"], drifters=run["X0"], capacity=K)
        prs = [eng.advance(1e9, max_steps=n) for n in (K - 7, 7)]
        prog = [(q.iteration, q.steps_done, q.n_rebuilds, q.index_counter, q.total_time, q.last_dt, q.delta_x) for q in prs]
        runs.append((prog, eng.download(), eng.tracers_read() if traced else None))
        eng.close()
    assert runs[0][0] == runs[1][0] == runs[2][0]
    for k, v in runs[0][1].items():
        np.testing.assert_array_equal(runs[1][1][k], v, err_msg=k)                  # the final state, bit for bit
    a, b = runs[1][2], runs[2][2]
    assert len(a["iteration"]) == K
    for k in ("iteration", "time", "dt", "drifter_position"):
        _same_bits(a[k], b[k], k) if a[k].dtype == np.float64 else np.testing.assert_array_equal(a[k], b[k])
    _same_bits(a["particles"]["values"], b["particles"]["values"]); _same_bits(a["drifters"]["position"], b["drifters"]["position"])
    _same_bits(a["drifters"]["sums"], b["drifters"]["sums"])                        # two traced runs: the same bits


# ---- 7. edges ------------------------------------------------------------------------------------------------------------------------------
def test_edges(request):
    import ctypes as C
    from sphexample_amd._abi import ERR_ARGUMENT, ERR_STATE, SphmiError, make_config
    from sphexample_amd.engine import Engine
    run = _run("dam_break_2d", 8, request)
    p, s = _state("dam_break_2d", request)
    cfg = make_config(len(p), s.SimConstants, s.SimKernel, s.SimMetaData, s.SimViscosity, s.SimDensityDiffusion, device_float_bytes=8, host_float_bytes=8)
    bare = Engine(cfg)                                                             # before the upload
    for call in (lambda: bare.tracers_enable(particles=[0]), bare.tracers_read):
        with pytest.raises(SphmiError) as ei:
            call()
        assert ei.value.status == ERR_STATE
    bare.close()
    eng = _engine(p, s, 8)
    with pytest.raises(SphmiError) as ei:                                          # read while disabled
        eng.tracers_read()
    assert ei.value.status == ERR_STATE
    one = p.Position[p.Type == 1].mean(0)[None, :]
    bad = (dict(particles=[0, 5, 0]), dict(particles=[len(p)]), dict(particles=[-1]), dict(particles=np.arange(1025)), dict(drifters=np.zeros((1025, 2))),
           dict(drifters=[[0.1, np.nan]]), dict(drifters=[[np.inf, 0.1]]), dict(drifters=one, min_weight=0.0), dict(drifters=one, min_weight=np.inf),
           dict(drifters=one, min_weight=np.nan), dict(drifters=one, capacity=0), dict(particles=[3], capacity=-1))
    for kw in bad:
        with pytest.raises(SphmiError) as ei:
            eng.tracers_enable(**kw)
        assert ei.value.status == ERR_ARGUMENT and str(ei.value).count("sphmi_tracers_enable: ") == 1, kw
    fe = eng._fn("tracers_enable"); fe.argtypes = None
    assert fe(eng._h, C.c_int32(2), None, C.c_int32(0), None, C.c_double(0.5), C.c_int64(4)) == ERR_ARGUMENT          # null tables
    assert fe(eng._h, C.c_int32(0), None, C.c_int32(1), None, C.c_double(0.5), C.c_int64(4)) == ERR_ARGUMENT
    # only particles; only drifters; one of each
    eng.tracers_enable(particles=run["rows"], capacity=8)
    eng.advance(1e9, max_steps=3)
    r = eng.tracers_read()
    assert r["particles"]["values"].shape == (3, 72, 8) and r["drifters"]["position"].shape == (3, 0, 3) and r["drifter_position"].shape == (0, 3)
    np.testing.assert_array_equal(r["iteration"], [1, 2, 3])
    eng.tracers_enable(drifters=run["X0"], capacity=8)                             # enabling again replaces the set and drops the series
    eng.advance(1e9, max_steps=3)
    r = eng.tracers_read()
    assert r["particles"]["values"].shape == (3, 0, 8) and r["drifters"]["position"].shape == (3, 70, 3)
    np.testing.assert_array_equal(r["iteration"], [4, 5, 6])
    _same_bits(r["drifters"]["position"][0], _pad3(run["X0"]))
    _chain([r], 2, "only drifters")
    moved_to = r["drifter_position"].copy()
    who = int(eng.download(("ID",))["ID"][len(p) - 1])                              # six steps in: the rows are no longer in upload order
    eng.tracers_enable(particles=[len(p) - 1], drifters=one, capacity=8)           # one of each: the drifter starts at ITS position, not where the old ones were
    eng.advance(1e9, max_steps=2)
    r = eng.tracers_read()
    assert r["particles"]["values"].shape == (2, 1, 8) and r["drifters"]["sums"].shape == (2, 1, 7)
    _same_bits(r["drifters"]["position"][0], _pad3(one))
    assert (r["drifters"]["weight"] > 0.5).all() and (r["drifter_position"] != _pad3(one)).any() and (moved_to[0] != r["drifter_position"][0]).any()
    _chain([r], 2, "one of each")
    d = eng.download(FIELDS + ("ID",))
    at = int(np.flatnonzero(d["ID"] == who)[0])
    _same_bits(r["particles"]["position"][-1, 0], _pad3(d["Position"][at])); _same_bits(r["particles"]["pressure"][-1, 0], d["Pressure"][at])
    # every output pointer NULL but the positions; capacity 0 asks and clears nothing
    eng.advance(1e9, max_steps=2)
    fr = eng._fn("tracers_read")
    fr.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 8
    n = C.c_int64()
    x = np.zeros((1, 3))
    assert fr(eng._h, 4, *[None] * 6, None, None) == ERR_ARGUMENT                  # null n_out
    assert fr(eng._h, -1, *[None] * 6, C.byref(n), None) == ERR_ARGUMENT
    assert fr(eng._h, 0, None, None, None, None, None, x.ctypes.data_as(C.c_void_p), C.byref(n), None) == 0 and n.value == 2
    assert (x != 0).any() and len(eng.tracers_read()["iteration"]) == 2
    # sphmi_forces_once moves and records nothing
    before = eng.tracers_read()["drifter_position"]
    eng.forces_once()
    r = eng.tracers_read()
    assert len(r["iteration"]) == 0
    _same_bits(r["drifter_position"], before)
    # both counts zero disables; the upload disables
    eng.tracers_enable()
    with pytest.raises(SphmiError) as ei:
        eng.tracers_read()
    assert ei.value.status == ERR_STATE
    eng.tracers_enable(particles=[0], drifters=one)
    eng.upload_particles(p)
    with pytest.raises(SphmiError) as ei:
        eng.tracers_read()
    assert ei.value.status == ERR_STATE
    eng.advance(1e9, max_steps=3)
    eng.close()
    # a multi-slab handle refuses, with the envelopes' status and kind of text
    dd = _engine(p, s, 8, devices=[0, 0])
    for call in (lambda: dd.tracers_enable(particles=[0], drifters=one), dd.tracers_read):
        with pytest.raises(SphmiError) as ei:
            call()
        assert ei.value.status == ERR_STATE and "single-device handles only" in str(ei.value)
    dd.advance(1e9, max_steps=2)
    dd.close()


# ---- 8. RunSimulation ----------------------------------------------------------------------------------------------------------------------
def test_run_simulation_hands_the_dicts_to_the_callback(dam_break_2d):
    import copy
    from sphexample_amd import simulation, tracers
    p, s = dam_break_2d
    meta = copy.deepcopy(s.SimMetaData)
    meta.SimulationTime, meta.OutputTimes = 0.002, 0.001
    F = p.Position[p.Type == 1]
    points = np.array([F.mean(0), F.max(0) + 1.0])
    rows = [0, int(np.flatnonzero(p.Type == 1)[10]), len(p) - 1]
    got = []
    steps = simulation.RunSimulation(SimGeometry=None, SimMetaData=meta, SimConstants=s.SimConstants, SimKernel=s.SimKernel, SimLogger=None,
                                     SimParticles=p.copy(), SimViscosity=s.SimViscosity, SimDensityDiffusion=s.SimDensityDiffusion,
                                     tracers=dict(particles=rows, drifters=points, min_weight=0.5), budgets=True,
                                     on_output=lambda m, pp, b, r: got.append((m.Iteration, m.TotalTime, len(b["iteration"]), r)))
    assert len(got) == len(steps) + 1 and got[0][3] is None                        # behind the other observers; nothing before the first step
    reads = [r for _, _, _, r in got]
    executed = got[-1][0]
    np.testing.assert_array_equal(np.concatenate([r["iteration"] for r in reads[1:]]), np.arange(1, executed + 1))
    for iteration, time, nb, r in got[1:]:
        assert len(r["iteration"]) == nb and int(r["iteration"][-1]) == iteration and float(r["time"][-1]) == time
        assert r["particles"]["values"].shape[1:] == (3, 8) and r["drifters"]["position"].shape[1:] == (2, 3)
    path = tracers.pathlines(reads)
    assert path.shape == (executed + 1, 2, 3)                                      # the executed steps plus one
    _same_bits(path[0], _pad3(points)); _same_bits(path[-1], reads[-1]["drifter_position"])
    _same_bits(path[:, 1], np.broadcast_to(_pad3(points)[1], (executed + 1, 3)))   # the point outside the grid never moved
    assert (tracers.dry(reads)[:, 1]).all() and not tracers.dry(reads)[:, 0].any()
    _chain(reads[1:], 2, "RunSimulation")
    keyed = tracers.by_id(reads, p.ID[rows])
    assert keyed["values"].shape == (executed, 3, 8) and (np.diff(keyed["id"]) > 0).all()
