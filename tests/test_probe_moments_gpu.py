"""The moment sums at fixed probes on every step (sphmi_probe_moments_enable / sphmi_probe_moments_read, csrc/sphmi_probe_moments.h)
and the fit over a whole series (sphexample_amd/probes.py: fit_series) — needs a real MI355X.

The reference is `brute_force_point_moments` of tests/test_point_moments_host.py: an O(M·N) numpy enumeration written from the
definition (pinned there by closed forms), fed the probes and the download taken after the sampled step.  It never calls the library.

Bars (the project's for a single evaluation, tests/test_probes_gpu.py): every RAW sum — S, SP, Sρ, Sv, M1, M2, P1, R1, V1 — within
BAR = 1e-10 of that sum's largest magnitude over the probe set on fp64 handles, 2e-4 on fp32 handles; n equal at every probe on fp64;
on fp32 a probe may differ only where the reference itself shows a Fluid row within 1e-6·H of the cut, at most 2 % of the probes,
and the reference alone must stay under that cap.  The sums of a step against sphmi_sample_point_moments on the state after it: the
same bars (the two kernels add in different orders).  Slots 0 … 6 against the probes and against dry drifters at the same points:
np.array_equal.  Slab handles against the one-device handle: 1e-9 / 1e-5, the bars of the existing slab tests.  fit_series over the
device's sums against linear_fit over the enumeration's: the rule of tests/test_point_moments_gpu.py::_check_fit.

Shapes: the shipped fixtures from `perturbed(p, seed=3, vel_scale=3.0)`; the probes are the 700-point `gradient_cloud` over the
Fluid rows of the sampled state (a scout run finds it): inside, at the surface, on walls, in empty space, outside the grid.  One run
per (case, precision) is shared by the tests that read it."""
import ctypes as C

import numpy as np
import pytest

from test_point_gradients_gpu import CASES as CLOUD_CASES, _check_counts
from test_point_gradients_host import gradient_cloud
from test_point_moments_gpu import _check_fit, _figures, _z_slots_are_zero
from test_point_moments_host import KEYS, SUMS, brute_force_point_moments
from test_probes_gpu import BAR, FIELDS, _engine, _lattice_probes, _state, _variant

pytestmark = pytest.mark.gpu

CASES = {k: CLOUD_CASES[k] for k in ("dam_break_2d", "dam_break_3d_shipped", "cubic_spline")}      # name → (fixture, steps, kernel variant)
CASES["still_wedge"] = ("still_wedge", 30, None)
SHARED = ("weight", "count", "sum_pressure", "sum_density", "sum_velocity")      # slots 0 … 6: the probes' own sums


def _setup(case, request):
    fixture, K, kernel = CASES[case]
    p, s = _state(fixture, request)
    if kernel:
        s = _variant(s, kernel, None)
    return p, s, K


def _named(rec, k=-1):
    """Step k of a probe_moments_read() by the names of the sums."""
    return {KEYS[key]: rec[key][k] for key in KEYS}


def _enumerate(eng, pts, d=None):
    d = d or eng.download(FIELDS)
    return brute_force_point_moments(eng.cfg, pts, d["Position"], d["Velocity"], d["Density"], d["Pressure"], d["Type"])


def _check_step(got, ref, fb, D, what):
    """The bars of the module docstring on one step; prints every figure before it asserts."""
    fig = _figures(got, ref)
    differ = got["n"] != ref["n"]
    print(f"{what} fp{8 * fb}: {len(ref['n'])} probes, {int((ref['n'] > 0).sum())} see fluid, n differs at {int(differ.sum())}, near the cut {int(ref['near'].sum())}; "
          + ", ".join(f"{q} {v:.3g}" for q, v in fig.items()) + f" (bar {BAR[fb]:g})")
    _check_counts(got["n"], ref["n"], ref["near"], fb)
    for q, v in fig.items():
        assert v <= BAR[fb], (what, q, v, BAR[fb])
    empty = ref["n"] == 0
    for q in SUMS:
        assert (got[q][empty] == 0).all(), q                                       # exact zeros where no row passes the cut
    if D == 2:
        _z_slots_are_zero(got)                                                     # exact zeros in every slot of the third axis


_RUNS = {}


def _run(case, fb, request):
    """One run per (case, precision): a scout without observers finds the cloud, a second handle records the probes, the moments and
    dry drifters at it over the same K steps.  Read-only for the tests."""
    if (case, fb) in _RUNS:
        return _RUNS[(case, fb)]
    p, s, K = _setup(case, request)
    scout = _engine(p, s, fb)
    ps = scout.advance(1e9, max_steps=K)
    d0 = scout.download()
    scout.close()
    cfg = scout.cfg
    pts = gradient_cloud(d0["Position"][d0["Type"] == 1].astype(np.float64), cfg.H, cfg.dx)
    assert len(pts) == 700
    eng = _engine(p, s, fb)
    eng.probes_enable(pts, capacity=K + 4)
    eng.probe_moments_enable(pts, capacity=K + 4)
    eng.tracers_enable(drifters=pts, min_weight=1e300, capacity=K + 4)              # dry drifters stay: the RAW sums of the probes' walk at the same points
    pr = eng.advance(1e9, max_steps=K)
    run = dict(K=K, pts=pts, cfg=cfg, D=eng.D, scout=(ps, d0), progress=pr, moments=eng.probe_moments_read(), dropped=eng.probe_moments_dropped,
               probes=eng.probes_read(), drifters=eng.tracers_read()["drifters"])
    run["download"] = eng.download()
    run["on_demand"] = eng.sample_point_moments(pts)
    run["ref"] = _enumerate(eng, pts, run["download"])
    run["eng_cfg"] = eng.cfg
    eng.close()
    _RUNS[(case, fb)] = run
    return run


# ---- 1. the last sample equals the enumeration; 7. sampling does not disturb the run ---------------------------------------------------
@pytest.mark.parametrize("fb", [8, 4])
@pytest.mark.parametrize("case", list(CASES))
def test_last_sample_equals_the_enumeration(case, fb, request):
    run = _run(case, fb, request)
    K, M, rec, pr = run["K"], len(run["pts"]), run["moments"], run["progress"]
    assert list(rec) == ["iteration", "time", "dt"] + list(KEYS) + ["h", "dims", "probe_moments_dropped"]
    assert (rec["h"], rec["dims"], rec["probe_moments_dropped"], run["dropped"]) == (run["cfg"].h, run["D"], 0, 0)
    assert len(rec["iteration"]) == K and rec["count"].dtype == np.int64 and rec["weight"].shape == rec["count"].shape == (K, M)
    assert rec["sum_velocity"].shape == rec["moment1"].shape == rec["moment_pressure"].shape == rec["moment_density"].shape == (K, M, 3)
    assert rec["moment2"].shape == rec["moment_velocity"].shape == (K, M, 3, 3)
    assert np.array_equal(rec["moment2"], np.swapaxes(rec["moment2"], 2, 3))        # filled from the six
    assert (int(rec["iteration"][-1]), float(rec["time"][-1]), float(rec["dt"][-1])) == (pr.iteration, pr.total_time, pr.last_dt)
    ref, got = run["ref"], _named(rec)
    _check_step(got, ref, fb, run["D"], f"{case} last of {K} steps")
    assert (ref["n"] > 0).sum() > 100 and (ref["n"] == 0).sum() > 0 and (ref["n"] < 0.5 * ref["n"].max()).sum() > 20      # inside, empty, at the edges
    assert np.abs(ref["V1"]).max() > 0 and np.abs(ref["P1"]).max() > 0 and np.abs(ref["M1"]).max() > 0
    if run["D"] == 2:
        for k in range(K):
            _z_slots_are_zero(_named(rec, k))


@pytest.mark.parametrize("case,fb", [("dam_break_2d", 4), ("dam_break_2d", 8), ("dam_break_3d_shipped", 4), ("still_wedge", 8)])
def test_sampling_does_not_disturb_the_run(case, fb, request):
    """The scout ran without an observer, the sampled handle with three: the same progress, the same download, byte for byte."""
    run = _run(case, fb, request)
    (ps, d0), pr, d = run["scout"], run["progress"], run["download"]
    prog = lambda q: (q.iteration, q.steps_done, q.n_rebuilds, q.index_counter, q.total_time, q.last_dt, q.delta_x)      # noqa: E731
    assert prog(ps) == prog(pr) and pr.n_rebuilds >= 1
    assert set(d) == set(d0)
    for k, v in d0.items():
        assert v.tobytes() == d[k].tobytes(), k


# ---- 2. steps far behind a rebuild ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fb", [8, 4])
def test_stale_lists(fb, request):
    """The construction of tests/test_probes_gpu.py::test_stale_lists: a fresh handle advanced j steps reports the rebuilds up to step
    j, so the history over j = 1 … K tells which steps open with one.  The step furthest behind its rebuild, and the last step of a
    stretch before the next one, are sampled by fresh handles and held against the enumeration on their own downloads: rows have
    drifted out of the cell `cstart` files them under."""
    p, s = _state("dam_break_2d", request)
    K = 60
    history = []
    for j in range(1, K + 1):
        eng = _engine(p, s, fb)
        history.append(eng.advance(1e9, max_steps=j).n_rebuilds)
        eng.close()
    rebuilt_before = [1] + [j for j in range(2, K + 1) if history[j - 1] > history[j - 2]]
    since = [j - max(b for b in rebuilt_before if b <= j) for j in range(1, K + 1)]
    far = 1 + int(np.argmax(since))
    print(f"fp{8 * fb}: rebuilds before steps {rebuilt_before}; step {far} lies {since[far - 1]} steps behind its rebuild")
    assert len(rebuilt_before) >= 2, "no Δx-triggered rebuild within the horizon"
    assert since[far - 1] >= 10 and far not in rebuilt_before, "no step lies 10 steps behind the last rebuild"
    ends = [b - 1 for b in rebuilt_before[1:] if b - 1 not in rebuilt_before]      # the last step before a Δx-triggered rebuild
    assert ends
    probes = None
    for j in sorted({far, ends[0]}):
        eng = _engine(p, s, fb)
        probes = _lattice_probes(p, eng.cfg) if probes is None else probes
        eng.probe_moments_enable(probes, capacity=K)
        pr = eng.advance(1e9, max_steps=j)
        assert pr.iteration == j and pr.n_rebuilds == history[j - 1] and (j == 1 or history[j - 1] == history[j - 2])      # not a rebuild step
        rec = eng.probe_moments_read()
        assert len(rec["iteration"]) == j
        ref = _enumerate(eng, probes)
        assert (ref["n"] > 0).sum() > 20
        _check_step(_named(rec), ref, fb, 2, f"step {j}, {since[j - 1]} steps behind a rebuild")
        eng.close()


# ---- 3. together with the probes: slots 0 … 6 are the probes' ---------------------------------------------------------------------------
@pytest.mark.parametrize("case,fb", [("dam_break_2d", 8), ("dam_break_2d", 4), ("dam_break_3d_shipped", 4), ("dam_break_3d_shipped", 8), ("cubic_spline", 8),
                                     ("still_wedge", 8)])
def test_the_shared_sums_hold_the_bits_of_the_probes(case, fb, request):
    """Probes, moment probes and dry drifters (min_weight beyond reach: they never move) at the same points over one batch of
    steps.  The drifters record the RAW sums of the probes' walk: np.array_equal with slots 0 … 6 of the moment record at every step.
    sphmi_probes_read normalises its record with one fp64 division per value, which numpy repeats on the moment record's sums."""
    run = _run(case, fb, request)
    m, pr, dr = run["moments"], run["probes"], run["drifters"]
    K = run["K"]
    for key in ("iteration", "time", "dt"):
        assert np.array_equal(m[key], pr[key]), key
    assert m["weight"].shape == pr["weight"].shape == (K, 700) and (m["count"] > 0).sum() > 100 * K and np.abs(m["sum_velocity"]).max() > 0
    raw = dr["sums"]                                                                # [K, M, 7]: S, SP, Sρ, Sv[3], n
    assert np.array_equal(dr["position"], np.broadcast_to(np.pad(run["pts"], ((0, 0), (0, 3 - run["D"]))), dr["position"].shape))      # they stayed
    same = {"weight": np.array_equal(m["weight"], raw[:, :, 0]), "count": np.array_equal(m["count"], raw[:, :, 6].astype(np.int64)),
            "sum_pressure": np.array_equal(m["sum_pressure"], raw[:, :, 1]), "sum_density": np.array_equal(m["sum_density"], raw[:, :, 2]),
            "sum_velocity": np.array_equal(m["sum_velocity"], raw[:, :, 3:6])}
    some = (m["count"] > 0) & (m["weight"] > 0)
    safe = np.where(some, m["weight"], 1.0)
    mean = lambda a: np.where(some if a.ndim == 2 else some[:, :, None], a / (safe if a.ndim == 2 else safe[:, :, None]), 0.0)      # noqa: E731
    same.update({"probes weight": np.array_equal(m["weight"], pr["weight"]), "probes count": np.array_equal(m["count"], pr["count"]),
                 "probes pressure": np.array_equal(mean(m["sum_pressure"]), pr["pressure"]), "probes density": np.array_equal(mean(m["sum_density"]), pr["density"]),
                 "probes velocity": np.array_equal(mean(m["sum_velocity"]), pr["velocity"])})
    print(f"{case} fp{8 * fb}: {K} steps x 700 probes; bit-equal: {same}")
    assert all(same.values()), same


# ---- 4. repeated runs give the same bytes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,fb", [("dam_break_2d", 4), ("dam_break_3d_shipped", 8)])
def test_two_handles_give_the_same_bytes(case, fb, request):
    run = _run(case, fb, request)
    p, s, K = _setup(case, request)
    eng = _engine(p, s, fb)
    eng.probes_enable(run["pts"], capacity=K + 4)
    eng.probe_moments_enable(run["pts"], capacity=K + 4)
    eng.tracers_enable(drifters=run["pts"], min_weight=1e300, capacity=K + 4)
    eng.advance(1e9, max_steps=K)
    again = eng.probe_moments_read()
    eng.close()
    assert list(again) == list(run["moments"])
    for key in list(KEYS) + ["iteration", "time", "dt"]:
        assert again[key].tobytes() == run["moments"][key].tobytes(), key


# ---- 5. every executed step across calls ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,fb", [("dam_break_2d", 4), ("dam_break_2d", 8), ("still_wedge", 0), ("dam_break_3d_shipped", 4)])
def test_every_executed_step_across_calls(case, fb, request):
    """Several sphmi_advance calls, batches cut by rebuilds, capacity overflow; mDBC handles, whose step control is a launch of its own."""
    p, s = _state(case, request)
    probes = _lattice_probes(p, _engine(p, s, fb).cfg, n=5)
    eng, small = _engine(p, s, fb), _engine(p, s, fb)
    eng.probe_moments_enable(probes, capacity=1000)
    eng.probes_enable(probes[::2], capacity=1000)                                  # a point set of its own
    small.probe_moments_enable(probes, capacity=50)
    calls = [5, 1, 33, 40, 2] if case != "dam_break_3d_shipped" else [5, 1, 20]
    total = sum(calls)
    recs = []
    for n in calls:
        pr = eng.advance(1e9, max_steps=n)
        small.advance(1e9, max_steps=n)
        r, q = eng.probe_moments_read(), eng.probes_read()
        assert len(r["iteration"]) == n == pr.steps_done and r["probe_moments_dropped"] == 0
        assert (int(r["iteration"][-1]), float(r["time"][-1]), float(r["dt"][-1])) == (pr.iteration, pr.total_time, pr.last_dt)
        for key in ("iteration", "time", "dt"):
            assert np.array_equal(r[key], q[key]), key                              # the clock of the probes, step by step
        assert np.array_equal(r["weight"][:, ::2], q["weight"]) and np.array_equal(r["count"][:, ::2], q["count"])
        recs.append(r)
    it = np.concatenate([r["iteration"] for r in recs])
    np.testing.assert_array_equal(it, np.arange(1, total + 1))                     # no sample for a cancelled step, none twice for a re-queued one
    assert pr.n_rebuilds >= len(calls)
    _check_step(_named(recs[-1]), _enumerate(eng, probes), eng.device_float_bytes, eng.D, f"{case} after {total} steps in {len(calls)} calls")
    # capacity overflow: the newest 50 stay, the others are counted; capacity 0 asks and clears nothing
    f = small._fn("probe_moments_read")
    n_wait, n_drop = C.c_int64(), C.c_int64()
    assert f(small._h, 0, *[None] * 13, C.byref(n_wait), C.byref(n_drop)) == 0
    assert n_wait.value == min(total, 50) and n_drop.value == max(total - 50, 0)
    rs = small.probe_moments_read()
    assert len(rs["iteration"]) == min(total, 50) and small.probe_moments_dropped == rs["probe_moments_dropped"] == max(total - 50, 0)
    np.testing.assert_array_equal(rs["iteration"], it[-len(rs["iteration"]):])
    for key in KEYS:
        whole = np.concatenate([r[key] for r in recs])
        assert np.array_equal(rs[key], whole[-len(rs["iteration"]):]), key
    small.advance(1e9, max_steps=2)
    assert len(small.probe_moments_read()["iteration"]) == 2 and small.probe_moments_dropped == 0
    eng.close(); small.close()


# ---- 6. the fit --------------------------------------------------------------------------------------------------------------------
class _Handle:
    """what _check_fit reads off a handle"""
    def __init__(self, cfg, D):
        self.cfg, self.D = cfg, D


@pytest.mark.parametrize("fb", [8, 4])
@pytest.mark.parametrize("case", list(CASES))
def test_the_fit_of_the_last_sample(case, fb, request):
    from sphexample_amd.fields import linear_fit
    from sphexample_amd.probes import fit_series
    run = _run(case, fb, request)
    rec, ref = run["moments"], run["ref"]
    fit = fit_series(rec)
    K = run["K"]
    assert fit["pressure"].shape == fit["linear"].shape == fit["rcond"].shape == (K, 700) and fit["velocity_gradient"].shape == (K, 700, 3, 3)
    assert np.array_equal(fit["iteration"], rec["iteration"])
    last = {k: rec[k][-1] for k in KEYS}
    last.update(h=rec["h"], dims=rec["dims"])
    one = linear_fit(last)
    for k in one:
        assert np.array_equal(fit[k][-1], one[k]), k                                # the series' last step IS linear_fit of that step
    _check_fit(_Handle(run["eng_cfg"], run["D"]), last, ref, fb, f"{case} fit of the last step")
    # … and against the on-demand sampler on the same state: the sums within the bar (another order of summation: not to the bit)
    od = {KEYS[k]: run["on_demand"][k] for k in KEYS}
    got = _named(rec)
    fig = _figures(got, od)
    print(f"{case} fp{8 * fb}: against sphmi_sample_point_moments on the same state: " + ", ".join(f"{q} {v:.3g}" for q, v in fig.items()) + f" (bar {BAR[fb]:g})")
    assert np.array_equal(got["n"], od["n"]) or fb == 4
    _check_counts(got["n"], od["n"], ref["near"], fb, cap_on_reference=False)
    for q, v in fig.items():
        assert v <= BAR[fb], (q, v)


# ---- 8. slabs in one handle -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("case,fb,axis", [("dam_break_2d", 8, 0), ("dam_break_2d", 4, 1), ("dam_break_3d_shipped", 4, 0), ("dam_break_3d_shipped", 8, 1)])
def test_slabs_in_one_handle(case, fb, axis, world, request):
    """Every slab sums the rows it owns for every probe, the handle adds the records in slab order.  Probes sit ON the cuts and within
    H of them: a ghost copy that counted would double their sums, a skipped owner halve them."""
    p, s, _ = _setup(case, request)
    lead, K = (30, 12) if case == "dam_break_2d" else (8, 6)
    one, dd = _engine(p, s, fb), _engine(p, s, fb, devices=[0] * world, slab_axis=axis)
    cfg = one.cfg
    # `lead` steps tell where the cuts lie and where the fluid is there; the set is then replaced by one with probes on and around the cuts
    for e in (one, dd):
        e.probe_moments_enable(_lattice_probes(p, cfg, n=3), capacity=1)
    pr, pd = one.advance(1e9, max_steps=lead), dd.advance(1e9, max_steps=lead)
    info = dd.multi_info()
    assert info.world == world and info.n_local == world and info.axis == axis and sum(info.n_live[:world]) > len(p)      # ghost copies are held
    d0 = one.download(FIELDS)
    F = d0["Position"][d0["Type"] == 1].astype(np.float64)
    on_cut = []
    for c in info.cuts[:world - 1]:
        xc = (c - 0.5) * cfg.H                                                     # cell column c covers |x/H - c| <= 1/2
        near = F[np.argsort(np.abs(F[:, axis] - xc))[:6]].copy()
        for i, off in enumerate((0.0, 0.0, -0.3 * cfg.H, 0.3 * cfg.H, -0.9 * cfg.H, 0.9 * cfg.H)):
            q = near[i].copy(); q[axis] = xc + off
            on_cut.append(q)
    probes = np.concatenate([_lattice_probes(p, cfg, n=7 if case == "dam_break_2d" else 5), np.array(on_cut)])
    for e in (one, dd):
        e.probe_moments_enable(probes, capacity=K)                                 # replaces the set and drops the series
    pr, pd = one.advance(1e9, max_steps=K), dd.advance(1e9, max_steps=K)
    assert (pd.iteration, pd.steps_done, pd.n_rebuilds) == (pr.iteration, pr.steps_done, pr.n_rebuilds)
    ro, rd = one.probe_moments_read(), dd.probe_moments_read()
    np.testing.assert_array_equal(rd["iteration"], ro["iteration"])
    np.testing.assert_array_equal(rd["iteration"], np.arange(lead + 1, lead + K + 1))
    assert (rd["count"][-1][-len(on_cut):] > 0).sum() >= len(on_cut) // 2           # the probes on the cuts see fluid
    # the slab handle's last sample against ITS OWN download: nothing counted twice, nothing lost
    _check_step(_named(rd), _enumerate(dd, probes), fb, dd.D, f"{case} {world} slabs along axis {axis}, own download")
    # … and the whole series against the one-device handle's, at the slab tests' bars
    tol = 1e-9 if fb == 8 else 1e-5
    worst = {}
    for key in KEYS:
        if key == "count":
            continue
        a, b = rd[key].reshape(K, -1), ro[key].reshape(K, -1)
        scale = np.abs(b).max(1)
        err = np.abs(a - b).max(1) / np.where(scale > 0, scale, 1.0)
        worst[key] = err.max()
    print(f"{case} fp{8 * fb} {world} slabs axis {axis}: series against the one-device handle over {K} steps: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()) + f" (bar {tol:g})")
    for key, v in worst.items():
        assert v <= tol, (key, v)
    one.close(); dd.close()


# ---- 9. errors and edges -----------------------------------------------------------------------------------------------------------
def test_edges(request):
    from sphexample_amd._abi import ERR_ARGUMENT, ERR_STATE, SphmiError, make_config
    from sphexample_amd.engine import Engine, rccl_unique_id
    p, s = _state("dam_break_2d", request)
    cfg = make_config(len(p), s.SimConstants, s.SimKernel, s.SimMetaData, s.SimViscosity, s.SimDensityDiffusion, device_float_bytes=8, host_float_bytes=8)

    def refused(call, status):
        with pytest.raises(SphmiError) as ei:
            call()
        assert ei.value.status == status

    bare = Engine(cfg)                                                             # before the upload
    refused(lambda: bare.probe_moments_enable([[0.1, 0.1]], capacity=4), ERR_STATE)
    refused(bare.probe_moments_read, ERR_STATE)
    bare.close()
    eng = _engine(p, s, 8)
    refused(eng.probe_moments_read, ERR_STATE)                                     # read while disabled
    one = p.Position[p.Type == 1].mean(0)[None, :]                                 # the middle of the water column
    for bad in (np.zeros((1025, 2)), np.array([[0.1, np.nan]]), np.array([[np.inf, 0.1]])):
        refused(lambda: eng.probe_moments_enable(bad, capacity=4), ERR_ARGUMENT)
    refused(lambda: eng.probe_moments_enable(one, capacity=0), ERR_ARGUMENT)
    fe = eng._fn("probe_moments_enable")
    assert fe(eng._h, 2, None, 4) == ERR_ARGUMENT                                  # null table
    assert fe(eng._h, -1, one.ctypes.data_as(C.c_void_p), 4) == ERR_ARGUMENT
    assert "sphmi_probe_moments_enable" in eng._fn("last_error")(eng._h).decode()
    refused(eng.probe_moments_read, ERR_STATE)                                     # a refused enable leaves it off
    eng.probe_moments_enable(one, capacity=8)
    fr = eng._fn("probe_moments_read")
    fr.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 15
    assert fr(eng._h, 4, *[None] * 13, None, None) == ERR_ARGUMENT                 # null n_out
    n = C.c_int64()
    assert fr(eng._h, -1, *[None] * 13, C.byref(n), None) == ERR_ARGUMENT
    # n_probes = 1, every output pointer NULL but one
    eng.advance(1e9, max_steps=5)
    m2 = np.zeros((8, 1, 6))
    assert fr(eng._h, 8, *[None] * 9, m2.ctypes.data_as(C.c_void_p), None, None, None, C.byref(n), None) == 0 and n.value == 5
    assert (m2[:5, 0, 0] > 0).all() and (m2[:5, 0, 3] > 0).all() and (m2[:5, 0, [2, 4, 5]] == 0).all() and (m2[5:] == 0).all()      # xx, yy; no z on a 2-D handle
    assert len(eng.probe_moments_read()["iteration"]) == 0                         # the read cleared
    # n_probes = 1024, against the enumeration; replace while enabled drops the series
    rng = np.random.default_rng(11)
    F = p.Position[p.Type == 1]
    many = F[rng.integers(0, len(F), 1024)] + rng.uniform(-0.05, 0.05, (1024, 2))
    eng.advance(1e9, max_steps=2)
    eng.probe_moments_enable(many, capacity=8)
    eng.advance(1e9, max_steps=3)
    r = eng.probe_moments_read()
    assert r["weight"].shape == (3, 1024) and r["moment_velocity"].shape == (3, 1024, 3, 3)
    _check_step(_named(r), _enumerate(eng, many), 8, 2, "1024 probes")
    # n_probes = 0 disables and drops the series
    eng.advance(1e9, max_steps=2)
    eng.probe_moments_enable(np.zeros((0, 2)), capacity=1)
    refused(eng.probe_moments_read, ERR_STATE)
    # sphmi_forces_once records nothing; the probes beside the moments keep a series of their own
    eng.probe_moments_enable(one, capacity=8)
    eng.probes_enable(many[:3], capacity=8)
    eng.forces_once()
    assert len(eng.probe_moments_read()["iteration"]) == 0
    eng.advance(1e9, max_steps=4)
    eng.probes_enable(np.zeros((0, 2)), capacity=1)                                # switching the probes off leaves the moments on
    assert eng.probe_moments_read()["weight"].shape == (4, 1)
    # the upload disables
    eng.upload_particles(p)
    refused(eng.probe_moments_read, ERR_STATE)
    eng.advance(1e9, max_steps=3)
    # handles with H < h
    th = _engine(p, _variant(s, None, 0.9), 8)
    refused(lambda: th.probe_moments_enable(one, capacity=4), ERR_STATE)
    refused(th.probe_moments_read, ERR_STATE)
    th.close()
    # rank-mode handles: one slab of the rows per process
    rk = _engine(p, s, 8, rank=0, world=1, unique_id=rccl_unique_id())
    refused(lambda: rk.probe_moments_enable(one, capacity=4), ERR_STATE)
    refused(rk.probe_moments_read, ERR_STATE)
    eng.close(); rk.close()


def test_generator_disables():
    from sphexample_amd._abi import ERR_STATE, SphmiError
    from sphexample_amd.cases import setup_dam_break_3d
    from sphexample_amd.engine import make_generated_dam_break_engine
    dp = 0.02
    eng = make_generated_dam_break_engine(dp, setup_dam_break_3d(dp), device_float_bytes=4)
    d = eng.download(FIELDS)
    F = d["Position"][d["Type"] == 1].astype(np.float64)
    pts = np.array([F.mean(0), F.min(0), F.max(0) + 1.0])
    eng.probe_moments_enable(pts, capacity=16)
    eng.advance(1e9, max_steps=3)
    r = eng.probe_moments_read()
    _check_step(_named(r), _enumerate(eng, pts), 4, 3, "generated lattice")
    eng._check(eng._fn("generate_dam_break_3d")(eng._h, dp))
    with pytest.raises(SphmiError) as ei:
        eng.probe_moments_read()
    assert ei.value.status == ERR_STATE
    eng.close()


def test_run_simulation_hands_the_records_to_the_callback(dam_break_2d):
    import copy
    from sphexample_amd import simulation
    from sphexample_amd.probes import fit_series
    p, s = dam_break_2d
    meta = copy.deepcopy(s.SimMetaData)
    meta.SimulationTime, meta.OutputTimes = 0.002, 0.001
    F = p.Position[p.Type == 1]
    points = np.array([F.mean(0), F.max(0) + 1.0])
    got = []
    steps = simulation.RunSimulation(SimGeometry=None, SimMetaData=meta, SimConstants=s.SimConstants, SimKernel=s.SimKernel, SimLogger=None,
                                     SimParticles=p.copy(), SimViscosity=s.SimViscosity, SimDensityDiffusion=s.SimDensityDiffusion,
                                     probes=points[:1], probe_moments=points, on_output=lambda m, pp, q, r: got.append((m.Iteration, m.TotalTime, q, r)))
    assert len(got) == len(steps) + 1 and len(got[0][3]["iteration"]) == 0 and got[0][3]["moment2"].shape == (0, 2, 3, 3)
    assert fit_series(got[0][3])["pressure"].shape == (0, 2)                      # the empty record of the first call fits to an empty series
    its = np.concatenate([r["iteration"] for _, _, _, r in got])
    np.testing.assert_array_equal(its, np.arange(1, got[-1][0] + 1))               # every step of the run, once, in order
    for iteration, time, q, r in got[1:]:
        assert r["weight"].shape[1:] == (2,) and int(r["iteration"][-1]) == iteration and float(r["time"][-1]) == time
        assert (r["weight"][:, 0] > 0.5).all() and (r["weight"][:, 1] == 0).all() and (r["moment_pressure"][:, 0] != 0).any()
        assert np.array_equal(r["weight"][:, :1], q["weight"])                     # behind the probes, which sample their own set
        fit = fit_series(r)
        assert fit["linear"][:, 0].all() and not fit["linear"][:, 1].any()
