"""Kernel sums and their moments at arbitrary points (sphmi_sample_point_moments, csrc/sphmi_point_moments.h) and the linear fit on
them (sphexample_amd/fields.py: linear_fit) — needs a real MI355X.

The reference is `brute_force_point_moments` of tests/test_point_moments_host.py: an O(M·N) numpy enumeration written from the
definition (pinned there by closed forms), fed the cloud and a download taken right after the call.  It never calls the library.

Bars (the project's for a single evaluation, tests/test_probes_gpu.py): every RAW sum — S, SP, Sρ, Sv, M1, M2, P1, R1, V1 — within
1e-10 of that sum's largest magnitude over the cloud on fp64 handles, 2e-4 on fp32 handles; n equal at every point on fp64; on fp32
a point may differ only where the reference itself shows a Fluid row within 1e-6·H of the cut, at most 2 % of the points, and the
reference alone must stay under that cap.  S, n, SP, Sρ and Sv against sphmi_sample_point_gradients on the same cloud: the same
bits.  Slab handles against the one-device handle: 1e-9 / 1e-5, the bars of tests/test_sample_points_gpu.py::
test_slabs_in_one_handle.  What a point reads must not depend on the other points of the call: np.array_equal on every output.
linear_fit over the device's sums against linear_fit over the enumeration's: the same `linear` flags wherever the enumeration's
reciprocal condition number is at least 10 × away from LINEAR_FIT_MIN_RCOND, and there the fitted values within BAR / rcond of the
field's largest magnitude over the cloud — the amplification the solve itself allows.
"""
import ctypes as C

import numpy as np
import pytest

from test_point_gradients_gpu import CASES, _check_counts, _fluid, _one_cell, _start
from test_point_gradients_host import gradient_cloud
from test_point_moments_host import KEYS, SUMS, as_sums, brute_force_point_moments
from test_probes_gpu import BAR, FIELDS, _engine, _state, _variant

pytestmark = pytest.mark.gpu

SHARED = ("weight", "count", "sum_pressure", "sum_density", "sum_velocity")      # the sums the gradient sampler delivers too


def _named(out):
    """The dict of sample_point_moments by the names of the sums."""
    return {KEYS[k]: v for k, v in out.items() if k in KEYS}


def _figures(got, ref):
    out = {}
    for q in SUMS:
        scale = np.abs(ref[q]).max()
        out[q] = np.abs(got[q] - ref[q]).max() / scale if scale > 0 else np.abs(got[q]).max()
    return out


def _z_slots_are_zero(got):
    assert (got["Sv"][:, 2] == 0).all() and (got["M1"][:, 2] == 0).all() and (got["P1"][:, 2] == 0).all() and (got["R1"][:, 2] == 0).all()
    for q in ("M2", "V1"):
        assert (got[q][:, 2, :] == 0).all() and (got[q][:, :, 2] == 0).all(), q


def _check_cloud(eng, pts, fb, what):
    """Sample, download right after, enumerate; prints every figure before it asserts.  Returns (out, named, ref)."""
    out = eng.sample_point_moments(pts)
    d = eng.download(FIELDS)
    M = len(pts)
    assert list(out) == list(KEYS) + ["h", "dims"] and out["count"].dtype == np.int64 and (out["h"], out["dims"]) == (eng.cfg.h, eng.D)
    assert out["weight"].shape == (M,) and out["moment1"].shape == (M, 3) and out["moment2"].shape == out["moment_velocity"].shape == (M, 3, 3)
    assert np.array_equal(out["moment2"], np.swapaxes(out["moment2"], 1, 2))        # filled from the six
    got = _named(out)
    ref = brute_force_point_moments(eng.cfg, pts, d["Position"], d["Velocity"], d["Density"], d["Pressure"], d["Type"])
    fig = _figures(got, ref)
    differ = got["n"] != ref["n"]
    print(f"{what} fp{8 * fb}: {M} points, {int((ref['n'] > 0).sum())} see fluid, n differs at {int(differ.sum())}, near the cut {int(ref['near'].sum())}; "
          + ", ".join(f"{q} {v:.3g}" for q, v in fig.items()) + f" (bar {BAR[fb]:g})")
    _check_counts(got["n"], ref["n"], ref["near"], fb)
    for q, v in fig.items():
        assert v <= BAR[fb], (what, q, v, BAR[fb])
    empty = ref["n"] == 0
    for q in SUMS:
        assert (got[q][empty] == 0).all(), q                                       # exact zeros where no row passes the cut
    if eng.D == 2:                                                                 # exact zeros in every z slot
        _z_slots_are_zero(got)
    return out, got, ref


def _check_fit(eng, out, ref, fb, what):
    """linear_fit over the device's sums against linear_fit over the enumeration's."""
    from sphexample_amd.fields import LINEAR_FIT_MIN_RCOND, linear_fit
    dev, want = linear_fit(out), linear_fit(as_sums(ref, eng.cfg, eng.D))
    rc = want["rcond"]
    clear = (rc >= 10 * LINEAR_FIT_MIN_RCOND) | (rc <= 0.1 * LINEAR_FIT_MIN_RCOND)
    both = clear & want["linear"] & dev["linear"]
    some = ref["n"] > 0
    S = np.where(some & (ref["S"] > 0), ref["S"], 1.0)
    scale = {"pressure": np.abs(ref["SP"] / S).max(), "density": np.abs(ref["Srho"] / S).max(), "velocity": np.abs(ref["Sv"] / S[:, None]).max()}
    worst = {}
    for k, sc in scale.items():
        err = np.abs(dev[k] - want[k]).reshape(len(rc), -1).max(1)
        worst[k] = (err[both] * rc[both]).max() / sc
    print(f"{what} fp{8 * fb}: {int(want['linear'].sum())} of {len(rc)} points fitted, {int((~clear).sum())} within 10 × of the threshold, rcond of the fitted "
          f"{rc[want['linear']].min():.3g} … {rc[want['linear']].max():.3g}; |fit − fit of the enumeration| · rcond / scale: "
          + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()) + f" (bar {BAR[fb]:g})")
    assert want["linear"].sum() > 100 and (~want["linear"] & some).sum() > 0        # fitted points, and wet points that fell back
    assert np.array_equal(dev["linear"][clear], want["linear"][clear]), np.flatnonzero(clear & (dev["linear"] != want["linear"]))
    for k, v in worst.items():
        assert v <= BAR[fb], (what, k, v)
    away = ~dev["linear"]
    assert (dev["pressure_gradient"][away] == 0).all() and (dev["velocity_gradient"][away] == 0).all() and (dev["pressure"][~some] == 0).all()


def _same_bits(a, b, what, rows=None, keys=KEYS):
    for k in keys:
        x = a[k] if rows is None else a[k][rows]
        assert np.array_equal(x, b[k]), (what, k, int((x != b[k]).sum()))


# ---- 1. equals the enumeration; the fit over it -----------------------------------------------------------------------------------
@pytest.mark.parametrize("fb", [8, 4])
@pytest.mark.parametrize("case", list(CASES))
def test_equals_the_enumeration(case, fb, request):
    eng, p, s, K = _start(case, fb, request)
    eng.advance(1e9, max_steps=K)
    if case == "moving_square":
        assert eng.cfg.h * 2 > eng.cfg.H * (1 + 1e-9)                              # k < 2
    if case == "cubic_spline":
        assert eng.cfg.kernel == 1
    pts = gradient_cloud(_fluid(eng), eng.cfg.H, eng.cfg.dx)
    assert len(pts) == 700
    out, got, ref = _check_cloud(eng, pts, fb, f"{case} cloud")
    assert (ref["n"] > 0).sum() > 100 and (ref["n"] < 0.5 * ref["n"].max()).sum() > 20      # inside the fluid, and at its edges
    assert np.abs(ref["V1"]).max() > 0 and np.abs(ref["P1"]).max() > 0 and np.abs(ref["M1"]).max() > 0
    _check_fit(eng, out, ref, fb, f"{case} fit")
    eng.close()


# ---- 2. the shared sums are the gradient sampler's ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case,fb", [("dam_break_2d", 8), ("dam_break_2d", 4), ("dam_break_3d_shipped", 8), ("dam_break_3d_shipped", 4), ("cubic_spline", 8)])
def test_the_shared_sums_hold_the_bits_of_the_gradient_sampler(case, fb, request):
    eng, p, s, K = _start(case, fb, request)
    eng.advance(1e9, max_steps=K)
    pts = gradient_cloud(_fluid(eng), eng.cfg.H, eng.cfg.dx, seed=11)
    m = eng.sample_point_moments(pts)
    g = eng.sample_point_gradients(pts)
    same = {k: bool(np.array_equal(m[k], g[k])) for k in SHARED}
    print(f"{case} fp{8 * fb}: {len(pts)} points, {int((m['count'] > 0).sum())} see fluid; bit-equal to sphmi_sample_point_gradients: {same}")
    assert (m["count"] > 0).sum() > 100 and np.abs(m["sum_velocity"]).max() > 0
    assert all(same.values()), same
    eng.close()


# ---- 3. independence --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,fb", [("dam_break_2d", 8), ("dam_break_2d", 4), ("dam_break_3d_shipped", 4), ("dam_break_3d_shipped", 8)])
def test_a_point_reads_the_same_whatever_else_is_in_the_call(case, fb, request):
    eng, p, s, K = _start(case, fb, request)
    eng.advance(1e9, max_steps=K)
    F = _fluid(eng)
    H, D = eng.cfg.H, eng.D
    rng = np.random.default_rng(17)
    # 257 points inside ONE cell: two tiles of one block
    out, got, ref = _check_cloud(eng, _one_cell(F, H, rng, 257), fb, f"{case} 257 points in one block")
    assert (ref["n"] > 0).all()
    # wholly outside the grid: all zeros
    X = eng.download(FIELDS)["Position"].astype(np.float64)
    outside = np.concatenate([X.min(0) - np.array([3.3 * H, 7 * H, 100.0][:D]) * np.ones((1, D)), X.max(0) + 3.3 * H + rng.uniform(0, 1e6, (40, D))])
    far = eng.sample_point_moments(outside)
    for k in KEYS:
        assert (far[k] == 0).all(), k
    pts = gradient_cloud(F, H, eng.cfg.dx, seed=23, count=1500)
    full = eng.sample_point_moments(pts)
    assert (full["count"] > 0).sum() > 200
    _same_bits(eng.sample_point_moments(pts), full, "the same call twice")
    perm = np.random.default_rng(29).permutation(len(pts))
    _same_bits(full, eng.sample_point_moments(pts[perm]), "the cloud shuffled", rows=perm)
    sub = np.sort(np.random.default_rng(31).choice(len(pts), 400, replace=False))
    _same_bits(full, eng.sample_point_moments(pts[sub]), "a subset of the cloud", rows=sub)
    inside = int(np.flatnonzero(full["count"] > 0)[0])
    twice = eng.sample_point_moments(np.concatenate([pts[inside:inside + 1], _one_cell(F, H, rng, 300), pts, outside]))
    _same_bits(twice, full, "the cloud behind 301 points, the outside behind it", rows=slice(301, 301 + len(pts)))
    for k in KEYS:
        assert np.array_equal(twice[k][0], full[k][inside]), ("a point given twice", k)
    # a subset of the outputs: the others travel as NULL, the bits stay
    part = eng.sample_point_moments(pts, fields=("moment_velocity", "count", "moment2"))
    assert set(part) == {"moment_velocity", "count", "moment2", "h", "dims"}
    _same_bits(part, full, "three outputs of ten", keys=("moment_velocity", "count", "moment2"))
    assert eng.sample_point_moments(np.zeros((0, D)))["moment2"].shape == (0, 3, 3)      # an empty cloud is legal
    eng.close()


# ---- 4. slabs in one handle -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("case,fb,axis", [("dam_break_2d", 8, 0), ("dam_break_2d", 4, 1), ("dam_break_3d_shipped", 4, 0), ("dam_break_3d_shipped", 8, 1)])
def test_slabs_in_one_handle(case, fb, axis, world, request):
    """Every slab bins and samples the whole cloud over the rows it owns, the handle adds the raw sums in slab order.  Some points lie
    ON the first cut, others 0.3·H to either side: a ghost copy that counted would double their sums, a skipped owner halve them."""
    fixture, _, _ = CASES[case]
    p, s = _state(fixture, request)
    K = 60 if case == "dam_break_2d" else 20
    ref, dd = _engine(p, s, fb), _engine(p, s, fb, devices=[0] * world, slab_axis=axis)
    pr, pd = ref.advance(1e9, max_steps=K), dd.advance(1e9, max_steps=K)
    assert (pd.iteration, pd.steps_done, pd.n_rebuilds) == (pr.iteration, pr.steps_done, pr.n_rebuilds)
    info = dd.multi_info()
    assert info.world == world and info.n_local == world and info.axis == axis
    cfg = ref.cfg
    H, D = cfg.H, ref.D
    F = _fluid(ref)
    cuts = [(c - 0.5) * H for c in info.cuts[:world - 1]]                          # cell column c covers |x/H - c| <= 1/2
    rng = np.random.default_rng(53)
    lo, hi = F.min(0) - 0.9 * H, F.max(0) + 0.9 * H
    from test_point_gradients_host import IRR
    pts = [rng.uniform(lo, hi, (500, D)) + IRR[:D] * cfg.dx]
    for xc in cuts:
        for shift in (0.0, -0.3 * H, 0.3 * H):
            q = rng.uniform(lo, hi, (30, D)) + IRR[:D] * cfg.dx
            q[:, axis] = xc + shift
            pts.append(q)
    pts = np.concatenate(pts)
    pts = pts[rng.permutation(len(pts))]
    one, gb, refsum = _check_cloud(ref, pts, fb, f"{case} one device")
    got = dd.sample_point_moments(pts)
    ga = _named(got)
    tol = 1e-9 if fb == 8 else 1e-5
    fig = _figures(ga, gb)
    differ = ga["n"] != gb["n"]
    print(f"{case} fp{8 * fb} {world} slabs axis {axis}: {len(pts)} points, n differs at {int(differ.sum())}, near the cut {int(refsum['near'].sum())}; "
          + ", ".join(f"{q} {v:.3g}" for q, v in fig.items()) + f" (bar {tol:g})")
    _check_counts(ga["n"], refsum["n"], refsum["near"], fb)                        # n as in test 1: against the enumeration
    assert not (differ & ~refsum["near"]).any() and differ.sum() <= 0.02 * len(differ)
    for q, v in fig.items():
        assert v <= tol, (q, v, tol)
    at_cut = np.abs(pts[:, axis] - cuts[0]) <= 0.3 * H + 1e-12
    assert at_cut.sum() >= 90 and (one["count"][at_cut] > 0).any()                 # points on and next to the cut lie in water
    _same_bits(dd.sample_point_moments(pts), got, "slab order: the same bits every time")
    ref.close(); dd.close()


# ---- 5. errors; the call changes nothing ------------------------------------------------------------------------------------------
def test_errors(request):
    from sphexample_amd._abi import ERR_ARGUMENT, ERR_STATE, MAX_SAMPLE_POINTS, OK, SphmiError
    from sphexample_amd.engine import rccl_unique_id
    p, s = _state("dam_break_2d", request)
    F = p.Position[p.Type == 1].astype(np.float64)
    pts = F[:: max(len(F) // 40, 1)][:40] + 0.013

    def status(e, call, x):
        with pytest.raises(SphmiError) as ei:
            getattr(e, call)(x)
        return ei.value.status, str(ei.value)

    def family(e, x):
        """The refusal next to sphmi_sample_points' on the same handle and cloud: the same status, the same text behind the name."""
        (sa, ta), (sb, tb) = status(e, "sample_point_moments", x), status(e, "sample_points", x)
        print(f"  {ta!r} / {tb!r}")
        assert sa == sb and "sphmi_sample_point_moments" in ta and ta.replace("sphmi_sample_point_moments", "sphmi_sample_points") == tb, (ta, tb)
        return sa, ta
    eng = _engine(p, s, 8)
    assert family(eng, pts)[0] == ERR_STATE                                        # uploaded, no step yet: no cell list
    eng.advance(1e9, max_steps=5)
    ok = eng.sample_point_moments(pts)
    assert ok["weight"].max() > 0.5
    f = eng._fn("sample_point_moments")
    assert f.argtypes == [C.c_void_p, C.c_int64] + [C.c_void_p] * 11
    x = np.ascontiguousarray(pts)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)                                   # noqa: E731
    last_error = lambda: (eng._fn("last_error")(eng._h) or b"").decode()           # noqa: E731
    assert f(eng._h, len(x), None, *[None] * 10) == ERR_ARGUMENT and "null positions" in last_error()      # null positions with n > 0
    assert f(eng._h, -1, ptr(x), *[None] * 10) == ERR_ARGUMENT
    assert f(eng._h, MAX_SAMPLE_POINTS + 1, ptr(x), *[None] * 10) == ERR_ARGUMENT and "SPHMI_MAX_SAMPLE_POINTS" in last_error()      # too many points
    assert f(eng._h, 0, None, *[None] * 10) == OK                                  # an empty cloud is legal
    assert f(eng._h, len(x), ptr(x), *[None] * 10) == OK                           # every output NULL
    y = x.copy(); y[17, 0] = np.nan
    st, text = family(eng, y)
    assert st == ERR_ARGUMENT and "point 17" in text
    _same_bits(eng.sample_point_moments(pts), ok, "after refused calls")
    assert eng.advance(1e9, max_steps=2).steps_done == 2                           # … and the handle still steps
    thin = _engine(p, _variant(s, None, 0.9), 8)                                   # handles with H < h
    st, text = family(thin, pts)
    assert st == ERR_STATE and "H < h" in text
    thin.close()
    rk = _engine(p, s, 8, rank=0, world=1, unique_id=rccl_unique_id())              # rank-mode handles: one slab of the rows per process
    st, text = family(rk, pts)
    assert st == ERR_STATE and "rank-mode" in text
    eng.close(); rk.close()


@pytest.mark.parametrize("case,fb", [("dam_break_2d", 4), ("dam_break_3d_shipped", 8)])
def test_does_not_disturb(case, fb, request):
    """A run with calls between the steps and a run without: the progress, the downloads and a probe series enabled alongside are
    equal bit for bit; a download before and after one call compares equal; the sibling samplers' plans and arenas survive."""
    fixture, _, _ = CASES[case]
    p, s = _state(fixture, request)
    F = p.Position[p.Type == 1]
    D = F.shape[1]
    calls = (40, 1, 33, 7) if D == 2 else (12, 1, 9)
    runs = []
    for sampled in (False, True):
        eng = _engine(p, s, fb)
        H = eng.cfg.H
        pts = np.random.default_rng(61).uniform(F.min(0) - 2 * H, F.max(0) + 2 * H, (900, D))
        probes = F[:: max(len(F) // 24, 1)][:24] + 0.3 * eng.cfg.dx
        eng.probes_enable(probes, capacity=200)
        prog, seen = [], []
        for n in calls:
            q = eng.advance(1e9, max_steps=n)
            prog.append((q.iteration, q.steps_done, q.n_rebuilds, q.index_counter, q.total_time, q.last_dt, q.delta_x))
            if sampled:
                before, held = eng.sample_point_gradients(pts), eng.download()
                m = eng.sample_point_moments(pts)
                after, now = eng.sample_point_gradients(pts), eng.download()
                for k in before:
                    np.testing.assert_array_equal(after[k], before[k], err_msg=k)  # the gradient sampler's plan and arena survive the call
                for k in held:
                    np.testing.assert_array_equal(now[k], held[k], err_msg=k)      # a download before and after
                seen.append(m)
        runs.append((prog, eng.download(), eng.probes_read(), seen))
        eng.close()
    assert runs[0][0] == runs[1][0]                                                # the progress blocks
    for k, v in runs[0][1].items():
        np.testing.assert_array_equal(runs[1][1][k], v, err_msg=k)                  # the downloads, bit for bit
    assert len(runs[0][2]["iteration"]) == sum(calls)
    for k in runs[0][2]:
        np.testing.assert_array_equal(runs[1][2][k], runs[0][2][k], err_msg=k)      # the probe series
    print(f"{case} fp{8 * fb}: {len(calls)} moment calls between {sum(calls)} steps; downloads and probe series equal")
    assert all(np.abs(m["weight"]).max() > 0.5 and np.abs(m["moment_velocity"]).max() > 0 for m in runs[1][3])
