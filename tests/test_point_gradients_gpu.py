"""Kernel sums and gradient sums at arbitrary points (sphmi_sample_point_gradients, csrc/sphmi_point_gradients.h) — needs a real
MI355X.

The reference is `brute_force_point_gradients` of tests/test_point_gradients_host.py: an O(M·N) numpy enumeration written from the
definition (pinned there by closed forms), fed the cloud and a download taken right after the call.  It never calls the library.

Bars (the project's for a single evaluation, tests/test_probes_gpu.py): every RAW sum — S, SP, Sρ, Sv, G, GP, Gρ, Gv — within 1e-10
of that sum's largest magnitude over the cloud on fp64 handles, 2e-4 on fp32 handles; n equal at every point on fp64; on fp32 a
point may differ only where the reference itself shows a Fluid row within 1e-6·H of the cut, at most 2 % of the points, and the
reference alone must stay under that cap.  S, n, SP, Sρ and Sv against sphmi_sample_points on the same cloud: the same bits (the
kernel forms them with the statements of k_point_cloud; that call delivers SP / S, so the quotient of the raw sums is compared,
a correctly rounded division on both sides).  Slab handles against the one-device handle: 1e-9 / 1e-5, the bars of
tests/test_sample_points_gpu.py::test_slabs_in_one_handle.  What a point reads must not depend on the other points of the call:
np.array_equal on every output.
"""
import ctypes as C

import numpy as np
import pytest

from test_point_gradients_host import IRR, KEYS, SUMS, brute_force_point_gradients, gradient_cloud
from test_probes_gpu import BAR, FIELDS, _engine, _state, _variant

pytestmark = pytest.mark.gpu

CASES = {  # name → (fixture, steps, kernel variant)
    "dam_break_2d": ("dam_break_2d", 30, None),
    "dam_break_3d_shipped": ("dam_break_3d_shipped", 12, None),
    "moving_square": ("moving_square", 25, None),                  # k < 2: H + h spans five cells per axis
    "cubic_spline": ("dam_break_2d", 30, "cubic"),
}


def _start(case, fb, request, **kw):
    fixture, K, kernel = CASES[case]
    p, s = _state(fixture, request)
    if kernel:
        s = _variant(s, kernel, None)
    eng = _engine(p, s, fb, **kw)
    return eng, p, s, K


def _named(out):
    """The dict of sample_point_gradients by the names of the sums."""
    return {KEYS[k]: v for k, v in out.items()}


def _figures(got, ref):
    out = {}
    for q in SUMS:
        scale = np.abs(ref[q]).max()
        out[q] = np.abs(got[q] - ref[q]).max() / scale if scale > 0 else np.abs(got[q]).max()
    return out


def _check_counts(got_n, ref_n, near, fb, cap_on_reference=True):
    differ = got_n != ref_n
    if cap_on_reference:
        assert near.sum() <= 0.02 * len(near), "the cloud itself has too many points with a row at the cut"
    if fb == 8:
        assert not differ.any(), np.flatnonzero(differ)
    else:
        assert not (differ & ~near).any(), np.flatnonzero(differ & ~near)          # excused only where the reference shows a row at the cut
        assert differ.sum() <= 0.02 * len(differ)
    return differ


def _check_cloud(eng, pts, fb, what):
    """Sample, download right after, enumerate; prints every figure before it asserts.  Returns (out, named, ref)."""
    out = eng.sample_point_gradients(pts)
    d = eng.download(FIELDS)
    M = len(pts)
    assert list(out) == list(KEYS) and out["count"].dtype == np.int64
    assert out["weight"].shape == (M,) and out["grad_pressure"].shape == (M, 3) and out["grad_velocity"].shape == (M, 3, 3)
    got = _named(out)
    ref = brute_force_point_gradients(eng.cfg, pts, d["Position"], d["Velocity"], d["Density"], d["Pressure"], d["Type"])
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
        assert (got["Sv"][:, 2] == 0).all() and (got["G"][:, 2] == 0).all() and (got["GP"][:, 2] == 0).all() and (got["Grho"][:, 2] == 0).all()
        assert (got["Gv"][:, 2, :] == 0).all() and (got["Gv"][:, :, 2] == 0).all()
    return out, got, ref


def _same_bits(a, b, what, rows=None):
    for k in KEYS:
        x = a[k] if rows is None else a[k][rows]
        assert np.array_equal(x, b[k]), (what, k, int((x != b[k]).sum()))


def _fluid(eng):
    d = eng.download(FIELDS)
    return d["Position"][d["Type"] == 1].astype(np.float64)


def _one_cell(F, H, rng, count):
    """`count` points inside the ONE cell (|x/H − c| < ½ per axis) that holds a Fluid row: inside one block of cells."""
    c = np.round(F[len(F) // 2] / H)
    pts = (c + rng.uniform(-0.45, 0.45, (count, F.shape[1]))) * H
    assert len(np.unique(np.round(pts / H), axis=0)) == 1
    return pts


# ---- 1. equals the enumeration ----------------------------------------------------------------------------------------------------
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
    assert np.abs(ref["Gv"]).max() > 0 and np.abs(ref["GP"]).max() > 0
    # what the sums are for: the helpers give finite gradients where there is fluid and NaN where there is not
    from sphexample_amd.fields import pressure_gradient, vorticity_at
    w, gp = vorticity_at(out), pressure_gradient(out)
    wet = out["weight"] >= 0.5
    assert wet.sum() > 50 and np.isfinite(w[wet]).all() and np.isfinite(gp[wet]).all() and np.isnan(w[out["weight"] == 0]).all()
    eng.close()


# ---- 2. agrees with the existing sampler ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,fb", [("dam_break_2d", 8), ("dam_break_2d", 4), ("dam_break_3d_shipped", 8), ("dam_break_3d_shipped", 4), ("cubic_spline", 8)])
def test_agrees_with_sample_points(case, fb, request):
    eng, p, s, K = _start(case, fb, request)
    eng.advance(1e9, max_steps=K)
    pts = gradient_cloud(_fluid(eng), eng.cfg.H, eng.cfg.dx, seed=11)
    g = eng.sample_point_gradients(pts)
    c = eng.sample_points(pts)
    S, n = g["weight"], g["count"]
    some = (n > 0) & (S > 0)
    safe = np.where(some, S, 1.0)
    mean = lambda a: np.where(some if a.ndim == 1 else some[:, None], a / (safe if a.ndim == 1 else safe[:, None]), 0.0)      # noqa: E731
    same = {"S": np.array_equal(S, c["weight"]), "n": np.array_equal(n, c["count"]), "SP / S": np.array_equal(mean(g["sum_pressure"]), c["pressure"]),
            "Srho / S": np.array_equal(mean(g["sum_density"]), c["density"]), "Sv / S": np.array_equal(mean(g["sum_velocity"]), c["velocity"])}
    worst = {"S": np.abs(S - c["weight"]).max(), "SP / S": np.abs(mean(g["sum_pressure"]) - c["pressure"]).max()}
    print(f"{case} fp{8 * fb}: {len(pts)} points, {int(some.sum())} see fluid; bit-equal to sphmi_sample_points: {same}; largest difference {worst}")
    assert some.sum() > 100
    assert all(same.values()), same
    eng.close()


# ---- 3. tile edges and independence -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,fb", [("dam_break_2d", 8), ("dam_break_2d", 4), ("dam_break_3d_shipped", 4), ("dam_break_3d_shipped", 8)])
def test_tile_edges_and_independence(case, fb, request):
    eng, p, s, K = _start(case, fb, request)
    eng.advance(1e9, max_steps=K)
    F = _fluid(eng)
    H, D = eng.cfg.H, eng.D
    rng = np.random.default_rng(17)
    # 1, 255, 256, 257 and 1 025 points inside one block: a tile with one lane, one short of full, full, full and a lane, four and a lane
    for count in (1, 255, 256, 257, 1025):
        out, got, ref = _check_cloud(eng, _one_cell(F, H, rng, count), fb, f"{case} {count} points in one block")
        assert (ref["n"] > 0).all()
    # wholly outside the grid: all zeros
    d = eng.download(FIELDS)
    X = d["Position"].astype(np.float64)
    outside = np.concatenate([X.min(0) - np.array([3.3 * H, 7 * H, 100.0][:D]) * np.ones((1, D)), X.max(0) + 3.3 * H + rng.uniform(0, 1e6, (40, D))])
    far = eng.sample_point_gradients(outside)
    for k in KEYS:
        assert (far[k] == 0).all(), k
    # a permuted cloud, a cloud with extra points, a point alone, the same call twice: a point's bits do not change
    pts = gradient_cloud(F, H, eng.cfg.dx, seed=23, count=1500)
    full = eng.sample_point_gradients(pts)
    assert (full["count"] > 0).sum() > 200
    _same_bits(eng.sample_point_gradients(pts), full, "the same call twice")
    perm = np.random.default_rng(29).permutation(len(pts))
    _same_bits(full, eng.sample_point_gradients(pts[perm]), "the cloud permuted", rows=perm)
    extra = np.concatenate([_one_cell(F, H, rng, 300), pts, outside])
    _same_bits(eng.sample_point_gradients(extra), full, "the cloud with 300 points in front and the outside behind", rows=slice(300, 300 + len(pts)))
    inside = int(np.flatnonzero(full["count"] > 0)[0])
    _same_bits(full, eng.sample_point_gradients(pts[inside:inside + 1]), "a point in a call of its own", rows=slice(inside, inside + 1))
    # a subset of the outputs: the others travel as NULL, the bits stay
    part = eng.sample_point_gradients(pts, fields=("grad_velocity", "count"))
    assert set(part) == {"grad_velocity", "count"} and np.array_equal(part["grad_velocity"], full["grad_velocity"]) and np.array_equal(part["count"], full["count"])
    assert eng.sample_point_gradients(np.zeros((0, D)))["grad_velocity"].shape == (0, 3, 3)      # an empty cloud is legal
    eng.close()


# ---- 4. does not disturb ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,fb", [("dam_break_2d", 4), ("dam_break_3d_shipped", 8)])
def test_does_not_disturb(case, fb, request):
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
                before = eng.sample_points(pts)
                g = eng.sample_point_gradients(pts)
                after = eng.sample_points(pts)
                for k in before:
                    np.testing.assert_array_equal(after[k], before[k], err_msg=k)  # the cloud sampler's plan and arena survive the call
                seen.append(g)
        runs.append((prog, eng.download(), eng.probes_read(), seen))
        eng.close()
    assert runs[0][0] == runs[1][0]                                                # the progress blocks
    for k, v in runs[0][1].items():
        np.testing.assert_array_equal(runs[1][1][k], v, err_msg=k)                  # the downloads, bit for bit
    assert len(runs[0][2]["iteration"]) == sum(calls)
    for k in runs[0][2]:
        np.testing.assert_array_equal(runs[1][2][k], runs[0][2][k], err_msg=k)      # the probe series
    print(f"{case} fp{8 * fb}: {len(calls)} gradient calls between {sum(calls)} steps; downloads and probe series equal")
    assert all(np.abs(g["weight"]).max() > 0.5 and np.abs(g["grad_velocity"]).max() > 0 for g in runs[1][3])


# ---- 5. slabs in one handle -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("case,fb,axis", [("dam_break_2d", 8, 0), ("dam_break_2d", 4, 0), ("dam_break_2d", 8, 1), ("dam_break_2d", 4, 1),
                                          ("dam_break_3d_shipped", 4, 0), ("dam_break_3d_shipped", 8, 1)])
def test_slabs_in_one_handle(case, fb, axis, world, request):
    """Every slab bins and samples the whole cloud over the rows it owns, the handle adds the raw sums in slab order.  Some points lie
    ON the first cut (the face between two slabs' cell columns), others 0.3·H to either side: a ghost copy that counted would
    double their sums, a skipped owner halve them."""
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
    pts = [rng.uniform(lo, hi, (500, D)) + IRR[:D] * cfg.dx]
    for xc in cuts:
        for shift in (0.0, -0.3 * H, 0.3 * H):
            q = rng.uniform(lo, hi, (30, D)) + IRR[:D] * cfg.dx
            q[:, axis] = xc + shift
            pts.append(q)
    pts = np.concatenate(pts)
    pts = pts[rng.permutation(len(pts))]
    one, gb, refsum = _check_cloud(ref, pts, fb, f"{case} one device")
    got = dd.sample_point_gradients(pts)
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
    _same_bits(dd.sample_point_gradients(pts), got, "slab order: the same bits every time")
    ref.close(); dd.close()


# ---- 6. errors --------------------------------------------------------------------------------------------------------------------
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
        """The refusal of the gradients next to sphmi_sample_points' on the same handle and cloud: the same status, the same text
        behind the name of the function."""
        (sa, ta), (sb, tb) = status(e, "sample_point_gradients", x), status(e, "sample_points", x)
        print(f"  {ta!r} / {tb!r}")
        assert sa == sb and "sphmi_sample_point_gradients" in ta and ta.replace("sphmi_sample_point_gradients", "sphmi_sample_points") == tb, (ta, tb)
        return sa, ta
    eng = _engine(p, s, 8)
    assert family(eng, pts)[0] == ERR_STATE                                        # uploaded, no step yet: no cell list
    eng.advance(1e9, max_steps=5)
    ok = eng.sample_point_gradients(pts)
    assert ok["weight"].max() > 0.5
    f = eng._fn("sample_point_gradients"); f.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 10
    x = np.ascontiguousarray(pts)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)                                   # noqa: E731
    last_error = lambda: (eng._fn("last_error")(eng._h) or b"").decode()           # noqa: E731
    assert f(eng._h, len(x), None, *[None] * 9) == ERR_ARGUMENT and "null positions" in last_error()      # null positions with n > 0
    assert f(eng._h, -1, ptr(x), *[None] * 9) == ERR_ARGUMENT
    assert f(eng._h, MAX_SAMPLE_POINTS + 1, ptr(x), *[None] * 9) == ERR_ARGUMENT and "SPHMI_MAX_SAMPLE_POINTS" in last_error()      # too many points
    assert f(eng._h, 0, None, *[None] * 9) == OK                                   # an empty cloud is legal
    assert f(eng._h, len(x), ptr(x), *[None] * 9) == OK                            # every output NULL
    y = x.copy(); y[17, 0] = np.nan
    st, text = family(eng, y)
    assert st == ERR_ARGUMENT and "point 17" in text
    _same_bits(eng.sample_point_gradients(pts), ok, "after refused calls")
    assert eng.advance(1e9, max_steps=2).steps_done == 2                           # … and the handle still steps
    thin = _engine(p, _variant(s, None, 0.9), 8)                                   # handles with H < h
    st, text = family(thin, pts)
    assert st == ERR_STATE and "H < h" in text
    thin.close()
    rk = _engine(p, s, 8, rank=0, world=1, unique_id=rccl_unique_id())              # rank-mode handles: one slab of the rows per process
    st, text = family(rk, pts)
    assert st == ERR_STATE and "rank-mode" in text
    eng.close(); rk.close()
