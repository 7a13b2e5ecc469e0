"""The flow through control boxes recorded on the device at every step (sphmi_flow_enable / sphmi_flow_read, csrc/sphmi_flow.h) —
needs a real MI355X.

Raw record of a step and a box, over the Fluid rows (x, v, rho the doubles of a download; a row is INSIDE iff lo <= x < hi per axis):
    0 n_after | 1 sum 1/rho over the rows inside after the step | 2-4 sum v over them | 5 entered | 6 left
and the read delivers count = n_after, volume = m0 s1, momentum = m0 s2..4, entered, left.

Every comparison is against downloads of the SAME handle.
  * count, entered, left: exact.  entered / left of a step against sphexample_amd.flow.restate of the download before it and the
    download after it (rows matched by ID: a rebuild permutes them).
  * volume, momentum: device and test add the same doubles (1/rho is one correctly rounded fp64 division on both sides) in a
    different order, |device - fsum(terms)| <= n eps sum|term|, eps = 2^-52, n the rows inside — the derived bar of
    test_budgets_gpu.py — scaled by m0, plus 2 ulp of the delivered value for the one multiplication on either side.

The stock layouts start at rest: like test_budgets_gpu.py the cases run from `perturbed(p, seed=3, vel_scale=3.0)`, which crosses
Δx-triggered rebuilds within the batch whose series is checked (asserted from the growth of sphmi_progress.n_rebuilds over that call).  The boxes of a checked step are cut from the
download before it (`box_set`): their faces lie on coordinates rows hold exactly, where the half-open rule decides."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import perturbed
from sphexample_amd import flow
from sphexample_amd._abi import ERR_ARGUMENT, ERR_STATE, SphmiError

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
INF = np.inf
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# case → steps from the perturbed state; the batch of K − 2 steps crosses at least two Δx-triggered rebuilds (the 3-D and the 512-row
# case run longer than test_budgets_gpu.py's horizons for that)
STEPS = {"dam_break_2d": 100, "moving_square": 40, "dam_break_3d_shipped": 45, "small": 150}
ROWS = {"dam_break_2d": 6881, "dam_break_3d_shipped": 17446}
CASES = ["dam_break_2d", "dam_break_3d_shipped", "moving_square", "small"]
FIELDS = ("Position", "Velocity", "Density", "Type", "ID")
# boxes of box_set: the strips along x, the strips along the last axis, everything, nothing, two overlapping, two on exact x
X_STRIPS, L_STRIPS, ALL, EMPTY, OVERLAP, EXACT = slice(0, 6), slice(6, 10), 10, 11, slice(12, 14), slice(14, 16)


def small_case(p0):
    """The one-launch path: 400 Fluid rows of the 2-D layout — the 20 x 20 block in the corner of the column, so that the cloud has
    twenty distinct coordinates per axis for the faces of `box_set` — and the Fixed rows nearest to them, at most 512 rows."""
    from sphexample_amd import particles_from_arrays
    x = p0.Position
    is_fluid = p0.Type == 1
    in_block = is_fluid & (x[:, 0] <= np.unique(x[is_fluid, 0])[19]) & (x[:, 1] <= np.unique(x[is_fluid, 1])[19])
    fluid = np.nonzero(in_block)[0]
    assert len(fluid) == 400
    centre = x[fluid].mean(0)
    fixed = np.nonzero(~is_fluid)[0]
    near = fixed[np.argsort(((x[fixed] - centre) ** 2).sum(1), kind="stable")[:112]]
    keep = np.sort(np.concatenate([fluid, near]))
    assert len(keep) == 512
    return particles_from_arrays(2, x[keep], p0.Density[keep], p0.Type[keep], p0.GroupMarker[keep], p0.ID[keep])


def _state(case, request, vel=3.0):
    if case == "small":
        p0, s = request.getfixturevalue("dam_break_2d")
        return perturbed(small_case(p0), seed=3, vel_scale=vel), s
    p0, s = request.getfixturevalue(case)
    p = perturbed(p0, seed=3, vel_scale=vel)
    if hasattr(p0, "geometries"):
        p.geometries = p0.geometries
    return p, s


def _engine(p, s, fb, **kw):
    from sphexample_amd.engine import make_engine
    return make_engine(p, s, device_float_bytes=fb, **kw)


def box_set(d):
    """The 16 boxes of the module, cut from the download `d`: every face along x and along the last axis lies on a coordinate some
    Fluid row holds exactly — a row that moves towards smaller coordinates at a quarter of the largest speed along that axis or
    more, so that the coming step takes it across the face: out of the box that starts there, into the one that ends there.
    (lo, hi), each [16, dims]."""
    fluid = d["Type"] == 1
    x, v = d["Position"][fluid].astype(np.float64), d["Velocity"][fluid].astype(np.float64)
    dims, last = x.shape[1], x.shape[1] - 1

    def at(axis, q):
        """the coordinates of such rows at the quantiles `q` of their distinct coordinates"""
        c = np.unique(x[v[:, axis] <= -0.25 * np.abs(v[:, axis]).max(), axis])
        return c[(np.asarray(q) * (len(c) - 1)).astype(int)]

    lo_x, hi_x = flow.strips(0, at(0, [0.15, 0.3, 0.5, 0.7, 0.85]), dims)
    lo_l, hi_l = flow.strips(last, at(last, [0.25, 0.5, 0.75]), dims)
    lo = [*lo_x, *lo_l, np.full(dims, -INF), np.full(dims, 1000.0)]
    hi = [*hi_x, *hi_l, np.full(dims, INF), np.full(dims, 1001.0)]
    # two finite boxes that overlap each other (and the strips); 3-D: a face through the fluid along the middle axis too
    for qa, qb, qt, qm in ((0.2, 0.6, 0.6, 0.85), (0.4, 0.9, 0.8, 0.95)):
        a, b = np.full(dims, -50.0), np.full(dims, 50.0)
        a[0], b[0], b[last] = at(0, qa), at(0, qb), at(last, qt)
        if dims == 3:
            b[1] = at(1, qm)
        lo.append(a); hi.append(b)
    # two adjacent boxes along x whose faces are the exact x of three Fluid rows, unbounded otherwise
    e = at(0, [0.35, 0.55, 0.65])
    for k in range(2):
        a, b = np.full(dims, -INF), np.full(dims, INF)
        a[0], b[0] = e[k], e[k + 1]
        lo.append(a); hi.append(b)
    lo, hi = np.array(lo), np.array(hi)
    assert lo.shape == hi.shape == (16, dims) and (lo < hi).all()
    on_face = (x[:, None, 0] == lo[None, :, 0]) | (x[:, None, 0] == hi[None, :, 0])
    assert on_face[:, EXACT].any(0).all()                        # rows sit exactly on the faces: equal doubles are compared
    return lo, hi


def _check_content(f, k, d, lo, hi, m0, label):
    """Sample k of the series `f` against the download `d`: count exactly, volume and momentum within the module's bar."""
    fluid = d["Type"] == 1
    member = flow.inside(d["Position"][fluid], lo, hi)
    D = d["Position"].shape[1]
    V = np.zeros((int(fluid.sum()), 3))
    V[:, :D] = d["Velocity"][fluid].astype(np.float64)
    terms = np.concatenate([(1.0 / d["Density"][fluid].astype(np.float64))[:, None], V], axis=1)
    np.testing.assert_array_equal(f["count"][k], member.sum(0))
    for b in range(len(lo)):
        n = int(member[:, b].sum())
        got = np.concatenate([[f["volume"][k, b]], f["momentum"][k, b]])
        for slot in range(4):
            t = terms[member[:, b], slot]
            want = m0 * math.fsum(t)
            bound = m0 * n * EPS * math.fsum(np.abs(t)) + 2.0 * EPS * abs(got[slot])
            err = abs(got[slot] - want)
            print(f"{label} box {b} slot {slot + 1}: n {n} device {got[slot]:.17g} download {want:.17g} |diff| {err:.3g} bound {bound:.3g}")
            assert err <= bound, (b, slot, got[slot], want, err, bound)
        if n == 0:
            assert (got == 0).all() and not np.signbit(got).any()
    if D == 2:
        assert (f["momentum"][:, :, 2] == 0).all()


def _check_conservation(f, n_before, n_fluid, label):
    """The identities of a series: count[k] − count[k−1] == entered[k] − left[k] (k = 0: against `n_before`, the counts of the
    download before the first step), tilings hold every Fluid row once, and what leaves one strip enters another."""
    prev = np.concatenate([np.asarray(n_before)[None, :], f["count"][:-1]])
    np.testing.assert_array_equal(f["count"] - prev, f["entered"] - f["left"])
    for tiling in (X_STRIPS, L_STRIPS):
        assert (f["count"][:, tiling].sum(1) == n_fluid).all(), label
        np.testing.assert_array_equal(f["entered"][:, tiling].sum(1), f["left"][:, tiling].sum(1))
    assert (f["count"][:, ALL] == n_fluid).all() and (f["entered"][:, ALL] == 0).all() and (f["left"][:, ALL] == 0).all()
    for key in ("count", "entered", "left", "volume"):
        assert (f[key][:, EMPTY] == 0).all(), key
    assert (f["momentum"][:, EMPTY] == 0).all()
    assert (f["entered"] >= 0).all() and (f["left"] >= 0).all()


def _busy(r):
    """Boxes with at least one entry AND one exit in the restated step `r`."""
    return int(((r["entered"] > 0) & (r["left"] > 0)).sum())


def _one_step(eng, m0, label, extra=()):
    """Download, cut the boxes from it, one step, download: entered and left equal the host restatement, box by box."""
    d0 = eng.download(FIELDS)
    lo, hi = box_set(d0)
    eng.flow_enable(lo, hi, capacity=4)
    pr = eng.advance(1e9, max_steps=1)
    assert pr.steps_done == 1
    f = eng.flow_read()
    d1 = eng.download(FIELDS + extra)
    assert len(f["iteration"]) == 1 and int(f["iteration"][0]) == pr.iteration
    r = flow.restate(d0, d1, lo, hi)
    print(f"{label}: entered {f['entered'][0].tolist()} left {f['left'][0].tolist()} (restated {r['entered'].tolist()} / {r['left'].tolist()})")
    assert _busy(r) >= 2, (label, r)                             # a comparison of zeros would show nothing
    for key in ("count", "entered", "left"):
        np.testing.assert_array_equal(f[key][0], r[key], err_msg=f"{label}: {key}")
    _check_content(f, 0, d1, lo, hi, m0, label)
    return d1, pr


def _whole(eng, p, s, K, label, extra=(), after_first=None):
    """Tests 1–3 on one handle: the first step exactly, a batch of K − 2 steps with rebuilds (conservation, the budgets' count, the
    last sample against the download), then one more step exactly.  Returns the downloads after step 1 and after step K − 1."""
    m0 = s.SimConstants.m0
    n_fluid = int((p.Type == 1).sum())
    d1, first = _one_step(eng, m0, f"{label} step 1", extra)
    if after_first:
        after_first()
    lo, hi = box_set(d1)
    n_before = flow.restate(d1, d1, lo, hi)["count"]
    eng.flow_enable(lo, hi, capacity=K + 8)
    eng.budgets_enable(capacity=K + 8)
    pr = eng.advance(1e9, max_steps=K - 2)
    # n_rebuilds counts over the life of the handle and every call opens with a rebuild: the difference to the first call's block
    # is the opener of THIS call plus the Δx-triggered rebuilds inside its batch
    inside = pr.n_rebuilds - first.n_rebuilds
    print(f"{label}: {inside} rebuilds in the call of {K - 2} steps (the opener and {inside - 1} triggered by Δx)")
    assert pr.steps_done == K - 2 and pr.iteration == K - 1 and inside >= 2, (first.n_rebuilds, pr.n_rebuilds)
    f, b = eng.flow_read(), eng.budgets_read()
    assert len(f["iteration"]) == K - 2 and eng.flow_dropped == 0
    np.testing.assert_array_equal(f["iteration"], np.arange(2, K))
    for key in ("iteration", "time", "dt"):
        np.testing.assert_array_equal(f[key], b[key])
    assert f["count"].shape == (K - 2, 16) and f["momentum"].shape == (K - 2, 16, 3)
    _check_conservation(f, n_before, n_fluid, label)
    for tiling in (X_STRIPS, L_STRIPS):
        np.testing.assert_array_equal(f["count"][:, tiling].sum(1), b["count"])
    assert f["entered"][:, X_STRIPS].sum() > 0 and f["entered"][:, OVERLAP].sum() > 0
    # iteration, time and dt of the last sample are the progress block, bit for bit
    assert (int(f["iteration"][-1]), float(f["time"][-1]), float(f["dt"][-1])) == (pr.iteration, pr.total_time, pr.last_dt)
    d = eng.download(FIELDS + extra)
    _check_content(f, K - 3, d, lo, hi, m0, f"{label} step {K - 1}")
    eng.budgets_enable(capacity=0)
    _one_step(eng, m0, f"{label} step {K}")          # (its own boxes, cut from the state before it)
    return d1, d


@pytest.mark.parametrize("fb", [8, 4])
@pytest.mark.parametrize("case", CASES)
def test_content_one_step_and_conservation(case, fb, request):
    p, s = _state(case, request)
    if case in ROWS:
        assert len(p) == ROWS[case]                              # 26 blocks + a ragged one / 69 blocks: the final stride wraps
    if case == "moving_square":
        assert set(np.unique(p.Type)) == {1, 2, 3}               # Fixed, Moving and Fluid rows: only Fluid counts
    if case == "small":
        assert len(p) <= 512                                     # one launch (k_fl_small)
    eng = _engine(p, s, fb)
    _whole(eng, p, s, STEPS[case], f"{case} fp{8 * fb}")
    eng.close()


CHILD = """
import sys
import numpy as np
sys.path[:0] = [{root!r}, {tests!r}]
from conftest import load_dam_break_2d, perturbed
from test_flow_gpu import FIELDS, box_set
from sphexample_amd.engine import make_engine
p0, s = load_dam_break_2d()
eng = make_engine(perturbed(p0, seed=3, vel_scale=3.0), s, device_float_bytes=4)
lo, hi = box_set(eng.download(FIELDS))
eng.flow_enable(lo, hi, capacity=64)
pr = eng.advance(1e9, max_steps=30)
f = eng.flow_read()
assert len(f["iteration"]) == 30 == pr.iteration, len(f["iteration"])
np.savez({out!r}, **f)
eng.close()
"""


def test_one_launch_and_two_stages_give_the_same_bytes(tmp_path):
    """$SPHMI_FLOW_SMALL_ROWS is read at enable: the default threshold, 0 (always two stages) and 8192 (one launch for the 6 881
    rows of this case), each in a fresh process — the whole series byte for byte; two default runs too."""
    runs = {"default": None, "two_stage": "0", "one_launch": "8192", "default_again": None}
    procs, series = {}, {}
    try:
        for name, rows in runs.items():
            env = {k: v for k, v in os.environ.items() if k != "SPHMI_FLOW_SMALL_ROWS"}
            if rows is not None:
                env["SPHMI_FLOW_SMALL_ROWS"] = rows
            code = CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), out=str(tmp_path / f"{name}.npz"))
            procs[name] = subprocess.Popen([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        for name, proc in procs.items():
            out, _ = proc.communicate(timeout=300)
            assert proc.returncode == 0, (name, out)
            series[name] = dict(np.load(str(tmp_path / f"{name}.npz")))
    finally:
        for proc in procs.values():              # trouble ends the step: no child outlives a failure or a time limit
            if proc.poll() is None:
                proc.kill()
                proc.communicate()
    ref = series["default"]
    assert len(ref["iteration"]) == 30 and ref["entered"].sum() > 0 and ref["left"].sum() > 0 and (ref["volume"][:, ALL] > 0).all()
    for name in ("two_stage", "one_launch", "default_again"):
        for key in ref:
            assert series[name][key].tobytes() == ref[key].tobytes(), f"{name}: {key}"


def test_slabs_in_one_handle(request):
    """Every slab marks and samples the rows it owns, the handle adds the slabs' records.  The water column straddles the cuts, rows
    change slab in the collective rebuilds, and no box face along the slab axis lies on a cut."""
    p, s = _state("dam_break_3d_shipped", request)
    K = STEPS["dam_break_3d_shipped"]
    dd = _engine(p, s, 4, devices=[0, 0, 0])
    early = []
    d1, d = _whole(dd, p, s, K, "dam_break_3d_shipped fp32 3 slabs", extra=("Cells",), after_first=lambda: early.append(dd.multi_info()))
    info = dd.multi_info()
    assert info.world == 3 and info.n_local == 3 and sum(info.n_live[:3]) > len(p)       # ghost copies are held
    axis, cuts = info.axis, list(info.cuts[:2])
    cols = d["Cells"][d["Type"] == 1][:, axis]
    assert any(cols.min() < cut <= cols.max() for cut in cuts)                            # the Fluid rows lie in more than one slab
    # migration: Fluid rows owned by another slab after step K − 1 than after step 1 (a slab owns the cell columns between its cuts)
    slab = lambda dl, c: dict(zip(dl["ID"][dl["Type"] == 1].tolist(), np.searchsorted(c, dl["Cells"][dl["Type"] == 1][:, axis], side="right").tolist()))      # noqa: E731
    s0, s1 = slab(d1, list(early[0].cuts[:2])), slab(d, cuts)
    moved = sum(1 for i in s0 if s0[i] != s1[i])
    print(f"Fluid rows that changed slab between step 1 and step {K - 1}: {moved}; cuts {list(early[0].cuts[:2])} -> {cuts}")
    assert moved > 0
    # No box face of the last checked step (cut from this very state) lies on a cut.  A cut is the plane between the cell column
    # below it and the column it starts; the rows have drifted by less than h < H since the rebuild that assigned their cells, so
    # the plane lies within H of the rows on either side of it.  Faces along the slab axis do pass through the fluid.
    lo, hi = box_set(d)
    faces = np.unique(np.concatenate([lo[:, axis], hi[:, axis]]))
    x, col = d["Position"][:, axis].astype(np.float64), d["Cells"][:, axis]
    fx = x[d["Type"] == 1]
    assert ((faces > fx.min()) & (faces < fx.max())).sum() >= 2, faces
    H = s.SimKernel.H
    for cut in cuts:
        below, above = x[col < cut].max(), x[col >= cut].min()
        print(f"cut {cut}: rows below it up to {below:.6g}, rows above it from {above:.6g}; faces {faces.tolist()}")
        assert abs(above - below) < 2 * H and not ((faces >= min(below, above) - H) & (faces <= max(below, above) + H)).any(), (cut, below, above, faces)
    dd.close()


def test_contract(request):
    from sphexample_amd._abi import make_config
    from sphexample_amd.engine import Engine, rccl_unique_id
    import ctypes as C
    p, s = _state("dam_break_2d", request)
    lo, hi = flow.strips(0, [0.3, 0.6], 2)
    # before the upload
    cfg = make_config(len(p), s.SimConstants, s.SimKernel, s.SimMetaData, s.SimViscosity, s.SimDensityDiffusion, device_float_bytes=8, host_float_bytes=8)
    bare = Engine(cfg)
    for call in (lambda: bare.flow_enable(lo, hi, capacity=4), bare.flow_read):
        with pytest.raises(SphmiError) as ei:
            call()
        assert ei.value.status == ERR_STATE
    bare.close()
    eng = _engine(p, s, 8)
    # read while disabled
    with pytest.raises(SphmiError) as ei:
        eng.flow_read()
    assert ei.value.status == ERR_STATE
    # argument errors: too many boxes, a NaN bound, lo == hi, lo > hi, capacity_steps < 1, null tables, null n_out, negative capacity
    many_lo, many_hi = flow.strips(0, np.arange(16) * 0.1, 2)
    bad = [(many_lo, many_hi, 4), ([[np.nan, 0.0]], [[1.0, 1.0]], 4), ([[0.0, 0.0]], [[1.0, np.nan]], 4), ([[0.0, 0.5]], [[1.0, 0.5]], 4),
           ([[0.0, 0.5]], [[1.0, 0.25]], 4), ([[-INF, 0.0]], [[-INF, 1.0]], 4), (lo, hi, 0), (lo, hi, -1)]
    for a, b, cap in bad:
        with pytest.raises(SphmiError) as ei:
            eng.flow_enable(a, b, capacity=cap)
        assert ei.value.status == ERR_ARGUMENT, (a, b, cap)
    enable = eng._fn("flow_enable")
    enable.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64]
    table = np.zeros(2)
    assert enable(eng._h, 1, None, table.ctypes.data, 4) == ERR_ARGUMENT and enable(eng._h, 1, table.ctypes.data, None, 4) == ERR_ARGUMENT
    assert enable(eng._h, -1, table.ctypes.data, table.ctypes.data, 4) == ERR_ARGUMENT
    with pytest.raises(SphmiError) as ei:                        # a refused enable enabled nothing
        eng.flow_read()
    assert ei.value.status == ERR_STATE
    eng.flow_enable(lo, hi, capacity=6)
    read = eng._fn("flow_read")
    read.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 10
    n = C.c_int64(-1)
    assert read(eng._h, 1, *[None] * 10) == ERR_ARGUMENT                           # null n_out
    assert read(eng._h, -1, *[None] * 8, C.addressof(n), None) == ERR_ARGUMENT     # negative capacity
    # more steps than capacity_steps between two reads: the newest stay, the oldest are counted
    ref = _engine(p, s, 8)
    ref.flow_enable(lo, hi, capacity=100)
    eng.advance(1e9, max_steps=50); ref.advance(1e9, max_steps=50)
    assert read(eng._h, 0, *[None] * 8, C.addressof(n), None) == 0 and n.value == 6          # capacity = 0: how many wait, nothing cleared
    f, r = eng.flow_read(), ref.flow_read()
    assert len(f["iteration"]) == 6 and eng.flow_dropped == 44 and len(r["iteration"]) == 50 and ref.flow_dropped == 0
    for key in f:
        np.testing.assert_array_equal(f[key], r[key][-6:], err_msg=key)
    assert (r["count"].sum(1) == int((p.Type == 1).sum())).all()
    # read clears
    assert len(eng.flow_read()["iteration"]) == 0 and eng.flow_dropped == 0
    # a second enable replaces the boxes and drops the series
    eng.advance(1e9, max_steps=3)
    lo4, hi4 = flow.strips(1, [0.1, 0.2, 0.3], 2)
    eng.flow_enable(lo4, hi4, capacity=8)
    assert len(eng.flow_read()["iteration"]) == 0
    eng.advance(1e9, max_steps=2)
    assert eng.flow_read()["count"].shape == (2, 4)
    # sphmi_forces_once adds no sample
    eng.forces_once()
    assert len(eng.flow_read()["iteration"]) == 0
    # group forces, probes, budgets and flow together: K samples each, the same clock columns
    K = 20
    fluid = p.Position[p.Type == 1]
    eng.flow_enable(lo, hi, capacity=K)
    eng.budgets_enable(capacity=K)
    eng.group_forces_enable([1, 2], capacity=K)
    eng.probes_enable(fluid.mean(0)[None, :], capacity=K)
    pr = eng.advance(1e9, max_steps=K)
    it, t, dt, F = eng.group_forces_read()
    probes, b, f = eng.probes_read(), eng.budgets_read(), eng.flow_read()
    assert len(it) == len(probes["iteration"]) == len(b["iteration"]) == len(f["iteration"]) == K
    for mine, theirs in ((f["iteration"], it), (f["time"], t), (f["dt"], dt)):
        np.testing.assert_array_equal(mine, theirs)
    for key in ("iteration", "time", "dt"):
        np.testing.assert_array_equal(f[key], probes[key])
        np.testing.assert_array_equal(f[key], b[key])
    np.testing.assert_array_equal(f["count"].sum(1), b["count"])
    assert (int(f["iteration"][-1]), float(f["time"][-1]), float(f["dt"][-1])) == (pr.iteration, pr.total_time, pr.last_dt)
    # n_boxes = 0 disables
    eng.flow_enable(np.zeros((0, 2)), np.zeros((0, 2)))
    with pytest.raises(SphmiError) as ei:
        eng.flow_read()
    assert ei.value.status == ERR_STATE
    # the upload disables
    eng.flow_enable(lo, hi, capacity=8)
    eng.upload_particles(p)
    with pytest.raises(SphmiError) as ei:
        eng.flow_read()
    assert ei.value.status == ERR_STATE
    eng.advance(1e9, max_steps=3)
    # rank-mode handles: one slab of the rows per process
    rk = _engine(p, s, 8, rank=0, world=1, unique_id=rccl_unique_id())
    for call in (lambda: rk.flow_enable(lo, hi, capacity=4), rk.flow_read):
        with pytest.raises(SphmiError) as ei:
            call()
        assert ei.value.status == ERR_STATE
    for e in (eng, ref, rk):
        e.close()


def test_run_simulation_hands_the_samples_to_the_callback(dam_break_2d):
    import copy
    from sphexample_amd import simulation
    p, s = dam_break_2d
    meta = copy.deepcopy(s.SimMetaData)
    meta.SimulationTime, meta.OutputTimes = 0.002, 0.001
    lo, hi = flow.strips(0, [0.2, 0.4], 2)
    got = []
    steps = simulation.RunSimulation(SimGeometry=None, SimMetaData=meta, SimConstants=s.SimConstants, SimKernel=s.SimKernel, SimLogger=None,
                                     SimParticles=p.copy(), SimViscosity=s.SimViscosity, SimDensityDiffusion=s.SimDensityDiffusion,
                                     flow_boxes=list(zip(lo, hi)), on_output=lambda m, pp, f: got.append((m.Iteration, m.TotalTime, f)))
    assert len(got) == len(steps) + 1 and len(got[0][2]["iteration"]) == 0 and got[0][2]["count"].shape == (0, 3)
    its = np.concatenate([f["iteration"] for _, _, f in got])
    np.testing.assert_array_equal(its, np.arange(1, got[-1][0] + 1))           # every step of the run, once, in order
    n_fluid = int((p.Type == 1).sum())
    for iteration, time, f in got[1:]:
        assert int(f["iteration"][-1]) == iteration and float(f["time"][-1]) == time and (f["count"].sum(1) == n_fluid).all()
        assert flow.cumulative(f).shape == f["count"].shape == flow.discharge(f, s.SimConstants.m0, s.SimConstants.rho0).shape
