"""The budgets of the fluid recorded on the device at every step (sphmi_budgets_enable / sphmi_budgets_read,
csrc/sphmi_budgets.h) — needs a real MI355X.

Raw record of a step, over the Fluid rows of the state a download delivers directly after it (x, v, rho the doubles of that
download; 2-D: z = vz = 0):
    0 n | 1 sum 1/2((vx vx + vy vy) + vz vz) | 2 sum x_last | 3 sum e(rho) | 4-6 sum v | 7-9 sum x cross v | 10-12 sum x
    13 max |v|^2 | 14, 15 min, max rho | 16-18, 19-21 min, max x
    e(rho) = ((r6 - 1)/6 + 1/r) - 1,  r = rho/rho0,  r2 = r r,  r6 = (r2 r2) r2
and the read delivers count = n, energy = (m0 s1, m0 g s2, m0 (B/rho0) s3), momentum = m0 s4..6, angular = m0 s7..9,
centre = s10..12 / n, extremes = (sqrt(s13), s14, s15), box = s16..21.

Every comparison is against the download of the SAME handle.  The test forms the terms in numpy float64 in the operation order
above — numpy rounds every ufunc call on its own, as the kernel does with contraction off — so the terms are the same doubles:
  * n and the extremes (slots 13-21): exact.  sqrt is correctly rounded on both sides.
  * a sum slot: device and test add the same doubles in a different order, |device - fsum(terms)| <= n eps sum|term|, eps = 2^-52
    (the bar of test_group_forces_gpu.py).  Slot 3 gets 8 n eps on top: e cancels from O(1) intermediates to O(delta^2), and
    the device's divisions are allowed 8 ulp of those per term.
  * the test sees the DELIVERED values, factor * raw or raw / n rounded once, and forms factor * fsum rounded once: 2 ulp of the
    delivered value on top of the scaled bound.

The stock layouts start at rest: like test_group_forces_gpu.py the cases run from `perturbed(p, seed=3, vel_scale=3.0)`, which
crosses Δx-triggered rebuilds within the horizon (asserted from sphmi_progress.n_rebuilds)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import perturbed
from sphexample_amd._abi import ERR_ARGUMENT, ERR_STATE, SphmiError

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# case → steps of one call that cross at least one Δx-triggered rebuild from the perturbed state
STEPS = {"dam_break_2d": 100, "moving_square": 40, "dam_break_3d_shipped": 30}
ROWS = {"dam_break_2d": 6881, "dam_break_3d_shipped": 17446}
FIELDS = ("Position", "Velocity", "Density", "Type")


def _state(case, request, vel=3.0):
    p0, s = request.getfixturevalue(case)
    p = perturbed(p0, seed=3, vel_scale=vel)
    if hasattr(p0, "geometries"):
        p.geometries = p0.geometries
    return p, s


def _engine(p, s, fb, **kw):
    from sphexample_amd.engine import make_engine
    return make_engine(p, s, device_float_bytes=fb, **kw)


def _factors(c):
    """m0, m0 g, m0 (B / rho0) with B = c0^2 rho0 / 7, each formed as the library forms it."""
    return c.m0, c.m0 * c.g, c.m0 * (((c.c0 * c.c0 * c.rho0) / 7.0) / c.rho0)


def _terms(d, rho0):
    """The 13 sum terms [n, 13] and the 9 extremes of a download, in the table's operation order."""
    fluid = d["Type"] == 1
    n, D = int(fluid.sum()), d["Position"].shape[1]
    X, V = np.zeros((n, 3)), np.zeros((n, 3))
    X[:, :D] = d["Position"][fluid].astype(np.float64)
    V[:, :D] = d["Velocity"][fluid].astype(np.float64)
    rho = d["Density"][fluid].astype(np.float64)
    x, y, z = X.T
    vx, vy, vz = V.T
    v2 = (vx * vx + vy * vy) + vz * vz
    r = rho / rho0
    r2 = r * r
    r6 = (r2 * r2) * r2
    T = np.zeros((n, 13))
    T[:, 0] = 1.0
    T[:, 1] = 0.5 * v2
    T[:, 2] = X[:, D - 1]
    T[:, 3] = ((r6 - 1.0) / 6.0 + 1.0 / r) - 1.0
    T[:, 4:7] = V
    if D == 3:
        T[:, 7] = y * vz - z * vy
        T[:, 8] = z * vx - x * vz
    T[:, 9] = x * vy - y * vx
    T[:, 10:13] = X
    ext = np.concatenate([[v2.max(), rho.min(), rho.max()], X.min(0), X.max(0)]) if n else None
    return T, ext


def _check_against_download(b, k, d, consts, label):
    """Sample k of the series `b` against the download `d`: n and the extremes exactly, the sums within the module's bars."""
    m0, f_pot, f_int = _factors(consts)
    T, ext = _terms(d, consts.rho0)
    n = len(T)
    assert int(b["count"][k]) == n and n > 0, (int(b["count"][k]), n)
    delivered = np.concatenate([[np.nan], b["energy"][k], b["momentum"][k], b["angular"][k], b["centre"][k]])
    factor = [np.nan, m0, f_pot, f_int] + [m0] * 6 + [None] * 3                     # None: divided by n
    for slot in range(1, 13):
        exact, mag = math.fsum(T[:, slot]), math.fsum(np.abs(T[:, slot]))
        bound = n * EPS * mag + (8.0 * n * EPS if slot == 3 else 0.0)
        want, scale = (exact / n, 1.0 / n) if factor[slot] is None else (factor[slot] * exact, abs(factor[slot]))
        bound = scale * bound + 2.0 * EPS * abs(delivered[slot])
        err = abs(delivered[slot] - want)
        print(f"{label} slot {slot}: device {delivered[slot]:.17g} download {want:.17g} |diff| {err:.3g} bound {bound:.3g}")
        assert err <= bound, (slot, delivered[slot], want, err, bound)
    got = np.concatenate([b["extremes"][k], b["box"][k]])
    want = ext.copy()
    want[0] = np.sqrt(want[0])
    for slot in range(13, 22):
        print(f"{label} slot {slot}: device {got[slot - 13]:.17g} download {want[slot - 13]:.17g}")
    np.testing.assert_array_equal(got, want)
    return T


@pytest.mark.parametrize("fb", [8, 4])
@pytest.mark.parametrize("case", ["dam_break_2d", "moving_square", "dam_break_3d_shipped"])
def test_last_sample_equals_the_download(case, fb, request):
    p, s = _state(case, request)
    K = STEPS[case]
    if case in ROWS:
        assert len(p) == ROWS[case]                              # 26 blocks + 225 rows / 69 blocks: a ragged block, a wrapped final stride
    if case == "moving_square":
        assert set(np.unique(p.Type)) == {1, 2, 3}               # Fixed, Moving and Fluid rows: only Fluid counts
    eng = _engine(p, s, fb)
    eng.budgets_enable(capacity=K + 8)
    pr = eng.advance(1e9, max_steps=K)
    assert pr.iteration == K and pr.n_rebuilds >= 2, pr.n_rebuilds
    b = eng.budgets_read()
    assert len(b["iteration"]) == K and eng.budgets_dropped == 0
    assert b["energy"].shape == (K, 3) and b["box"].shape == (K, 6)
    d = eng.download(FIELDS)
    T = _check_against_download(b, K - 1, d, s.SimConstants, f"{case} fp{8 * fb}")
    assert len(T) == int((p.Type == 1).sum()) < len(p)
    assert b["extremes"][-1, 0] > 0 and b["energy"][-1, 0] > 0 and (b["count"] == len(T)).all()
    if p.Position.shape[1] == 2:
        assert (b["angular"][:, :2] == 0).all() and (b["momentum"][:, 2] == 0).all() and (b["centre"][:, 2] == 0).all()
        assert (b["box"][:, 2] == 0).all() and (b["box"][:, 5] == 0).all()
    # iteration, time and dt of the last sample are the progress block, bit for bit
    assert (int(b["iteration"][-1]), float(b["time"][-1]), float(b["dt"][-1])) == (pr.iteration, pr.total_time, pr.last_dt)
    eng.close()


def test_every_step_is_sampled(request):
    """Sample j of one call of K steps is the last sample of a fresh handle advanced j steps from the same upload."""
    p, s = _state("dam_break_2d", request)
    K = 24
    eng = _engine(p, s, 8)
    eng.budgets_enable(capacity=K)
    eng.advance(1e9, max_steps=K)
    b = eng.budgets_read()
    assert len(b["iteration"]) == K                                # no sample for a cancelled step, none twice for a re-queued one
    np.testing.assert_array_equal(b["iteration"], np.arange(1, K + 1))
    assert (np.diff(b["time"]) > 0).all() and (b["dt"] > 0).all()
    np.testing.assert_array_equal(b["time"][1:], b["time"][:-1] + b["dt"][1:])      # TotalTime += dt, as the control does it
    for j in range(1, K + 1):
        e = _engine(p, s, 8)
        e.budgets_enable(capacity=K)
        q = e.advance(1e9, max_steps=j)
        bj = e.budgets_read()
        assert len(bj["iteration"]) == j
        assert (int(bj["iteration"][-1]), float(bj["time"][-1]), float(bj["dt"][-1])) == (q.iteration, q.total_time, q.last_dt)
        for key in b:
            np.testing.assert_array_equal(bj[key][-1], b[key][j - 1], err_msg=f"{key}, step {j}")
        e.close()
    eng.close()


CHILD = """
import sys
import numpy as np
sys.path[:0] = [{root!r}, {tests!r}]
from conftest import load_dam_break_2d, perturbed
from sphexample_amd.engine import make_engine
p0, s = load_dam_break_2d()
eng = make_engine(perturbed(p0, seed=3, vel_scale=3.0), s, device_float_bytes=4)
eng.budgets_enable(capacity=64)
pr = eng.advance(1e9, max_steps=30)
b = eng.budgets_read()
assert len(b["iteration"]) == 30 == pr.iteration, len(b["iteration"])
np.savez({out!r}, **b)
eng.close()
"""


def test_one_launch_and_two_stages_give_the_same_bits(tmp_path):
    """$SPHMI_BUDGETS_SMALL_ROWS is read at enable: the default threshold, 0 (always two stages) and 8192 (one launch for the 6 881
    rows of this case, whatever the default is), each in a fresh process — the whole series bit for bit; two default runs too."""
    runs = {"default": None, "two_stage": "0", "one_launch": "8192", "default_again": None}
    procs = {}
    for name, rows in runs.items():
        env = {k: v for k, v in os.environ.items() if k != "SPHMI_BUDGETS_SMALL_ROWS"}
        if rows is not None:
            env["SPHMI_BUDGETS_SMALL_ROWS"] = rows
        code = CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), out=str(tmp_path / f"{name}.npz"))
        procs[name] = subprocess.Popen([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    series = {}
    for name, proc in procs.items():
        out, _ = proc.communicate(timeout=300)
        assert proc.returncode == 0, (name, out)
        series[name] = dict(np.load(str(tmp_path / f"{name}.npz")))
    ref = series["default"]
    assert len(ref["iteration"]) == 30 and ref["extremes"][-1, 0] > 0
    for name in ("two_stage", "one_launch", "default_again"):
        for key in ref:
            np.testing.assert_array_equal(series[name][key], ref[key], err_msg=f"{name}: {key}")


def test_closed_form(dam_break_3d_shipped):
    """Three Fluid rows 10 H apart, no boundary row (the engine takes such a handle), rho = rho0, v0 = (0.3, -0.2, 0.5): no row has a
    neighbour, so a = (0, 0, -g) at every step.  p_x, p_y stay; p_z falls linearly; the corrector's x += 1/2 (v_new + v_old) dt
    makes E_kin + E_pot exact for constant a, which pins the sign and the axis of E_pot; rho stays rho0 and E_int = 0."""
    from sphexample_amd import particles_from_arrays
    _, s = dam_break_3d_shipped
    c, H = s.SimConstants, s.SimKernel.H
    pos = np.array([[1.0, 1.0, 1.0]]) + np.arange(3)[:, None] * np.array([[10.0 * H, 0.0, 0.0]])
    p = particles_from_arrays(3, pos, np.full(3, c.rho0), np.ones(3, dtype=np.uint8), np.full(3, 2), np.arange(1, 4))
    v0 = np.array([0.3, -0.2, 0.5])
    p.Velocity[:] = v0
    K = 50
    eng = _engine(p, s, 8)
    eng.budgets_enable(capacity=K)
    pr = eng.advance(1e9, max_steps=K)
    assert pr.iteration == K
    b = eng.budgets_read()
    assert len(b["iteration"]) == K and (b["count"] == 3).all()
    m0, g, t = c.m0, c.g, b["time"]
    assert g > 0
    for axis in (0, 1):
        want = m0 * (3.0 * v0[axis])
        err = np.abs(b["momentum"][:, axis] - want).max()
        print(f"p[{axis}]: |diff| {err:.3g} bound {4 * EPS * abs(want):.3g}")
        assert err <= 4 * EPS * abs(want), (axis, err)
    want = m0 * 3.0 * (v0[2] - g * t)
    bound = 50 * EPS * m0 * 3.0 * (abs(v0[2]) + g * t)
    print(f"p[2]: max |diff| / bound {(np.abs(b['momentum'][:, 2] - want) / bound).max():.3g}")
    assert (np.abs(b["momentum"][:, 2] - want) <= bound).all()
    mech = b["energy"][:, 0] + b["energy"][:, 1]
    scale = (np.abs(b["energy"][:, 0]) + np.abs(b["energy"][:, 1])).max()
    print(f"E_kin + E_pot: spread {mech.max() - mech.min():.3g} bound {200 * EPS * scale:.3g}; E_kin {b['energy'][0, 0]:.6g} -> {b['energy'][-1, 0]:.6g}")
    assert np.abs(mech - mech[0]).max() <= 200 * EPS * scale
    assert b["energy"][-1, 0] != b["energy"][0, 0]                 # the kinetic energy did change: the potential one made up for it
    B = (c.c0 * c.c0 * c.rho0) / 7.0
    print(f"E_int: max {np.abs(b['energy'][:, 2]).max():.3g} bound {8 * 3 * EPS * m0 * B / c.rho0:.3g}")
    assert (np.abs(b["energy"][:, 2]) <= 8 * 3 * EPS * m0 * B / c.rho0).all()
    np.testing.assert_array_equal(b["extremes"][:, 1:], np.full((K, 2), c.rho0))
    eng.close()


def test_slabs_in_one_handle(request):
    """Every slab reduces the rows it owns, the handle combines the slabs' records: sums add, extremes take min or max.  The water
    column straddles the cuts, so a ghost copy that was counted would show in n."""
    p, s = _state("dam_break_3d_shipped", request)
    K = STEPS["dam_break_3d_shipped"]
    dd = _engine(p, s, 4, devices=[0, 0, 0])
    dd.budgets_enable(capacity=K)
    pr = dd.advance(1e9, max_steps=K)
    assert pr.iteration == K and pr.n_rebuilds >= 2
    info = dd.multi_info()
    assert info.world == 3 and info.n_local == 3 and sum(info.n_live[:3]) > len(p)       # ghost copies are held
    b = dd.budgets_read()
    assert len(b["iteration"]) == K
    np.testing.assert_array_equal(b["iteration"], np.arange(1, K + 1))
    d = dd.download(FIELDS + ("Cells",))
    _check_against_download(b, K - 1, d, s.SimConstants, "dam_break_3d_shipped fp32 3 slabs")
    cols = d["Cells"][d["Type"] == 1][:, info.axis]
    assert any(cols.min() < cut <= cols.max() for cut in info.cuts[:2])                   # the Fluid rows lie in more than one slab
    assert (int(b["iteration"][-1]), float(b["time"][-1]), float(b["dt"][-1])) == (pr.iteration, pr.total_time, pr.last_dt)
    dd.close()


def test_contract(request):
    from sphexample_amd._abi import make_config
    from sphexample_amd.engine import Engine, rccl_unique_id
    import ctypes as C
    p, s = _state("dam_break_2d", request)
    # before the upload
    cfg = make_config(len(p), s.SimConstants, s.SimKernel, s.SimMetaData, s.SimViscosity, s.SimDensityDiffusion, device_float_bytes=8, host_float_bytes=8)
    bare = Engine(cfg)
    for call in (lambda: bare.budgets_enable(capacity=4), bare.budgets_read):
        with pytest.raises(SphmiError) as ei:
            call()
        assert ei.value.status == ERR_STATE
    bare.close()
    eng = _engine(p, s, 8)
    # read while disabled; argument errors
    with pytest.raises(SphmiError) as ei:
        eng.budgets_read()
    assert ei.value.status == ERR_STATE
    with pytest.raises(SphmiError) as ei:
        eng.budgets_enable(capacity=-1)
    assert ei.value.status == ERR_ARGUMENT
    eng.budgets_enable(capacity=6)
    read = eng._fn("budgets_read")
    read.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 12
    assert read(eng._h, 1, *[None] * 12) == ERR_ARGUMENT                           # null n_out
    # more steps than capacity_steps between two reads: the newest stay, the oldest are counted
    ref = _engine(p, s, 8)
    ref.budgets_enable(capacity=100)
    eng.advance(1e9, max_steps=50); ref.advance(1e9, max_steps=50)
    b, r = eng.budgets_read(), ref.budgets_read()
    assert len(b["iteration"]) == 6 and eng.budgets_dropped == 44 and len(r["iteration"]) == 50 and ref.budgets_dropped == 0
    for key in b:
        np.testing.assert_array_equal(b[key], r[key][-6:], err_msg=key)
    # read clears
    assert len(eng.budgets_read()["iteration"]) == 0 and eng.budgets_dropped == 0
    # a re-enable drops the series
    eng.advance(1e9, max_steps=3)
    eng.budgets_enable(capacity=8)
    assert len(eng.budgets_read()["iteration"]) == 0
    # sphmi_forces_once adds no sample
    eng.forces_once()
    assert len(eng.budgets_read()["iteration"]) == 0
    # group forces, probes and budgets together: K samples each, the same clock columns
    K = 20
    fluid = p.Position[p.Type == 1]
    eng.budgets_enable(capacity=K)
    eng.group_forces_enable([1, 2], capacity=K)
    eng.probes_enable(fluid.mean(0)[None, :], capacity=K)
    pr = eng.advance(1e9, max_steps=K)
    it, t, dt, F = eng.group_forces_read()
    probes, b = eng.probes_read(), eng.budgets_read()
    assert len(it) == len(probes["iteration"]) == len(b["iteration"]) == K
    for mine, theirs in ((b["iteration"], it), (b["time"], t), (b["dt"], dt)):
        np.testing.assert_array_equal(mine, theirs)
    for key in ("iteration", "time", "dt"):
        np.testing.assert_array_equal(b[key], probes[key])
    assert (int(b["iteration"][-1]), float(b["time"][-1]), float(b["dt"][-1])) == (pr.iteration, pr.total_time, pr.last_dt)
    # capacity_steps = 0 disables
    eng.budgets_enable(capacity=0)
    with pytest.raises(SphmiError) as ei:
        eng.budgets_read()
    assert ei.value.status == ERR_STATE
    # the upload disables
    eng.budgets_enable(capacity=8)
    eng.upload_particles(p)
    with pytest.raises(SphmiError) as ei:
        eng.budgets_read()
    assert ei.value.status == ERR_STATE
    eng.advance(1e9, max_steps=3)
    # rank-mode handles: one slab of the rows per process
    rk = _engine(p, s, 8, rank=0, world=1, unique_id=rccl_unique_id())
    for call in (lambda: rk.budgets_enable(capacity=4), rk.budgets_read):
        with pytest.raises(SphmiError) as ei:
            call()
        assert ei.value.status == ERR_STATE
    for e in (eng, ref, rk):
        e.close()


def test_run_simulation_hands_the_samples_to_the_callback(dam_break_2d):
    import copy
    from sphexample_amd import budgets, simulation
    p, s = dam_break_2d
    meta = copy.deepcopy(s.SimMetaData)
    meta.SimulationTime, meta.OutputTimes = 0.002, 0.001
    got = []
    steps = simulation.RunSimulation(SimGeometry=None, SimMetaData=meta, SimConstants=s.SimConstants, SimKernel=s.SimKernel, SimLogger=None,
                                     SimParticles=p.copy(), SimViscosity=s.SimViscosity, SimDensityDiffusion=s.SimDensityDiffusion,
                                     budgets=True, on_output=lambda m, pp, b: got.append((m.Iteration, m.TotalTime, b)))
    assert len(got) == len(steps) + 1 and len(got[0][2]["iteration"]) == 0
    its = np.concatenate([b["iteration"] for _, _, b in got])
    np.testing.assert_array_equal(its, np.arange(1, got[-1][0] + 1))           # every step of the run, once, in order
    n_fluid = int((p.Type == 1).sum())
    for iteration, time, b in got[1:]:
        assert int(b["iteration"][-1]) == iteration and float(b["time"][-1]) == time and (b["count"] == n_fluid).all()
        assert budgets.total_energy(b).shape == b["time"].shape
        np.testing.assert_array_equal(budgets.front_position(b), b["box"][:, 3])
