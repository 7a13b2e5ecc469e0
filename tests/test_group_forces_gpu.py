"""The per-step force on particle groups recorded on the device (sphmi_group_forces_enable / sphmi_group_forces_read,
csrc/sphmi_group_forces.h) — needs a real MI355X.

    F_g = m0 * sum of Acceleration[i] over the rows with GroupMarker[i] == g, after every executed step, summed in fp64.

The stock layouts start at rest and do not ask for a cell-list rebuild within a test's horizon: like
test_engine_gpu.py::test_device_side_rebuild_is_the_host_side_rebuild the cases run from `perturbed(p, seed=3, vel_scale=3.0)`,
which crosses Δx-triggered rebuilds within tens of steps (asserted from sphmi_progress.n_rebuilds).

Bars
  * against the download of the same handle: the device and the test add the SAME fp64 values (fp32 handles: the fp32 values
    widened) in a different order — n_g * 2^-52 * m0 * sum|a_i| per component.
  * against the oracle: a sum of n values each within eps * max|a| is within n * eps * max|a|; eps is the acceleration bar of
    test_engine_gpu.py::test_k_step_parity for the same cases and step counts on fp64 handles (1e-8 of the field maximum) and
    DESIGN.md section 6's force bar on fp32 handles (2e-4 of the field maximum).
  * action = reaction: tests/test_oracle.py::test_conservation_properties (fp64, 1e-9) and
    test_engine_gpu.py::test_full_size_properties (fp32, 2e-5), relative to m0 * sum_i |a_i|.  The gravity term of a row is
    g * GravityFactor (src/PreProcess.jl:78-87: Fluid -1, Moving +1, Fixed 0), so the forces of all groups add up to
    m0 * g * (N_moving - N_fluid) along the gravity axis: m0 * g * N_fluid downwards on the dam breaks.
"""
import math

import numpy as np
import pytest

from conftest import perturbed
from sphexample_amd._abi import ERR_ARGUMENT, ERR_STATE, SphmiError

pytestmark = pytest.mark.gpu

# case → steps of one call that cross at least one Δx-triggered rebuild from the perturbed state
STEPS = {"dam_break_2d": 100, "moving_square": 40, "dam_break_3d_shipped": 30}


def _state(case, request, vel=3.0):
    p0, s = request.getfixturevalue(case)
    p = perturbed(p0, seed=3, vel_scale=vel)
    if hasattr(p0, "geometries"):
        p.geometries = p0.geometries
    return p, s


def _engine(p, s, fb, **kw):
    from sphexample_amd.engine import make_engine
    return make_engine(p, s, device_float_bytes=fb, **kw)


def _markers(p):
    return sorted(int(m) for m in np.unique(p.GroupMarker))


def _sums(d, markers, m0):
    """Per group: m0 * fsum(a) per component, sum|a| per component, rows — from a download."""
    a = d["Acceleration"].astype(np.float64)
    D = a.shape[1]
    exp = np.zeros((len(markers), 3)); mag = np.zeros((len(markers), 3)); rows = np.zeros(len(markers), dtype=np.int64)
    for k, g in enumerate(markers):
        sel = a[d["GroupMarker"] == g]
        rows[k] = len(sel)
        for c in range(D):
            exp[k, c] = m0 * math.fsum(sel[:, c])
            mag[k, c] = math.fsum(np.abs(sel[:, c]))
    return exp, mag, rows


@pytest.mark.parametrize("fb", [8, 4])
@pytest.mark.parametrize("case", ["dam_break_2d", "moving_square", "dam_break_3d_shipped"])
def test_last_sample_equals_the_download(case, fb, request):
    p, s = _state(case, request)
    K, markers, m0 = STEPS[case], _markers(p), s.SimConstants.m0
    if case == "moving_square":
        assert markers == [1, 2, 3] and set(np.unique(p.Type)) == {1, 2, 3}          # Fixed, Moving and Fluid groups
    eng = _engine(p, s, fb)
    eng.group_forces_enable(markers, capacity=K + 8)
    pr = eng.advance(1e9, max_steps=K)
    assert pr.iteration == K and pr.n_rebuilds >= 2, pr.n_rebuilds                   # the opening rebuild + a Δx-triggered one
    it, t, dt, F = eng.group_forces_read()
    assert len(it) == K and F.shape == (K, len(markers), 3) and eng.group_forces_dropped == 0
    d = eng.download(("Acceleration", "GroupMarker"))
    exp, mag, rows = _sums(d, markers, m0)
    assert rows.sum() == len(p) and (rows > 0).all()
    for k in range(len(markers)):
        for c in range(3):
            bound = rows[k] * 2.0 ** -52 * m0 * mag[k, c]
            err = abs(F[-1, k, c] - exp[k, c])
            print(f"{case} fp{8 * fb} group {markers[k]} component {c}: F {F[-1, k, c]:.17g} download {exp[k, c]:.17g} |diff| {err:.3g} bound {bound:.3g}")
            assert err <= bound, (markers[k], c, err, bound)
    assert np.abs(F[-1]).max() > 0
    if p.Position.shape[1] == 2:
        assert (F[:, :, 2] == 0).all()
    # iteration, time and dt of the last sample are the progress block, bit for bit
    assert (int(it[-1]), float(t[-1]), float(dt[-1])) == (pr.iteration, pr.total_time, pr.last_dt)


def test_every_step_is_sampled(request):
    """Sample j of one call of K steps is the last sample of a fresh handle advanced j steps from the same upload — one call with
    max_steps = j executes the first j steps of the call with max_steps = K — at a size where rebuilds cut the batches."""
    p, s = _state("dam_break_2d", request)
    K, markers = 80, _markers(p)
    eng = _engine(p, s, 8)
    eng.group_forces_enable(markers, capacity=K)
    pr = eng.advance(1e9, max_steps=K)
    assert pr.n_rebuilds >= 2
    it, t, dt, F = eng.group_forces_read()
    assert len(it) == K                                            # no sample for a cancelled step, none twice for a re-queued one
    np.testing.assert_array_equal(it, np.arange(1, K + 1))
    assert (np.diff(t) > 0).all() and (dt > 0).all()
    np.testing.assert_array_equal(t[1:], t[:-1] + dt[1:])          # TotalTime += dt, as the control does it
    for j in range(1, K + 1):
        e = _engine(p, s, 8)
        e.group_forces_enable(markers, capacity=K)
        q = e.advance(1e9, max_steps=j)
        ij, tj, dj, Fj = e.group_forces_read()
        assert len(ij) == j and (int(ij[-1]), float(tj[-1]), float(dj[-1])) == (q.iteration, q.total_time, q.last_dt)
        assert (int(ij[-1]), float(tj[-1]), float(dj[-1])) == (int(it[j - 1]), float(t[j - 1]), float(dt[j - 1])), j
        np.testing.assert_array_equal(Fj[-1], F[j - 1], err_msg=f"step {j}")
        e.close()


@pytest.mark.parametrize("fb,eps", [(8, 1e-8), (4, 2e-4)])
@pytest.mark.parametrize("case,steps", [("dam_break_2d", 40), ("dam_break_3d_shipped", 25)])
def test_last_sample_against_the_oracle(case, steps, fb, eps, request):
    """The cases and step counts of test_engine_gpu.py::test_k_step_parity (the stock layouts as they are)."""
    from oracle.oracle import make_oracle
    p, s = request.getfixturevalue(case)
    markers, m0 = _markers(p), s.SimConstants.m0
    eng, orc = _engine(p, s, fb), make_oracle(p, s)
    eng.group_forces_enable(markers, capacity=steps)
    pe, po = eng.advance(1e9, max_steps=steps), orc.advance(1e9, max_steps=steps)
    assert pe.iteration == po.iteration == steps and pe.n_rebuilds == po.n_rebuilds
    F = eng.group_forces_read()[3]
    o = orc.download(("Acceleration", "GroupMarker"))
    exp, _, rows = _sums(o, markers, m0)
    amax = np.abs(o["Acceleration"]).max()
    for k in range(len(markers)):
        bound = rows[k] * eps * amax * m0
        err = np.abs(F[-1, k] - exp[k]).max()
        print(f"{case} fp{8 * fb} group {markers[k]}: |F - oracle| {err:.3g} bound {bound:.3g}")
        assert err <= bound, (markers[k], err, bound)


@pytest.mark.parametrize("fb,tol", [(8, 1e-9), (4, 2e-5)])
@pytest.mark.parametrize("case", ["dam_break_2d", "moving_square", "dam_break_3d_shipped"])
def test_action_equals_reaction(case, fb, tol, request):
    p, s = _state(case, request)
    K, markers, m0, g = 12, _markers(p), s.SimConstants.m0, s.SimConstants.g
    eng = _engine(p, s, fb)
    eng.group_forces_enable(markers, capacity=K)
    eng.advance(1e9, max_steps=K)
    F = eng.group_forces_read()[3]
    d = eng.download(("Acceleration",))
    scale = m0 * np.abs(d["Acceleration"].astype(np.float64)).sum()
    D = p.Position.shape[1]
    n_fluid, n_moving = int((p.Type == 1).sum()), int((p.Type == 3).sum())
    if case != "moving_square":
        assert n_moving == 0
    total = F[-1].sum(0)
    want = np.zeros(3)
    want[D - 1] = m0 * g * (n_moving - n_fluid)                    # GravityFactor: Fluid -1, Moving +1 (src/PreProcess.jl:78-87)
    print(f"{case} fp{8 * fb}: sum of the groups {total}, gravity {want[D - 1]:.17g}, scale {scale:.6g}")
    assert np.abs(total - want).max() <= tol * scale, (total, want, scale)


@pytest.mark.parametrize("case,fb", [("dam_break_2d", 4), ("dam_break_2d", 8), ("dam_break_3d_shipped", 4), ("still_wedge", 8)])
def test_sampling_does_not_disturb_the_run(case, fb, request):
    p, s = _state(case, request)
    K, markers = 100, _markers(p)
    runs = []
    for sampled in (False, True, True):
        eng = _engine(p, s, fb)
        if sampled:
            eng.group_forces_enable(markers, capacity=K)
        prs = [eng.advance(1e9, max_steps=n) for n in (K - 7, 7)]
        prog = [(q.iteration, q.steps_done, q.n_rebuilds, q.index_counter, q.total_time, q.last_dt, q.delta_x) for q in prs]
        runs.append((prog, eng.download(), eng.group_forces_read() if sampled else None))
        eng.close()
    assert runs[0][0][-1][2] >= 3
    assert runs[0][0] == runs[1][0] == runs[2][0]
    for k, v in runs[0][1].items():
        np.testing.assert_array_equal(runs[1][1][k], v, err_msg=k)
    assert len(runs[1][2][0]) == K
    for a, b in zip(runs[1][2], runs[2][2]):
        np.testing.assert_array_equal(a, b)                        # two sampled runs: the same bits


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("case,fb,axis", [("dam_break_2d", 8, 0), ("dam_break_2d", 4, 0), ("dam_break_3d_shipped", 8, None)])
def test_slabs_in_one_handle(case, fb, axis, world, request):
    """Every slab sums the rows it owns, the handle adds the slabs' records.  Both groups straddle every cut (the tank's bottom and
    the water column span x), so a ghost copy that was counted would show as a surplus of its whole acceleration."""
    p, s = _state(case, request)
    K, markers, m0 = STEPS[case], _markers(p), s.SimConstants.m0          # (the 2-D dam break needs its 100 steps to cross a Δx-triggered rebuild)
    ref = _engine(p, s, fb)
    dd = _engine(p, s, fb, devices=[0] * world, slab_axis=axis)
    for e in (ref, dd):
        e.group_forces_enable(markers, capacity=K)
    pr, pd = ref.advance(1e9, max_steps=K), dd.advance(1e9, max_steps=K)
    assert (pd.iteration, pd.steps_done, pd.n_rebuilds) == (pr.iteration, pr.steps_done, pr.n_rebuilds) and pr.n_rebuilds >= 2
    info = dd.multi_info()
    assert info.world == world and info.n_local == world
    assert sum(info.n_live[:world]) > len(p)                       # ghost copies are held …
    r = ref.download(("ID", "Cells", "Density", "Position", "Acceleration", "GroupMarker"))
    d = dd.download(("ID", "Cells", "Density", "Position", "Acceleration", "GroupMarker"))
    np.testing.assert_array_equal(d["ID"], r["ID"])
    np.testing.assert_array_equal(d["Cells"], r["Cells"])
    tol = 1e-9 if fb == 8 else 1e-5
    assert np.abs(d["Density"] - r["Density"]).max() / np.abs(r["Density"]).max() < tol
    assert np.abs(d["Position"] - r["Position"]).max() / np.abs(r["Position"]).max() < tol
    # … and each group straddles a cut: its rows lie in more than one slab's cell columns
    ax = info.axis
    for g in markers:
        cols = d["Cells"][d["GroupMarker"] == g][:, ax]
        assert any(cols.min() < c <= cols.max() for c in info.cuts[:world - 1]), g
    ir, tr, dr, Fr = ref.group_forces_read()
    id_, td, dd_, Fd = dd.group_forces_read()
    np.testing.assert_array_equal(id_, ir)
    assert len(id_) == K
    np.testing.assert_allclose(td, tr, rtol=1e-12 if fb == 8 else 1e-6)
    # the slab run's own download is what its last sample must add up to (the bound of the download test, once per slab sum) …
    exp, mag, rows = _sums(d, markers, m0)
    bit_equal = np.array_equal(d["Acceleration"], r["Acceleration"])
    amax = np.abs(r["Acceleration"]).max()
    for k in range(len(markers)):
        for c in range(3):
            own = world * rows[k] * 2.0 ** -52 * m0 * mag[k, c]
            assert abs(Fd[-1, k, c] - exp[k, c]) <= own, (markers[k], c)
            # … and the one-device series: summation order only when the accelerations are bit-equal, else the slab tests' bar
            bound = own if bit_equal else tol * rows[k] * m0 * amax
            err = abs(Fd[-1, k, c] - Fr[-1, k, c])
            print(f"{case} fp{8 * fb} {world} slabs group {markers[k]} component {c}: |slabs - one device| {err:.3g} bound {bound:.3g} bit-equal accelerations {bit_equal}")
            assert err <= bound, (markers[k], c, err, bound)
    # every step of the series, at the slab tests' bar
    for k in range(len(markers)):
        assert np.abs(Fd[:, k] - Fr[:, k]).max() <= tol * rows[k] * m0 * max(amax, np.abs(Fr[:, k]).max() / (rows[k] * m0)), markers[k]


def test_edges(dam_break_2d, request):
    from sphexample_amd._abi import make_config
    from sphexample_amd.engine import Engine, rccl_unique_id
    p, s = _state("dam_break_2d", request)
    # before the upload
    cfg = make_config(len(p), s.SimConstants, s.SimKernel, s.SimMetaData, s.SimViscosity, s.SimDensityDiffusion, device_float_bytes=8, host_float_bytes=8)
    bare = Engine(cfg)
    for call in (lambda: bare.group_forces_enable([1], capacity=4), bare.group_forces_read):
        with pytest.raises(SphmiError) as ei:
            call()
        assert ei.value.status == ERR_STATE
    bare.close()
    eng = _engine(p, s, 8)
    # read while disabled; argument errors
    with pytest.raises(SphmiError) as ei:
        eng.group_forces_read()
    assert ei.value.status == ERR_STATE
    for bad in ([1, 2, 1], list(range(17))):
        with pytest.raises(SphmiError) as ei:
            eng.group_forces_enable(bad, capacity=4)
        assert ei.value.status == ERR_ARGUMENT
    eng._fn("group_forces_enable").argtypes = None
    import ctypes as C
    assert eng._fn("group_forces_enable")(eng._h, C.c_int32(2), None, C.c_int64(4)) == ERR_ARGUMENT      # null table
    # a marker no particle carries: zeros; the others are what they are without it
    eng.group_forces_enable([1, 77, 2], capacity=100)
    eng.advance(1e9, max_steps=5)
    it, t, dt, F = eng.group_forces_read()
    assert len(it) == 5 and (F[:, 1] == 0).all() and np.abs(F[:, 0]).max() > 0 and np.abs(F[:, 2]).max() > 0
    # read clears
    assert len(eng.group_forces_read()[0]) == 0
    # more steps than capacity between two reads: the newest stay, the oldest are counted
    eng.group_forces_enable([1, 2], capacity=6)
    ref = _engine(p, s, 8)
    ref.group_forces_enable([1, 2], capacity=100)
    for e in (eng, ref):
        e.advance(1e9, max_steps=5)                                # (both handles have done the five steps above or do them now)
    ref.advance(1e9, max_steps=5); ref.group_forces_read()
    eng.advance(1e9, max_steps=45); ref.advance(1e9, max_steps=45)
    it, t, dt, F = eng.group_forces_read()
    ir, tr, dr, Fr = ref.group_forces_read()
    assert eng.group_forces_dropped == 50 - 6 and len(it) == 6 and len(ir) == 45
    np.testing.assert_array_equal(it, ir[-6:]); np.testing.assert_array_equal(F, Fr[-6:]); np.testing.assert_array_equal(t, tr[-6:])
    eng.advance(1e9, max_steps=2)
    assert len(eng.group_forces_read()[0]) == 2 and eng.group_forces_dropped == 0
    # n_groups = 0 disables and drops the series
    eng.advance(1e9, max_steps=2)
    eng.group_forces_enable([], capacity=1)
    with pytest.raises(SphmiError) as ei:
        eng.group_forces_read()
    assert ei.value.status == ERR_STATE
    # sphmi_forces_once records nothing
    eng.group_forces_enable([1, 2], capacity=8)
    eng.forces_once()
    assert len(eng.group_forces_read()[0]) == 0
    # the upload disables
    eng.upload_particles(p)
    with pytest.raises(SphmiError) as ei:
        eng.group_forces_read()
    assert ei.value.status == ERR_STATE
    eng.advance(1e9, max_steps=3)
    # rank-mode handles: one slab of the rows per process
    rk = _engine(p, s, 8, rank=0, world=1, unique_id=rccl_unique_id())
    for call in (lambda: rk.group_forces_enable([1], capacity=4), rk.group_forces_read):
        with pytest.raises(SphmiError) as ei:
            call()
        assert ei.value.status == ERR_STATE
    for e in (eng, ref, rk):
        e.close()


@pytest.mark.parametrize("case,steps", [("duckling", 12), ("still_wedge", 40), ("moving_square", 30)])
def test_handles_whose_control_is_a_launch_of_its_own(case, steps, request):
    """mDBC and moving-body handles (fp64 by the library's policy): the sample follows the corrector of the same control block."""
    p, s = _state(case, request, vel=1.0)
    markers, m0 = _markers(p), s.SimConstants.m0
    eng = _engine(p, s, 0)
    eng.group_forces_enable(markers, capacity=steps)
    pr = eng.advance(1e9, max_steps=steps)
    it, t, dt, F = eng.group_forces_read()
    assert len(it) == steps == pr.iteration and (int(it[-1]), float(t[-1]), float(dt[-1])) == (pr.iteration, pr.total_time, pr.last_dt)
    exp, mag, rows = _sums(eng.download(("Acceleration", "GroupMarker")), markers, m0)
    for k in range(len(markers)):
        for c in range(3):
            assert abs(F[-1, k, c] - exp[k, c]) <= rows[k] * 2.0 ** -52 * m0 * mag[k, c], (markers[k], c)


def test_run_simulation_hands_the_samples_to_the_callback(dam_break_2d):
    import copy
    from sphexample_amd import simulation
    p, s = dam_break_2d
    meta = copy.deepcopy(s.SimMetaData)
    meta.SimulationTime, meta.OutputTimes = 0.002, 0.001
    got = []
    steps = simulation.RunSimulation(SimGeometry=None, SimMetaData=meta, SimConstants=s.SimConstants, SimKernel=s.SimKernel, SimLogger=None,
                                     SimParticles=p.copy(), SimViscosity=s.SimViscosity, SimDensityDiffusion=s.SimDensityDiffusion,
                                     group_forces=[1, 2], on_output=lambda m, pp, f: got.append((m.Iteration, m.TotalTime, f)))
    assert len(got) == len(steps) + 1 and len(got[0][2][0]) == 0
    its = np.concatenate([f[0] for _, _, f in got])
    np.testing.assert_array_equal(its, np.arange(1, got[-1][0] + 1))           # every step of the run, once, in order
    for iteration, time, f in got[1:]:
        assert f[3].shape[1:] == (2, 3) and int(f[0][-1]) == iteration and float(f[1][-1]) == time
