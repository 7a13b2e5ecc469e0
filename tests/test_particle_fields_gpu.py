"""Vorticity, velocity divergence, div r, the free-surface normal, the Shepard sum and the neighbour count at the particles
(sphmi_particle_fields, csrc/sphmi_particle_fields.h) — needs a real MI355X.

The reference is `brute_force_particle_fields` of tests/test_particle_fields_host.py: an O(M·N) numpy enumeration in fp64 written
from the definition, pinned there against analysis, fed the Position, Velocity and Density of a download taken right after the
call.  It never calls the code under test.

Bars (the project's bars for a single evaluation, tests/test_probes_gpu.py): every sum within 1e-10 of that field's maximum on fp64
handles and 2e-4 on fp32 handles (over the rows the reference was formed for: with a subset of targets that maximum is at most
the one over all rows, so the check is no wider).

n must be equal at EVERY row, on fp64 and on fp32 handles: no row is excused.  The probes excuse a probe on fp32 handles when the
reference shows a row within 1e-6·H of the cut for it, under a cap of 2 % that the reference alone must keep.  Rows cannot keep
such a cap: the walls of the stock layouts sit on a lattice of spacing dp with H = 4·dp exactly (dam_break_2d), so every wall row —
2 465 of 6 881 — has a neighbour AT the cut for as long as the run lasts.  Nor do they need the excuse: the kernel forms r² from
the very doubles sphmi_download delivers (record + low word on fp32 handles), term by term without contraction, as numpy does, so
a row at the cut is in or out for both.  The number of rows with a neighbour that close is printed with the other figures.

Every test prints its figures before it asserts; profiles/particle_fields.md holds the worst deviation per arithmetic.
"""
import ctypes as C

import numpy as np
import pytest

from test_particle_fields_host import brute_force_particle_fields
from test_probes_gpu import BAR, _engine, _state, _variant

pytestmark = pytest.mark.gpu

STATE = ("Position", "Velocity", "Density", "Type")
SUMS = {"S": "shepard", "N": "normal", "div_r": "div_r", "div_v": "div_v", "w": "vorticity"}


def _check(eng, fb, what, targets=None, got=None):
    """One call against the enumeration on the download taken right after it; prints every figure before it asserts."""
    got = got or eng.particle_fields()
    d = eng.download(STATE)
    ref = brute_force_particle_fields(eng.cfg, d["Position"], d["Velocity"], d["Density"], targets)
    rows = slice(None) if targets is None else np.asarray(targets)
    M = len(ref["n"])
    tol = BAR[fb]
    figures = {}
    for q, name in SUMS.items():
        scale = np.abs(ref[q]).max()
        figures[name] = np.abs(got[name][rows] - ref[q]).max() / scale if scale > 0 else np.abs(got[name][rows]).max()
    differ = got["count"][rows] != ref["n"]
    print(f"{what} fp{8 * fb}: {M} rows of {len(d['Type'])}, n differs at {int(differ.sum())}, near the cut {int(ref['near'].sum())}; "
          + ", ".join(f"{q} {v:.3g}" for q, v in figures.items()) + f" (bar {tol:g})")
    assert not differ.any(), np.flatnonzero(differ)                                 # fp32 handles too: nothing is excused (module docstring)
    for q, v in figures.items():
        assert v <= tol, (what, q, v, tol)
    if d["Position"].shape[1] == 2:
        assert (got["vorticity"][:, :2] == 0).all() and (got["normal"][:, 2] == 0).all()      # exact zeros
    return got, ref, d


# ---- 1. equals the enumeration ------------------------------------------------------------------------------------------------
CASES = {  # name → (fixture, steps, kernel variant, targets: None = all rows)
    "dam_break_2d": ("dam_break_2d", 30, None, None),
    "dam_break_3d_shipped": ("dam_break_3d_shipped", 12, None, 2048),
    "moving_square": ("moving_square", 25, None, None),
    "cubic_spline": ("dam_break_2d", 20, "cubic", None),
}


@pytest.mark.parametrize("fb", [8, 4])
@pytest.mark.parametrize("case", list(CASES))
def test_equals_the_enumeration(case, fb, request):
    fixture, K, kernel, subset = CASES[case]
    p, s = _state(fixture, request)
    if kernel:
        s = _variant(s, kernel, None)
    eng = _engine(p, s, fb)
    assert eng.advance(1e9, max_steps=K).iteration == K
    targets = None if subset is None else np.sort(np.random.default_rng(17).choice(len(p), subset, replace=False))
    got, ref, d = _check(eng, fb, case, targets)
    assert all(got[k].shape == ((len(p), 3) if k in ("normal", "vorticity") else (len(p),)) for k in got)
    assert (got["count"] > 0).sum() > len(p) // 2
    assert (got["count"][d["Type"] == 2] > 0).any()                                # walls are targets and neighbours like any row
    if fixture == "moving_square":
        assert eng.cfg.H < 2 * eng.cfg.h and (got["count"][d["Type"] == 3] > 0).any()      # k < 2: five candidate cells per axis; Moving rows
    assert np.abs(got["vorticity"]).max() > 0
    # a subset of the fields is the same numbers
    part = eng.particle_fields(fields=("div_r", "count"))
    assert set(part) == {"div_r", "count"}
    np.testing.assert_array_equal(part["div_r"], got["div_r"]); np.testing.assert_array_equal(part["count"], got["count"])
    eng.close()


# ---- 2. stale lists ---------------------------------------------------------------------------------------------------------------
def test_stale_lists(request):
    """A call at least 15 steps behind the last rebuild — rows have drifted out of the cell `cstart` files them under — and a call
    directly behind one.  n_rebuilds of a fresh handle stopped after j steps, for every j, tells where the rebuilds of the run are."""
    for vel in (1.0, 0.3):                                                         # slower particles: longer stretches between rebuilds
        p, s = _state("dam_break_2d", request, vel=vel)
        K = 64
        history = []
        for j in range(1, K + 1):
            eng = _engine(p, s, 8)
            history.append(eng.advance(1e9, max_steps=j).n_rebuilds)
            eng.close()
        rebuilt_before = [1] + [j for j in range(2, K + 1) if history[j - 1] > history[j - 2]]
        since = [j - max(b for b in rebuilt_before if b <= j) for j in range(1, K + 1)]      # steps executed after the last rebuild, less one
        print(f"vel {vel}: rebuilds before steps {rebuilt_before}; longest stretch without one {max(since) + 1} steps")
        if max(since) >= 15:
            break
    assert max(since) >= 15, "no step of the run lies 15 steps behind the last rebuild"
    far = 1 + int(np.argmax(since))
    eng = _engine(p, s, 8)
    pr = eng.advance(1e9, max_steps=far)
    assert pr.n_rebuilds == history[far - 1]
    _check(eng, 8, f"step {far}, {since[far - 1] + 1} steps behind the last rebuild")
    before = pr.n_rebuilds
    pr = eng.advance(1e9, max_steps=1)                                             # every sphmi_advance opens with a rebuild
    assert pr.n_rebuilds == before + 1
    _check(eng, 8, "one step behind a rebuild")
    eng.close()


# ---- 3. the same bits, no side effects ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fb", [8, 4])
def test_repeats_and_does_not_disturb(fb, request):
    p, s = _state("dam_break_2d", request)
    markers = sorted(int(m) for m in np.unique(p.GroupMarker))
    F = p.Position[p.Type == 1]
    probes = np.array([F.mean(0), F.min(0) + 0.05, F.max(0) - 0.05])
    runs = []
    for called in (False, True):
        eng = _engine(p, s, fb)
        eng.group_forces_enable(markers, capacity=64)
        eng.probes_enable(probes, capacity=64)
        prog = []
        for _ in range(8):
            q = eng.advance(1e9, max_steps=5)
            prog.append((q.iteration, q.steps_done, q.n_rebuilds, q.index_counter, q.total_time, q.last_dt, q.delta_x))
            if called:
                a, b = eng.particle_fields(), eng.particle_fields()                # no step in between: the same bytes
                for k in a:
                    assert a[k].tobytes() == b[k].tobytes(), k
        runs.append((prog, eng.download(), eng.group_forces_read(), eng.probes_read()))
        if called:
            # a download begun before the call completes with the snapshot taken at its begin
            want = eng.download()
            spec = {k: np.zeros_like(want[k]) for k in ("Position", "Velocity", "Acceleration", "Density", "Pressure", "ID", "Type", "GroupMarker", "GhostPoints", "Cells")}
            fbeg = eng._fn("download_begin"); fbeg.argtypes = [C.c_void_p] * 11
            eng._check(fbeg(eng._h, *[spec[k].ctypes.data_as(C.c_void_p) for k in spec]))
            mid = eng.particle_fields()
            eng.download_end()
            for k in spec:
                np.testing.assert_array_equal(spec[k], want[k], err_msg=k)
            for k in mid:
                assert mid[k].tobytes() == a[k].tobytes(), k
        eng.close()
    assert runs[0][0][-1][0] == 40 and runs[0][0] == runs[1][0]                    # the progress blocks, n_rebuilds among them
    for k, v in runs[0][1].items():
        assert runs[1][1][k].tobytes() == v.tobytes(), k                            # the final download, byte for byte
    for a, b in zip(runs[0][2], runs[1][2]):
        np.testing.assert_array_equal(a, b)                                         # the group-force series
    assert len(runs[0][3]["iteration"]) == 40
    for k in runs[0][3]:
        np.testing.assert_array_equal(runs[1][3][k], runs[0][3][k], err_msg=k)      # the probe series


# ---- 4. tile edges ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fb", [8, 4])
@pytest.mark.parametrize("rows", [1, 255, 256, 257, 513])
def test_tile_edges(rows, fb, request):
    """The first `rows` rows of dam_break_2d as a cloud of their own (with velocities on every row, so that every sum has
    something to add): one row, one short of a tile of 256, a tile, a tile and a row, two tiles and a row."""
    from sphexample_amd.preprocess import FIELD_NAMES, SimParticles
    p0, s = request.getfixturevalue("dam_break_2d")
    assert len(p0) > rows
    p = SimParticles(p0.Dimensions, p0.FloatType, **{k: np.ascontiguousarray(getattr(p0, k)[:rows]).copy() for k in FIELD_NAMES})
    p.Velocity[...] = np.random.default_rng(23).uniform(-1.0, 1.0, p.Velocity.shape)
    eng = _engine(p, s, fb)
    assert eng.advance(1e9, max_steps=1).iteration == 1
    got, ref, d = _check(eng, fb, f"{rows} rows")
    assert all(len(got[k]) == rows for k in got)
    if rows == 1:
        cfg = eng.cfg
        assert got["count"][0] == 0
        assert got["shepard"][0] == pytest.approx((cfg.m0 / float(d["Density"][0])) * cfg.alphaD, rel=1e-15 if fb == 8 else 1e-12)      # V·W(0)
        for k in ("normal", "div_r", "div_v", "vorticity"):
            assert (got[k] == 0).all(), k
    else:
        assert (got["count"] > 0).any()
    eng.close()


# ---- 5. errors ------------------------------------------------------------------------------------------------------------------------
def test_errors(request):
    from sphexample_amd._abi import ERR_STATE, SphmiError, make_config
    from sphexample_amd.engine import Engine
    p, s = _state("dam_break_2d", request)

    def refused(eng, word):
        with pytest.raises(SphmiError) as ei:
            eng.particle_fields()
        assert ei.value.status == ERR_STATE and word in str(ei.value), str(ei.value)

    cfg = make_config(len(p), s.SimConstants, s.SimKernel, s.SimMetaData, s.SimViscosity, s.SimDensityDiffusion, device_float_bytes=8, host_float_bytes=8)
    bare = Engine(cfg)
    refused(bare, "before sphmi_upload")
    bare.upload_particles(p)
    refused(bare, "has not executed a step")                                       # uploaded, no step yet: no cell list
    assert bare.advance(1e9, max_steps=3).iteration == 3                            # the handle still advances …
    assert bare.particle_fields(fields=()) == {}                                   # … and serves: all outputs NULL is legal
    assert (bare.particle_fields(fields=("count",))["count"] > 0).any()
    bare.upload_particles(p)                                                       # a new particle set: refused until a step has run
    refused(bare, "has not executed a step")
    assert bare.advance(1e9, max_steps=1).steps_done == 1
    bare.close()
    slabs = _engine(p, s, 8, devices=[0, 0])                                       # two slabs on one GPU
    refused(slabs, "single-device")
    slabs.advance(1e9, max_steps=3)
    refused(slabs, "single-device")                                                # … with a cell list too
    assert slabs.advance(1e9, max_steps=2).steps_done == 2
    slabs.close()
    thin = _engine(p, _variant(s, None, 0.9), 8)                                   # H < h
    refused(thin, "H < h")
    assert thin.advance(1e9, max_steps=2).steps_done == 2
    thin.close()
