"""The neighbour list of every row in CSR form, built on the device (sphmi_neighbors_build / _read / _release,
csrc/sphmi_neighbor_list.h) — needs a real MI355X.

The reference is `brute_force_neighbors` of tests/test_neighbor_list_host.py: an O(M·N) numpy enumeration with
r^2 = ((dx^2 + dy^2) + dz^2) <= H^2 on the Position of a download taken right after the build, pinned there on a regular lattice.
It never calls the code under test.  Offsets and entries must be EQUAL to it, on fp64 and on fp32 handles, at every row: the
kernel forms r^2 from the very doubles sphmi_download delivers, term by term without contraction, so a row at the cut is in or
out for both (tests/test_particle_fields_gpu.py shows the same cut reproducible on fp32 handles).

Not tested here: offsets beyond 2^31 (more than 10^7 rows; the 64-bit scan is reviewed, not exercised) and SPHMI_ERR_DEVICE (an
arena the device cannot hold needs as many rows).
"""
import ctypes as C

import numpy as np
import pytest

from sphexample_amd import neighbors
from sphexample_amd._abi import ERR_ARGUMENT, ERR_STATE, SphmiError
from test_neighbor_list_host import brute_force_neighbors
from test_probes_gpu import BAR, _engine, _state, _variant, kernel_w

pytestmark = pytest.mark.gpu


def _check(eng, what, targets=None, half_too=True):
    """One build against the enumeration on the download taken right after it; prints its figures before it asserts.  Returns
    (offsets, neighbors, download)."""
    n_rows, n_pairs = eng.neighbors_build()
    off, nbr = eng.neighbors_read()
    d = eng.download(("Position", "Density", "Type"))
    N = len(d["Type"])
    cnt = np.diff(off)
    print(f"{what}: {N} rows, {n_pairs} pairs, mean {n_pairs / N:.1f}, longest row {int(cnt.max())}, empty rows {int((cnt == 0).sum())}")
    assert n_rows == N and off.shape == (N + 1,) and off.dtype == np.int64 and nbr.dtype == np.int32
    assert off[0] == 0 and off[-1] == len(nbr) == n_pairs and (cnt >= 0).all()
    assert nbr.min(initial=0) >= 0 and nbr.max(initial=0) < N
    i, j = neighbors.pairs(off, nbr)
    inner = np.ones(len(nbr), bool)
    inner[off[:-1][cnt > 0]] = False                                                # not the first entry of a row
    assert (np.diff(nbr.astype(np.int64), prepend=-1)[inner] > 0).all()             # every row strictly ascending
    assert (i != j).all()
    ref_off, ref_nbr = brute_force_neighbors(eng.cfg, d["Position"], targets)
    if targets is None:
        np.testing.assert_array_equal(off, ref_off)
        np.testing.assert_array_equal(nbr, ref_nbr)
    else:
        t = np.asarray(targets)
        np.testing.assert_array_equal(cnt[t], np.diff(ref_off))
        take = np.concatenate([np.arange(off[r], off[r + 1]) for r in t]) if len(t) else np.zeros(0, np.int64)
        np.testing.assert_array_equal(nbr[take], ref_nbr)
    assert neighbors.symmetric(off, nbr)                                            # over ALL rows: the ones outside `targets` too
    np.testing.assert_array_equal(cnt, eng.particle_fields(("count",))["count"])
    if half_too:
        rows_h, pairs_h = eng.neighbors_build(half=True)
        off_h, nbr_h = eng.neighbors_read()
        assert rows_h == N and 2 * pairs_h == n_pairs
        np.testing.assert_array_equal(nbr_h, nbr[j > i])
        np.testing.assert_array_equal(np.diff(off_h), np.bincount(i[j > i], minlength=N))
        assert off_h[0] == 0 and off_h[-1] == pairs_h
    eng.neighbors_release()
    return off, nbr, d


# ---- 1. equals the enumeration ------------------------------------------------------------------------------------------------
CASES = {  # name → (fixture, steps, kernel variant, targets: None = all rows)
    "dam_break_2d": ("dam_break_2d", 30, None, None),
    "moving_square": ("moving_square", 25, None, None),
    "cubic_spline": ("dam_break_2d", 20, "cubic", None),
    "dam_break_3d_shipped": ("dam_break_3d_shipped", 12, None, 4096),
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
    if fixture == "dam_break_2d":
        assert len(p) == 6881
    if fixture == "dam_break_3d_shipped":
        assert len(p) == 17446
    if fixture == "moving_square":
        assert eng.cfg.H < 2 * eng.cfg.h                                            # k < 2: five candidate cells per axis
    targets = None if subset is None else np.sort(np.random.default_rng(17).choice(len(p), subset, replace=False))
    off, nbr, d = _check(eng, f"{case} fp{8 * fb}", targets)
    assert (np.diff(off) > 0).sum() > len(p) // 2
    # neighbor_list(): build, read and release in one call — the same arrays, and nothing is held afterwards
    off2, nbr2 = eng.neighbor_list()
    assert off2.tobytes() == off.tobytes() and nbr2.tobytes() == nbr.tobytes()
    with pytest.raises(SphmiError):
        eng.neighbors_read()
    eng.close()


# ---- 2. a user pair term ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fb", [8, 4])
def test_a_user_pair_term_reproduces_the_shepard_sum(fb, request):
    """S_i = V_i W(0) + sum_j V_j W_ij formed with numpy from the list and one download: the library's own Shepard sum."""
    p, s = _state("dam_break_2d", request)
    eng = _engine(p, s, fb)
    assert eng.advance(1e9, max_steps=30).iteration == 30
    off, nbr = eng.neighbor_list()
    want = eng.particle_fields(("shepard",))["shepard"]
    d = eng.download(("Position", "Density"))
    cfg = eng.cfg
    X, V = np.asarray(d["Position"], np.float64), cfg.m0 / np.asarray(d["Density"], np.float64)
    i, j = neighbors.pairs(off, nbr)
    r = np.sqrt(((X[i] - X[j]) ** 2).sum(1))
    S = V * float(kernel_w(cfg, 0.0)) + neighbors.pair_sum(off, V[j] * kernel_w(cfg, r * cfg.h_inv))
    worst = np.abs(S - want).max() / np.abs(want).max()
    print(f"fp{8 * fb}: {len(nbr)} entries, Shepard sum from the list against the library's: {worst:.3g} of its maximum (bar {BAR[fb]:g})")
    assert worst <= BAR[fb]
    eng.close()


# ---- 3. stale lists ---------------------------------------------------------------------------------------------------------------
def test_stale_cell_lists(request):
    """A build at least 15 steps behind the last rebuild — rows have drifted out of the cell `cstart` files them under — and one
    directly behind a rebuild, found as tests/test_particle_fields_gpu.py::test_stale_lists finds them."""
    for vel in (1.0, 0.3):                                                         # slower particles: longer stretches between rebuilds
        p, s = _state("dam_break_2d", request, vel=vel)
        K = 64
        history = []
        for k in range(1, K + 1):
            eng = _engine(p, s, 8)
            history.append(eng.advance(1e9, max_steps=k).n_rebuilds)
            eng.close()
        rebuilt_before = [1] + [k for k in range(2, K + 1) if history[k - 1] > history[k - 2]]
        since = [k - max(b for b in rebuilt_before if b <= k) for k in range(1, K + 1)]
        print(f"vel {vel}: rebuilds before steps {rebuilt_before}; longest stretch without one {max(since) + 1} steps")
        if max(since) >= 15:
            break
    assert max(since) >= 15, "no step of the run lies 15 steps behind the last rebuild"
    far = 1 + int(np.argmax(since))
    eng = _engine(p, s, 8)
    pr = eng.advance(1e9, max_steps=far)
    assert pr.n_rebuilds == history[far - 1]
    _check(eng, f"step {far}, {since[far - 1] + 1} steps behind the last rebuild")
    before = pr.n_rebuilds
    pr = eng.advance(1e9, max_steps=1)                                             # every sphmi_advance opens with a rebuild
    assert pr.n_rebuilds == before + 1
    _check(eng, "one step behind a rebuild")
    eng.close()


# ---- 4. run and row-length edges --------------------------------------------------------------------------------------------------------
def _cloud(p0, rows, position=None, walls=False):
    from sphexample_amd.preprocess import FIELD_NAMES, SimParticles
    p = SimParticles(p0.Dimensions, p0.FloatType, **{k: np.ascontiguousarray(getattr(p0, k)[:rows]).copy() for k in FIELD_NAMES})
    if position is not None:
        p.Position[...] = position
    if walls:
        p.Type[...] = 2
        p.Velocity[...] = 0
    return p


@pytest.mark.parametrize("fb", [8, 4])
@pytest.mark.parametrize("rows", [1, 255, 256, 257, 513])
def test_run_edges(rows, fb, request):
    """The first `rows` rows of dam_break_2d as a cloud of their own: one row, one short of a run of 256, a run, a run and a row,
    two runs and a row."""
    p0, s = request.getfixturevalue("dam_break_2d")
    assert len(p0) > rows
    eng = _engine(_cloud(p0, rows), s, fb)
    assert eng.advance(1e9, max_steps=1).iteration == 1
    off, nbr, _ = _check(eng, f"{rows} rows fp{8 * fb}")
    if rows == 1:
        assert off.tolist() == [0, 0] and len(nbr) == 0
        assert eng.neighbors_build() == (1, 0)
        only_off, none = eng.neighbors_read(neighbors=False)                        # neighbors_out = NULL
        assert none is None and only_off.tolist() == [0, 0]
        none, only_nbr = eng.neighbors_read(offsets=False)
        assert none is None and len(only_nbr) == 0
    else:
        assert len(nbr) > 0
    eng.close()


@pytest.mark.parametrize("fb", [8, 4])
def test_row_length_edges(fb, request):
    """Rows of 0, 1, 2, … 64 neighbours side by side, so that segments of every length and every alignment follow one another in
    the arena: fixed clusters of m rows on a segment shorter than H/2 — everyone within H of everyone, m - 1 neighbours each —
    3H apart.  (The fill pass that shipped stores entry by entry: there is no flush length whose edges would need cases.)"""
    p0, s = request.getfixturevalue("dam_break_2d")
    H = s.SimKernel.H
    sizes = [1, 2, 16, 17, 18, 34, 3, 65, 5, 48, 2, 20]
    pos, x0 = [], 0.0
    for m in sizes:
        for k in range(m):
            pos.append((x0 + 0.45 * H * k / max(m - 1, 1), 0.1 + 0.05 * H * (k % 3)))
        x0 += 3 * H
    pos = np.array(pos)
    eng = _engine(_cloud(p0, len(pos), pos, walls=True), s, fb)
    assert eng.advance(1e9, max_steps=1).iteration == 1
    off, nbr, _ = _check(eng, f"row-length edges fp{8 * fb}")
    cnt = np.diff(off)
    print(f"row lengths present: {sorted(set(cnt.tolist()))}")
    assert {0, 1, 15, 16, 17, 33, 64} <= set(cnt.tolist())
    assert sorted(cnt.tolist()) == sorted(m - 1 for m in sizes for _ in range(m))
    eng.close()


# ---- 5. the same bytes, no side effects --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fb", [8, 4])
def test_repeats_and_does_not_disturb(fb, request):
    p, s = _state("dam_break_2d", request)
    markers = sorted(int(m) for m in np.unique(p.GroupMarker))
    Fl = p.Position[p.Type == 1]
    probes = np.array([Fl.mean(0), Fl.min(0) + 0.05, Fl.max(0) - 0.05])
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
                eng.neighbors_build()
                a = eng.neighbors_read()
                eng.neighbors_build()                                              # no step in between: the same bytes
                b = eng.neighbors_read()
                assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
                assert eng.neighbors_read()[1].tobytes() == a[1].tobytes()          # … and a second read of one build
        runs.append((prog, eng.download(), eng.group_forces_read(), eng.probes_read()))
        if called:
            # a download begun before a build completes with the snapshot taken at its begin
            want = eng.download()
            spec = {k: np.zeros_like(want[k]) for k in ("Position", "Velocity", "Acceleration", "Density", "Pressure", "ID", "Type", "GroupMarker", "GhostPoints", "Cells")}
            fbeg = eng._fn("download_begin"); fbeg.argtypes = [C.c_void_p] * 11
            eng._check(fbeg(eng._h, *[spec[k].ctypes.data_as(C.c_void_p) for k in spec]))
            eng.neighbors_build()
            mid = eng.neighbors_read()
            eng.download_end()
            for k in spec:
                np.testing.assert_array_equal(spec[k], want[k], err_msg=k)
            assert mid[0].tobytes() == a[0].tobytes() and mid[1].tobytes() == a[1].tobytes()
        eng.close()
    assert runs[0][0][-1][0] == 40 and runs[0][0] == runs[1][0]                    # the progress blocks, n_rebuilds among them
    for k, v in runs[0][1].items():
        assert runs[1][1][k].tobytes() == v.tobytes(), k                            # the final download, byte for byte
    for a, b in zip(runs[0][2], runs[1][2]):
        np.testing.assert_array_equal(a, b)                                         # the group-force series
    assert len(runs[0][3]["iteration"]) == 40
    for k in runs[0][3]:
        np.testing.assert_array_equal(runs[1][3][k], runs[0][3][k], err_msg=k)      # the probe series


# ---- 6. lifetime and errors --------------------------------------------------------------------------------------------------------
def _refused(call, status, word):
    with pytest.raises(SphmiError) as ei:
        call()
    assert ei.value.status == status and word in str(ei.value), str(ei.value)


def test_lifetime(request):
    p, s = _state("dam_break_2d", request)
    eng = _engine(p, s, 8)
    _refused(eng.neighbors_read, ERR_STATE, "no neighbour list")                   # before any build (and before any step)
    assert eng.advance(1e9, max_steps=3).iteration == 3
    _refused(eng.neighbors_read, ERR_STATE, "no neighbour list")
    n_rows, n_pairs = eng.neighbors_build()
    off, nbr = eng.neighbors_read()
    assert len(off) == n_rows + 1 and len(nbr) == n_pairs > 0
    assert eng.advance(1e9, max_steps=1).steps_done == 1
    _refused(eng.neighbors_read, ERR_STATE, "stale")                               # rows may have moved
    assert eng.neighbors_build()[0] == n_rows                                      # a new build after a stale result serves again
    off2, nbr2 = eng.neighbors_read()
    ref = brute_force_neighbors(eng.cfg, eng.download(("Position",))["Position"])
    np.testing.assert_array_equal(off2, ref[0]); np.testing.assert_array_equal(nbr2, ref[1])
    eng.forces_once()
    _refused(eng.neighbors_read, ERR_STATE, "stale")
    assert eng.advance(1e9, max_steps=1).steps_done == 1
    eng.neighbors_build()
    eng.upload_particles(p)                                                        # a new particle set
    _refused(eng.neighbors_read, ERR_STATE, "stale")
    _refused(eng.neighbors_build, ERR_STATE, "has not executed a step")
    _refused(eng.neighbors_read, ERR_STATE, "")                                    # (a refused build leaves nothing to read)
    assert eng.advance(1e9, max_steps=2).steps_done == 2
    eng.neighbors_build()
    eng.neighbors_release()
    _refused(eng.neighbors_read, ERR_STATE, "no neighbour list")                   # after release
    eng.neighbors_release()                                                        # releasing nothing is legal
    assert eng.neighbors_build()[1] == len(eng.neighbors_read()[1])
    assert eng.advance(1e9, max_steps=1).steps_done == 1
    eng.close()


def test_errors(request):
    from sphexample_amd._abi import make_config
    from sphexample_amd.engine import Engine
    p, s = _state("dam_break_2d", request)
    cfg = make_config(len(p), s.SimConstants, s.SimKernel, s.SimMetaData, s.SimViscosity, s.SimDensityDiffusion, device_float_bytes=8, host_float_bytes=8)
    bare = Engine(cfg)
    _refused(bare.neighbors_build, ERR_STATE, "before sphmi_upload")
    bare.upload_particles(p)
    _refused(bare.neighbors_build, ERR_STATE, "has not executed a step")           # uploaded, no step yet: no cell list
    assert bare.advance(1e9, max_steps=3).iteration == 3                            # the handle still advances …
    f = bare._fn("neighbors_build")
    f.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    rows, pairs = C.c_int64(), C.c_int64()
    for mode in (2, -1, 7):
        _refused(lambda: bare._check(f(bare._h, mode, C.byref(rows), C.byref(pairs))), ERR_ARGUMENT, "unknown mode")
    _refused(lambda: bare._check(f(bare._h, 0, C.byref(rows), None)), ERR_ARGUMENT, "null n_pairs_out")
    bare._check(f(bare._h, 1, None, C.byref(pairs)))                               # n_rows_out may be NULL
    with pytest.raises(RuntimeError, match="did not build"):                       # the wrapper sizes its arrays from its OWN build: it
        bare.neighbors_read()                                                      # refuses a list built behind its back, and writes nothing
    assert pairs.value > 0 and bare.neighbors_build() == (len(p), 2 * pairs.value)  # … and serves
    assert bare.advance(1e9, max_steps=1).steps_done == 1
    bare.close()
    slabs = _engine(p, s, 8, devices=[0, 0])                                       # two slabs on one GPU
    _refused(slabs.neighbors_build, ERR_STATE, "single-device")
    slabs.advance(1e9, max_steps=3)
    _refused(slabs.neighbors_build, ERR_STATE, "single-device")                    # … with a cell list too
    _refused(slabs.neighbors_read, ERR_STATE, "no neighbour list")
    slabs.neighbors_release()
    assert slabs.advance(1e9, max_steps=2).steps_done == 2
    slabs.close()
    thin = _engine(p, _variant(s, None, 0.9), 8)                                   # H < h
    _refused(thin.neighbors_build, ERR_STATE, "H < h")
    assert thin.advance(1e9, max_steps=1).steps_done == 1
    _refused(thin.neighbors_build, ERR_STATE, "H < h")
    assert thin.advance(1e9, max_steps=2).steps_done == 2
    thin.close()


def test_errors_rank_mode(request):
    """A rank-mode handle holds one slab of the rows per process: refused like a multi-device handle, and it goes on advancing.
    (Its own test: bringing up the communicator of a rank-mode handle takes most of the time.)"""
    p, s = _state("dam_break_2d", request)
    from sphexample_amd.engine import rccl_unique_id
    rk = _engine(p, s, 8, rank=0, world=1, unique_id=rccl_unique_id())             # rank mode: one slab of the rows per process
    for _ in range(2):                                                             # before the first step, and with a cell list
        with pytest.raises(SphmiError) as ei:
            rk.neighbors_build()
        assert ei.value.status == ERR_STATE and "single-device" in str(ei.value) and "rank-mode" in str(ei.value), str(ei.value)
        _refused(rk.neighbors_read, ERR_STATE, "no neighbour list")
        rk.neighbors_release()
        assert rk.advance(1e9, max_steps=2).steps_done == 2                         # the handle still advances
    rk.close()
