"""sphmi_attach_columns / sphmi_download_columns* — the caller's passive columns on the device.

The reference's sort! permutes all 17 fields of the SimParticles StructArray (src/SPHCellList.jl:142); the engine carries ten.
The others are attached once as opaque rows, stay on the device, and every output delivers them in the current cell-sorted
order: the permutation never visits the host.  Every comparison here is BYTE-EXACT — a column is opaque bytes and a
permutation has no tolerance; no row is sampled.
"""
import copy
import ctypes as C
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 3, 4, 8, 12, 16, 24, 40, 64, 1, 8, 24, 7, 33, 64)


def _random_columns(n, widths=WIDTHS, seed=5):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=(n, w), dtype=np.uint8) for w in widths]


def _like(cols):
    return [np.full_like(a, 0xA5) for a in cols]


def _seven(ids, ft=np.float64, dims=3):
    """The RunSimulation set (ChunkID, GravityFactor, MotionLimiter, BoundaryBool, GhostNormals, Kernel, KernelGradient) with
    every value a function of the particle's ID: 81 bytes per row in 3-D Float64."""
    f = ids.astype(ft)
    vec = lambda a, b: np.ascontiguousarray(np.stack([f * a + b * k for k in range(dims)], axis=1))  # noqa: E731
    return [ids * 3 + 1, f * ft(0.5), -f, (ids % 251).astype(np.uint8), vec(1.0, 0.25), f + ft(0.25), vec(-2.0, 1.0)]


def _origins_from_the_oracle(q, s, n_calls=4, steps=25):
    """origin_k[i]: the upload row of the particle in row i after interval k — composed from the ORACLE's permutations."""
    from oracle.oracle import make_oracle
    orc = make_oracle(q, s)
    origin, out = np.arange(len(q)), []
    for _ in range(n_calls):
        orc.advance(1e9, max_steps=steps)
        origin = origin[orc.download_permutation()]
        out.append(origin.copy())
    orc.close()
    return out


@pytest.fixture(scope="module")
def fast_2d(dam_break_2d):
    """The input of tests/test_permutation.py (>= 3 rebuilds and moved rows within four intervals of 25 steps)."""
    from conftest import perturbed
    p, s = dam_break_2d
    return perturbed(p, seed=1, vel_scale=3.0), s


@pytest.fixture(scope="module")
def oracle_origins(fast_2d):
    return _origins_from_the_oracle(*fast_2d)


@pytest.fixture(scope="module")
def c3_flowing():
    from conftest import load_dam_break_3d_c3_flowing
    return load_dam_break_3d_c3_flowing()


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host32", [False, True])
@pytest.mark.parametrize("fb", [4, 8])
def test_round_trip_without_a_sort(dam_break_2d, fb, host32):
    from sphexample_amd.engine import make_engine
    from test_host_float32_gpu import as_float32
    p, s = dam_break_2d
    eng = make_engine(as_float32(p) if host32 else p, s, device_float_bytes=fb)
    cols = _random_columns(len(p))
    eng.attach_columns(cols)
    outs = _like(cols)
    eng.download_columns(outs)
    for c, (a, b) in enumerate(zip(cols, outs)):
        np.testing.assert_array_equal(b, a, err_msg=f"column {c}, {WIDTHS[c]} bytes")
    # NULL entries skip their column
    outs = _like(cols)
    eng.download_columns([o if c % 3 == 1 else None for c, o in enumerate(outs)])
    for c, (a, b) in enumerate(zip(cols, outs)):
        np.testing.assert_array_equal(b, a if c % 3 == 1 else np.full_like(a, 0xA5), err_msg=f"column {c}")
    # one column, every width class on its own
    for w in (1, 3, 4, 24, 64):
        one = _random_columns(len(p), (w,), seed=w)
        eng.attach_columns(one)
        got = _like(one)
        eng.download_columns(got)
        np.testing.assert_array_equal(got[0], one[0], err_msg=f"single column of {w} bytes")
    eng.close()


# 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices", [None, [0, 0], [0, 0, 0]])
def test_columns_follow_the_sorts_like_the_oracles_permutation(fast_2d, oracle_origins, devices):
    from sphexample_amd.engine import make_engine
    q, s = fast_2d
    eng = make_engine(q, s, device_float_bytes=8, devices=devices)
    cols = _random_columns(len(q))[:15] + [np.ascontiguousarray(q.ID * 3 + 1)]
    eng.attach_columns(cols)
    moved = 0
    for origin in oracle_origins:
        prog = eng.advance(1e9, max_steps=25)
        ids = eng.download(("ID",))["ID"]
        outs = _like(cols)
        eng.download_columns(outs)
        for c, (a, b) in enumerate(zip(cols, outs)):
            np.testing.assert_array_equal(b, a[origin], err_msg=f"column {c}")
        np.testing.assert_array_equal(outs[15], ids * 3 + 1)
        moved += int((origin != np.arange(len(q))).sum())
    assert moved > 0 and prog.n_rebuilds >= 3
    eng.close()


# 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_columns_do_not_depend_on_download_permutation(fast_2d, devices):
    from sphexample_amd.engine import make_engine
    q, s = fast_2d
    cols = _random_columns(len(q), (1, 8, 24, 7), seed=9) + [np.ascontiguousarray(q.ID * 3 + 1)]
    asks, never, bare = (make_engine(q, s, device_float_bytes=8, devices=devices) for _ in range(3))
    asks.attach_columns(cols); never.attach_columns(cols)
    calls = {1: 1, 2: 2, 3: 1, 4: 0}                       # download_permutation calls of `asks` (and `bare`) after interval k
    for k in (1, 2, 3, 4):
        for e in (asks, never, bare):
            e.advance(1e9, max_steps=25)
        for _ in range(calls[k]):
            np.testing.assert_array_equal(asks.download_permutation(), bare.download_permutation())
        a, b = _like(cols), _like(cols)
        asks.download_columns(a); never.download_columns(b)
        ids = never.download(("ID",))["ID"]
        for c in range(len(cols)):
            np.testing.assert_array_equal(a[c], b[c], err_msg=f"interval {k}, column {c}")
        np.testing.assert_array_equal(b[-1], ids * 3 + 1)
        # a column download does not move the permutation's epoch: asked twice, the second answer is the identity
        if k == 2:
            np.testing.assert_array_equal(asks.download_permutation(), np.arange(len(q)))
            np.testing.assert_array_equal(bare.download_permutation(), np.arange(len(q)))
    for e in (asks, never, bare):
        e.close()


@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_attach_late_in_a_run(fast_2d, devices):
    """Attached after sorts the caller never asked about (the row column is not the identity then): row r of the attached arrays
    is the particle of row r of the download at that moment."""
    from sphexample_amd.engine import make_engine
    q, s = fast_2d
    eng = make_engine(q, s, device_float_bytes=8, devices=devices)
    eng.advance(1e9, max_steps=50)
    ids0 = eng.download(("ID",))["ID"]
    assert (ids0 != q.ID).any()
    cols = [np.ascontiguousarray(ids0 * 3 + 1), (ids0 % 251).astype(np.uint8)]
    eng.attach_columns(cols)
    for k in range(3):
        eng.advance(1e9, max_steps=25)
        if k == 1:
            eng.download_permutation()
        ids = eng.download(("ID",))["ID"]
        outs = _like(cols)
        eng.download_columns(outs)
        np.testing.assert_array_equal(outs[0], ids * 3 + 1)
        np.testing.assert_array_equal(outs[1], (ids % 251).astype(np.uint8))
    assert (ids != ids0).any()
    eng.close()


# 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page_locked", [True, False])
def test_asynchronous_columns_hold_the_snapshot_before_the_advance(fast_2d, page_locked):
    from sphexample_amd.engine import make_engine
    q, s = fast_2d
    cols = _random_columns(len(q), (1, 8, 24, 12), seed=2) + [np.ascontiguousarray(q.ID * 3 + 1)]
    eng, twin = make_engine(q, s, device_float_bytes=8), make_engine(q, s, device_float_bytes=8)
    eng.attach_columns(cols); twin.attach_columns(cols)
    pe, pt = q.copy(), q.copy()
    outs, want = _like(cols), _like(cols)
    if page_locked:
        eng.pin(pe); eng.pin(outs)
    for e in (eng, twin):
        e.advance(1e9, max_steps=50)
    twin.download_into(pt); twin.download_columns(want)
    eng.download_into_begin(pe)
    eng.download_columns_begin(outs)
    eng.advance(1e9, max_steps=25)
    eng.download_end()
    np.testing.assert_array_equal(pe.ID, pt.ID)
    np.testing.assert_array_equal(pe.Position, pt.Position)
    for c in range(len(cols)):
        np.testing.assert_array_equal(outs[c], want[c], err_msg=f"column {c}")
    np.testing.assert_array_equal(outs[-1], pe.ID * 3 + 1)
    assert (eng.download(("ID",))["ID"] != pe.ID).any()          # the advance in between did sort
    eng.unpin(); eng.close(); twin.close()


# 5 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_columns_do_not_depend_on_unique_ids(fast_2d, devices):
    from sphexample_amd.engine import make_engine
    q, s = fast_2d
    dup = q.copy()
    dup.ID[:] = 7
    cols = _random_columns(len(q), (4, 1, 24), seed=4)
    ref, eng = make_engine(q, s, device_float_bytes=8, devices=devices), make_engine(dup, s, device_float_bytes=8, devices=devices)
    ref.attach_columns(cols); eng.attach_columns(cols)
    for k in range(4):
        ref.advance(1e9, max_steps=25); eng.advance(1e9, max_steps=25)
        a, b = _like(cols), _like(cols)
        ref.download_columns(a); eng.download_columns(b)
        assert (eng.download(("ID",))["ID"] == 7).all()
        for c in range(len(cols)):
            np.testing.assert_array_equal(b[c], a[c], err_msg=f"interval {k}, column {c}")
    assert any((a[c] != cols[c]).any() for c in range(len(cols)))
    ref.close(); eng.close()


# 6 ---------------------------------------------------------------------------------------------------------------------
def _three_d(p, s, steps):
    from sphexample_amd.engine import make_engine
    eng = make_engine(p, s, device_float_bytes=4)
    cols = _seven(p.ID)
    assert sum(a.nbytes // len(p) for a in cols) == 81
    eng.attach_columns(cols)
    for n in steps:
        prog = eng.advance(1e9, max_steps=n)
        ids = eng.download(("ID",))["ID"]
        outs = _like(cols)
        eng.download_columns(outs)
        for c, (a, b) in enumerate(zip(_seven(ids), outs)):
            np.testing.assert_array_equal(b, a, err_msg=f"column {c}")
    eng.close()
    return prog, int((ids != p.ID).sum())


def test_three_d_device_rebuild(dam_break_3d_shipped):
    from conftest import flowing
    p, s = dam_break_3d_shipped
    assert len(p) == 17446
    prog, moved = _three_d(flowing(p), s, (40, 40, 40))       # every call opens with a rebuild (Δx re-armed, src/SPHCellList.jl:739)
    assert prog.n_rebuilds >= 3 and moved > 0, (prog.n_rebuilds, moved)


def test_three_d_host_path_rebuild_at_a_million_rows(c3_flowing):
    p, s = c3_flowing
    assert len(p) == 1057738
    prog, moved = _three_d(p, s, (20, 60))             # every call opens with a rebuild; the Δx criterion asks ≈ 33 steps after one
    assert prog.n_rebuilds >= 3 and moved > 0, (prog.n_rebuilds, moved)


# 7 ---------------------------------------------------------------------------------------------------------------------
def test_life_cycle_and_errors(dam_break_2d):
    from sphexample_amd._abi import ERR_ARGUMENT, ERR_STATE, SphmiError, make_config
    from sphexample_amd.engine import Engine, make_engine
    p, s = dam_break_2d
    n = len(p)
    eng = make_engine(p, s, device_float_bytes=8)
    first, second = _random_columns(n, (8, 1), seed=1), _random_columns(n, (3, 16, 5), seed=2)
    eng.attach_columns(first)
    eng.attach_columns(second)                             # replaces the set
    outs = _like(second)
    eng.download_columns(outs)
    for a, b in zip(second, outs):
        np.testing.assert_array_equal(b, a)
    with pytest.raises(ValueError):
        eng.download_columns(_like(first))                 # (the wrapper refuses arrays that do not match the attached widths)
    eng.attach_columns([])                                 # detach
    with pytest.raises(SphmiError) as ei:
        eng.download_columns([])
    assert ei.value.status == ERR_STATE and "attach" in str(ei.value)
    eng.attach_columns(first)
    eng.upload_particles(p)                                # a new particle set detaches
    table = (C.c_void_p * 2)(*[a.ctypes.data for a in _like(first)])
    raw = eng._fn("download_columns")
    raw.argtypes = [C.c_void_p, C.c_void_p]
    assert raw(eng._h, table) == ERR_STATE
    # argument errors, each with a text
    attach = eng._fn("attach_columns")
    attach.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    last = lambda: eng._fn("last_error")(eng._h).decode()  # noqa: E731
    blob = np.zeros((n, 65), dtype=np.uint8)
    ptrs = (C.c_void_p * 17)(*[blob.ctypes.data] * 17)
    for widths, count, tab, word in (([0], 1, ptrs, "row_bytes"), ([65], 1, ptrs, "row_bytes"), ([1] * 17, 17, ptrs, "n_columns"),
                                     ([4], 1, None, "null"), ([4], -1, ptrs, "n_columns"),
                                     ([4, 4], 2, (C.c_void_p * 2)(blob.ctypes.data, None), "null column")):
        w = (C.c_int32 * len(widths))(*widths)
        assert attach(eng._h, count, tab, w) == ERR_ARGUMENT, (widths, count)
        assert word in last(), (word, last())
    assert attach(eng._h, 1, ptrs, None) == ERR_ARGUMENT
    eng.attach_columns(first)
    assert raw(eng._h, None) == ERR_ARGUMENT and "null" in last()
    eng.close()
    # before the upload
    cfg = make_config(n, s.SimConstants, s.SimKernel, s.SimMetaData, s.SimViscosity, s.SimDensityDiffusion, device_float_bytes=8)
    cold = Engine(cfg)
    with pytest.raises(SphmiError) as ei:
        cold.attach_columns(first)
    assert ei.value.status == ERR_STATE
    with pytest.raises(SphmiError) as ei:
        cold.download_columns(_like(first))
    assert ei.value.status == ERR_STATE
    cold.close()


# 8 ---------------------------------------------------------------------------------------------------------------------
def test_run_simulation_takes_the_device_path(dam_break_2d_mdbc, monkeypatch):
    from oracle.oracle import Oracle
    from sphexample_amd import simulation
    from sphexample_amd.simulation import PASSIVE_FIELDS, RunSimulation
    p, s = dam_break_2d_mdbc
    host_gather = simulation.permute_passive_fields
    calls = {"n": 0}

    def counted(*a, **kw):
        calls["n"] += 1
        return host_gather(*a, **kw)

    def refused(*a, **kw):
        raise AssertionError("the host gathers ran")

    got, n_calls = {}, {}
    runs = (("gpu", dict(device_float_bytes=8, async_output=True), refused, None), ("gpu_sync", dict(device_float_bytes=8), refused, None),
            ("cpu", dict(backend_factory=Oracle), counted, None), ("gpu_off", dict(device_float_bytes=8, async_output=True), counted, "0"),
            ("gpu_sync_off", dict(device_float_bytes=8), counted, "0"))
    for name, kw, gather, switch in runs:
        monkeypatch.setattr(simulation, "permute_passive_fields", gather)
        if switch is None:
            monkeypatch.delenv("SPHMI_COLUMNS", raising=False)
        else:
            monkeypatch.setenv("SPHMI_COLUMNS", switch)
        calls["n"] = 0
        meta = copy.deepcopy(s.SimMetaData)
        meta.SimulationTime, meta.OutputTimes = 0.004, 0.001
        q = p.copy()
        q.ChunkID[:] = q.ID * 3 + 1
        assert np.abs(q.GhostNormals).max() > 0
        normal_of_id = dict(zip(q.ID.tolist(), map(tuple, q.GhostNormals)))
        snaps = []
        RunSimulation(SimGeometry=None, SimMetaData=meta, SimConstants=s.SimConstants, SimKernel=s.SimKernel, SimLogger=None,
                      SimParticles=q, SimViscosity=s.SimViscosity, SimDensityDiffusion=s.SimDensityDiffusion,
                      on_output=lambda m, pp: snaps.append({k: getattr(pp, k).copy() for k in PASSIVE_FIELDS + ("ID", "Type", "Kernel", "KernelGradient")}), **kw)
        got[name], n_calls[name] = snaps, calls["n"]
        for sn in snaps:
            np.testing.assert_array_equal(sn["ChunkID"], sn["ID"] * 3 + 1)
            np.testing.assert_array_equal(sn["GravityFactor"], np.where(sn["Type"] == 1, -1.0, np.where(sn["Type"] == 3, 1.0, 0.0)))
            np.testing.assert_array_equal(sn["MotionLimiter"], (sn["Type"] == 1).astype(float))
            np.testing.assert_array_equal(sn["BoundaryBool"], (sn["Type"] != 1).astype(np.uint8))
            assert all(tuple(nrm) == normal_of_id[int(i)] for i, nrm in zip(sn["ID"], sn["GhostNormals"]))
    assert len(got["cpu"]) >= 5 and all(len(v) == len(got["cpu"]) for v in got.values())
    assert n_calls["gpu"] == n_calls["gpu_sync"] == 0
    assert n_calls["cpu"] == n_calls["gpu_off"] == n_calls["gpu_sync_off"] == len(got["cpu"]) - 1      # one per interval (the first output is the initial state)
    for name in ("gpu", "gpu_sync", "gpu_off", "gpu_sync_off"):
        for a, b in zip(got[name], got["cpu"]):
            for k in a:
                np.testing.assert_array_equal(a[k], b[k], err_msg=f"{name}: {k}")


# 9 ---------------------------------------------------------------------------------------------------------------------
def test_device_path_is_faster_than_the_host_gathers(c3_flowing):
    """Median of five, the two alternating in one process, page-locked targets, 1 057 738 rows x the seven columns (81 bytes):
    `download_columns` against `download_permutation` + one np.take per column.  The condition is only that the device path
    wins; both medians are printed (profiles/columns_on_device.md records them)."""
    from sphexample_amd.engine import make_engine
    p, s = c3_flowing
    eng = make_engine(p, s, device_float_bytes=4)
    cols = _seven(p.ID)
    eng.attach_columns(cols)
    outs = _like(cols)
    eng.pin(outs)
    host = [a.copy() for a in cols]
    t_dev, t_host = [], []
    for _ in range(5):
        eng.advance(1e9, max_steps=40)                     # opens with a rebuild and reaches the next: both paths see a fresh sort
        t0 = time.perf_counter()
        eng.download_columns(outs)
        t1 = time.perf_counter()
        prev = eng.download_permutation()
        for a in host:
            a[...] = np.take(a, prev, axis=0)
        t2 = time.perf_counter()
        t_dev.append(t1 - t0); t_host.append(t2 - t1)
    ids = eng.download(("ID",))["ID"]
    for c, (a, b, h) in enumerate(zip(_seven(ids), outs, host)):
        np.testing.assert_array_equal(b, a, err_msg=f"column {c}")
        np.testing.assert_array_equal(h, a, err_msg=f"host column {c}")
    dev, hst = float(np.median(t_dev)), float(np.median(t_host))
    print(f"\ncolumns at N = {len(p)}: device path {dev * 1e3:.2f} ms, host path {hst * 1e3:.2f} ms (medians of 5), ratio {hst / dev:.1f}")
    eng.unpin(); eng.close()
    assert dev < hst, (t_dev, t_host)
