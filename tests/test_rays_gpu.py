"""The first crossing of S = level along rays on the device (sphmi_cast_rays, csrc/sphmi_rays.h) — needs a real MI355X.

The yardstick predates the kernel: `sphexample_amd.rays.restate` performs the complete search on the host with
``Backend.sample_point_gradients`` as its only evaluator, and the device must deliver the same status, interval, bracket, point and
five sums BIT FOR BIT (np.array_equal on every output; NaN brackets compare equal as NaN).  Against an evaluator that never calls
the library — `brute_force_weight` of tests/test_rays_host.py, an O(M·N) enumeration — brackets agree within step / 2²⁴ + 1e-12; a ray
may be excluded only where the enumeration itself shows an evaluated point with |S − level| < 1e-9, at most 1 % of the rays
(tests/test_rays_host.py asserts the cap on the enumeration alone)."""
import numpy as np
import pytest

from sphexample_amd import rays
from sphexample_amd._abi import ERR_ARGUMENT, ERR_STATE, SphmiError
from test_probes_gpu import FIELDS, _engine, _state, _variant
from test_rays_host import BRUTE_K, BRUTE_SEED, KS, brute_force_weight, gauge_rays

pytestmark = pytest.mark.gpu

CASES = {"dam_break_2d": 30, "dam_break_3d_shipped": 12}          # fixture → steps
KEYS = ("status", "interval", "bracket", "point", "weight", "count", "sum_pressure", "sum_density", "sum_velocity")
SUMS = ("weight", "count", "sum_pressure", "sum_density", "sum_velocity")


def _start(case, fb, request, steps=None, **kw):
    p, s = _state(case, request)
    eng = _engine(p, s, fb, **kw)
    eng.advance(1e9, max_steps=CASES[case] if steps is None else steps)
    return eng, p, s


def _evaluator(eng):
    return lambda x: eng.sample_point_gradients(x, fields=SUMS)


def _same(got, want, what):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(got[k], want[k], equal_nan=got[k].dtype == np.float64), (what, k, np.flatnonzero((got[k] != want[k]).reshape(len(got[k]), -1).any(1))[:8])


def _fluid_box(p):
    F = np.asarray(p.Position, np.float64)[np.asarray(p.Type) == 1]
    return F.min(0), F.max(0)


@pytest.mark.parametrize("fb", [8, 4])
@pytest.mark.parametrize("case", list(CASES))
def test_bitwise_against_the_existing_sampler(case, fb, request):
    """Every mode; 1, 63, 64, 65 and 257 rays; K = 1, 63, 64, 65, 129; then t_begin shifted by whole steps so that the crossing lands
    on 63, 64 and 65 — the seam between two march rounds."""
    eng, p, s = _start(case, fb, request)
    lo, hi = _fluid_box(p)
    H = eng.cfg.H
    ev = _evaluator(eng)
    hits = 0
    # (… and off the diagonal: one ray with a long march, a tail workgroup of short ones)
    for n, K, seed in [(n, K, 100 + n) for n, K in zip((1, 63, 64, 65, 257), KS)] + [(1, 129, 201), (257, 1, 457), (65, 129, 265)]:
        o, d, te, step = gauge_rays(lo, hi, H, n, K, seed=seed)
        for mode in rays.MODES:
            got = eng.cast_rays(o, d, te, step=step, level=0.5, mode=mode)
            want = rays.restate(ev, o, d, 0.0, te, step, 0.5, mode)
            assert (rays.intervals(0.0, te, step) == K).all()
            _same(got, want, f"{n} rays, K = {K}, {mode}")
            hits += int((got["status"] & 1).sum())
            assert np.all(got["weight"][(got["status"] & 1) != 0] >= 0.5)            # the record describes fluid
    assert hits > 300
    # the seam: march with a fine step, then start every ray earlier by whole steps so that its crossing index becomes `target`
    o, d, te, step = gauge_rays(lo, hi, H, 96, 129, seed=7)
    first = eng.cast_rays(o, d, te, step=step, mode="enter")
    sel = first["interval"] >= 1
    assert sel.sum() >= 40
    o, d, te, k0 = o[sel], d[sel], te[sel], first["interval"][sel]
    for target in (63, 64, 65):
        tb = -(target - k0).astype(np.float64) * step
        got = eng.cast_rays(o, d, te, t_begin=tb, step=step, mode="enter")
        want = rays.restate(ev, o, d, tb, te, step, 0.5, "enter")
        _same(got, want, f"seam {target}")
        print(f"{case} fp{8 * fb}: target {target}: intervals {np.bincount(np.maximum(got['interval'], 0), minlength=70)[60:68].tolist()} at 60..67")
        assert (got["interval"] == target).sum() >= len(k0) // 2 and np.abs(got["interval"] - target).max() <= 1
    eng.close()


@pytest.mark.parametrize("fb", [8, 4])
@pytest.mark.parametrize("case", list(CASES))
def test_record_at_the_hit_and_independence(case, fb, request):
    eng, p, s = _start(case, fb, request)
    lo, hi = _fluid_box(p)
    D = eng.D
    o, d, te, step = gauge_rays(lo, hi, eng.cfg.H, 200, 40, seed=11)
    r = eng.cast_rays(o, d, te, step=step, mode="any")
    pts, idx = rays.hit_points(r, D)
    assert len(idx) > 100
    at = eng.sample_point_gradients(pts, fields=SUMS)
    for k in SUMS:
        assert np.array_equal(at[k], r[k][idx]), k                                  # the record is the sampler's at point_out
    if D == 2:
        assert (r["point"][idx, 2] == 0).all() and (r["sum_velocity"][:, 2] == 0).all() and (r["point"][:, 2][(r["status"] & 1) == 0] == 0).all()
    miss = (r["status"] & 1) == 0
    assert np.isnan(r["bracket"][miss]).all() and np.isnan(r["point"][miss, :D]).all() and (r["interval"][miss] == -1).all()
    assert all((r[k][miss] == 0).all() for k in SUMS)
    # a repeated call, a subset, the rays shuffled, a ray given twice
    _same(eng.cast_rays(o, d, te, step=step, mode="any"), r, "repeat")
    sub = np.arange(0, 200, 3)
    perm = np.random.default_rng(5).permutation(200)
    twice = np.concatenate([np.arange(200), [17, 17, 133]])
    for name, sel in (("subset", sub), ("shuffled", perm), ("twice", twice)):
        g = eng.cast_rays(o[sel], d[sel], te[sel], step=step, mode="any")
        _same(g, {k: r[k][sel] for k in KEYS}, name)
    # outputs may be NULL
    only = eng.cast_rays(o, d, te, step=step, mode="any", fields=("bracket",))
    assert list(only) == ["bracket"] and np.array_equal(only["bracket"], r["bracket"], equal_nan=True)
    eng.close()


@pytest.mark.parametrize("fb", [8, 4])
def test_against_brute_force(fb, request):
    eng, p, s = _start("dam_break_2d", fb, request)
    lo, hi = _fluid_box(p)
    o, d, te, step = gauge_rays(lo, hi, eng.cfg.H, 120, BRUTE_K, seed=BRUTE_SEED)
    dl = eng.download(FIELDS)
    brute = lambda x: {"weight": brute_force_weight(eng.cfg, x, dl["Position"], dl["Density"], dl["Type"])}      # noqa: E731
    for mode in rays.MODES:
        got = eng.cast_rays(o, d, te, step=step, mode=mode)
        ref = rays.restate(brute, o, d, 0.0, te, step, 0.5, mode)
        near = ref["margin"] < 1e-9                                                 # an evaluated point at the level: its side is rounding's
        both = ((got["status"] & 1) != 0) & ((ref["status"] & 1) != 0)
        gap = np.where(both, np.abs(got["bracket"] - ref["bracket"]).max(axis=1), 0.0)
        differs = (got["status"] != ref["status"]) | (got["interval"] != ref["interval"]) | ~(gap <= step / 2 ** 24 + 1e-12)
        excluded = differs & near
        print(f"fp{8 * fb} {mode}: {int(both.sum())} hits of {len(o)}, {int(near.sum())} rays with a point within 1e-9 of the level, {int(differs.sum())} differ, "
              f"{int(excluded.sum())} excluded, worst bracket gap {gap[~excluded].max():.3g} (bar {step / 2 ** 24 + 1e-12:.3g})")
        assert not (differs & ~near).any(), np.flatnonzero(differs & ~near)
        assert excluded.sum() <= 0.01 * len(o)
        assert both.sum() > 40
    eng.close()


@pytest.mark.parametrize("fb", [8, 4])
@pytest.mark.parametrize("case", list(CASES))
def test_places(case, fb, request):
    eng, p, s = _start(case, fb, request)
    lo, hi = _fluid_box(p)
    D, H = eng.D, eng.cfg.H
    ev = _evaluator(eng)
    mid = 0.5 * (lo + hi)
    down, up = np.zeros(D), np.zeros(D)
    down[D - 1], up[D - 1] = -1.0, 1.0
    step = 0.5 * eng.cfg.h
    inside = mid.copy(); inside[0] = lo[0] + 2 * H; inside[D - 1] = lo[D - 1] + 2 * H
    far = lo - 500 * H
    above = mid.copy(); above[D - 1] = hi[D - 1] + 6 * H
    across = up.copy(); across[0] = 1.0
    o = np.array([inside, inside, far, inside, above, inside])
    d = np.array([up, up, up, up, across, down])
    te = np.array([hi[D - 1] - lo[D - 1] + 4 * H, 0.0, 10 * H, 900 * step, 20 * step, 0.0])
    for mode in rays.MODES:
        got = eng.cast_rays(o, d, te, step=step, mode=mode)
        _same(got, rays.restate(ev, o, d, 0.0, te, step, 0.5, mode), mode)
        st, iv = got["status"], got["interval"]
        assert st[0] & 2 and st[3] & 2                                              # starts inside the fluid
        assert (st[0] & 1) == (mode != "enter")                                     # upwards: LEAVE and ANY find the surface, ENTER nothing
        assert st[1] == 2 and iv[1] == -1 and st[5] == 2                            # t_end == t_begin: no crossing
        assert st[2] == 0 and iv[2] == -1                                           # wholly outside the cell grid
        assert (st[3] & 1) == (mode != "enter")                                     # leaves the fluid, then the grid
        assert st[4] == 0                                                           # empty space above the column
    none = eng.cast_rays(np.zeros((0, D)), np.zeros((0, D)), 1.0, step=step)
    assert list(none) == list(KEYS) and all(len(v) == 0 for v in none.values())
    assert eng.cast_rays(o, d, te)["status"].shape == (6,)                          # the default step, h / 2
    eng.close()


@pytest.mark.parametrize("fb", [8, 4])
def test_stale_lists(fb, request):
    """Calls far behind a rebuild, where rows have drifted out of the cell `cstart` files them under (what
    tests/test_sample_points_gpu.py::test_stale_lists does for the cloud): still the sampler's bits."""
    p, s = _state("dam_break_2d", request)
    lo, hi = _fluid_box(p)
    since = []
    for j in (1, 2, 9, 17, 33, 47, 64, 81, 110):
        eng = _engine(p, s, fb)
        pr = eng.advance(1e9, max_steps=j)
        assert pr.iteration == j
        since.append(pr.n_rebuilds)
        o, d, te, step = gauge_rays(lo, hi, eng.cfg.H, 64, 65, seed=j)
        _same(eng.cast_rays(o, d, te, step=step, mode="any"), rays.restate(_evaluator(eng), o, d, 0.0, te, step, 0.5, "any"), f"step {j}")
        eng.close()
    print(f"fp{8 * fb}: rebuilds so far at the checked steps {since}")
    assert len(set(since)) < len(since), "no two checked calls share a cell list: none lies behind a stale one"


def _raises(status, needle, call):
    with pytest.raises(SphmiError) as e:
        call()
    assert e.value.status == status and needle in str(e.value), str(e.value)


def test_errors(request):
    from sphexample_amd._abi import make_config
    from sphexample_amd.engine import Engine, rccl_unique_id
    p, s = _state("dam_break_2d", request)
    o, d = np.array([[0.3, 1.0], [0.5, 1.0]]), np.array([[0.0, -1.0], [0.0, -1.0]])
    cfg = make_config(len(p), s.SimConstants, s.SimKernel, s.SimMetaData, s.SimViscosity, s.SimDensityDiffusion, device_float_bytes=8, host_float_bytes=8)
    bare = Engine(cfg)
    _raises(ERR_STATE, "sphmi_cast_rays", lambda: bare.cast_rays(o, d, 1.0, step=0.01))      # before the upload
    bare.close()
    eng = _engine(p, s, 8)
    _raises(ERR_STATE, "step", lambda: eng.cast_rays(o, d, 1.0, step=0.01))         # before the first executed step
    eng.advance(1e9, max_steps=3)
    good = eng.cast_rays(o, d, 1.0, step=0.01)
    nan, inf = float("nan"), float("inf")
    bad_o, bad_d, zero_d = o.copy(), d.copy(), d.copy()
    bad_o[1, 0], bad_d[0, 1], zero_d[1] = nan, inf, 0.0
    for needle, call in (("non-finite coordinate at ray 1", lambda: eng.cast_rays(bad_o, d, 1.0, step=0.01)),
                         ("non-finite coordinate at ray 0", lambda: eng.cast_rays(o, bad_d, 1.0, step=0.01)),
                         ("non-finite parameter at ray 1", lambda: eng.cast_rays(o, d, [1.0, nan], step=0.01)),
                         ("non-finite parameter at ray 0", lambda: eng.cast_rays(o, d, 1.0, t_begin=[inf, 0.0], step=0.01)),
                         ("zero direction at ray 1", lambda: eng.cast_rays(o, zero_d, 1.0, step=0.01)),
                         ("t_end < t_begin at ray 0", lambda: eng.cast_rays(o, d, [0.1, 1.0], t_begin=0.5, step=0.01)),
                         ("step", lambda: eng.cast_rays(o, d, 1.0, step=0.0)), ("step", lambda: eng.cast_rays(o, d, 1.0, step=-1.0)),
                         ("step", lambda: eng.cast_rays(o, d, 1.0, step=nan)), ("step", lambda: eng.cast_rays(o, d, 1.0, step=inf)),
                         ("SPHMI_MAX_RAY_POINTS", lambda: eng.cast_rays(o, d, 1.0, step=1e-6)),
                         ("level", lambda: eng.cast_rays(o, d, 1.0, step=0.01, level=0.0)), ("level", lambda: eng.cast_rays(o, d, 1.0, step=0.01, level=nan)),
                         ("level", lambda: eng.cast_rays(o, d, 1.0, step=0.01, level=inf)), ("level", lambda: eng.cast_rays(o, d, 1.0, step=0.01, level=-0.5))):
        _raises(ERR_ARGUMENT, needle, call)
    # what the Python binding refuses itself goes through the C call here: null pointers, the ray count, the mode
    import ctypes as C
    f = eng._fn("cast_rays")
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)                                    # noqa: E731
    tb, te = np.zeros(2), np.ones(2)
    raw = lambda n, po, pd, pb, pe, mode: f(eng._h, n, po, pd, pb, pe, 0.01, 0.5, mode, *[None] * 9)      # noqa: E731
    for needle, call in (("null", lambda: raw(2, None, ptr(d), ptr(tb), ptr(te), 0)), ("null", lambda: raw(2, ptr(o), None, ptr(tb), ptr(te), 0)),
                         ("null", lambda: raw(2, ptr(o), ptr(d), None, ptr(te), 0)), ("null", lambda: raw(2, ptr(o), ptr(d), ptr(tb), None, 0)),
                         ("n_rays", lambda: raw(-1, ptr(o), ptr(d), ptr(tb), ptr(te), 0)), ("n_rays", lambda: raw((1 << 20) + 1, ptr(o), ptr(d), ptr(tb), ptr(te), 0)),
                         ("mode", lambda: raw(2, ptr(o), ptr(d), ptr(tb), ptr(te), 3))):
        _raises(ERR_ARGUMENT, needle, lambda: eng._check(call()))
    assert raw(0, None, None, None, None, 2) == 0                                   # n_rays == 0 is legal
    _same(eng.cast_rays(o, d, 1.0, step=0.01), good, "the handle stays usable")
    eng.close()
    # two slabs on one device: refused, and the text says why
    dd = _engine(p, s, 8, devices=[0, 0], slab_axis=0)
    dd.advance(1e9, max_steps=3)
    _raises(ERR_STATE, "combined S", lambda: dd.cast_rays(o, d, 1.0, step=0.01))
    assert dd.sample_points(o)["weight"].shape == (2,)                              # … and stays usable
    dd.close()
    # H < h
    e2 = _engine(p, _variant(s, None, 0.9), 8)
    e2.advance(1e9, max_steps=1)
    _raises(ERR_STATE, "H < h", lambda: e2.cast_rays(o, d, 1.0, step=0.01))
    e2.close()
    # rank-mode handles: one slab of the rows per process
    rk = _engine(p, s, 8, rank=0, world=1, unique_id=rccl_unique_id())
    _raises(ERR_STATE, "rank-mode", lambda: rk.cast_rays(o, d, 1.0, step=0.01))
    rk.close()


@pytest.mark.parametrize("case,fb", [("dam_break_2d", 4), ("dam_break_3d_shipped", 8)])
def test_does_not_disturb(case, fb, request):
    """A run with cast_rays between its advance calls reports the same progress blocks, downloads the same bytes and records the
    same probe series as one without.  Results HELD on the device across the call — the neighbour list, the isosurface, the
    components — read back with the same bytes and are not stale; the lattice, the cloud and the gradients, whose arenas lie next
    to the rays', give the same bits before and after it.  A download begun before the call completes with the snapshot taken at its
    begin (as tests/test_sample_points_gpu.py::test_does_not_disturb shows for the cloud)."""
    import ctypes as C
    p, s = _state(case, request)
    lo, hi = _fluid_box(p)
    D = len(lo)
    F = np.asarray(p.Position, np.float64)[np.asarray(p.Type) == 1]
    calls = (7, 1, 9) if D == 2 else (5, 1, 4)
    runs = []
    for cast in (False, True):
        eng = _engine(p, s, fb)
        H = eng.cfg.H
        counts = np.array([21, 17] if D == 2 else [11, 9, 7], dtype=np.int64)
        origin = lo - 1.2 * H + 0.318309886 * eng.cfg.dx                           # (no node on the particle lattice)
        lattice = (origin, (hi + 1.2 * H - origin) / (counts - 1), counts)
        pts = np.random.default_rng(61).uniform(lo - 2 * H, hi + 2 * H, (300, D))
        eng.probes_enable(F[:: max(len(F) // 24, 1)][:24] + 0.3 * eng.cfg.dx, capacity=64)
        o, d, te, step = gauge_rays(lo, hi, H, 70, 65, seed=3)
        prog, last = [], None
        for n in calls:
            q = eng.advance(1e9, max_steps=n)
            prog.append((q.iteration, q.steps_done, q.n_rebuilds, q.index_counter, q.total_time, q.last_dt, q.delta_x))
            if not cast:
                continue
            eng.neighbors_build(); eng.isosurface_build(*lattice); eng.components_build()
            read = lambda: eng.neighbors_read() + eng.isosurface_read(pressure=True, velocity=True) + eng.components_read()      # noqa: E731 (a stale result refuses the read)
            held = read()
            on_demand = lambda: (eng.sample_grid(*lattice), eng.sample_points(pts), eng.sample_point_gradients(pts))      # noqa: E731
            before = on_demand()
            last = eng.cast_rays(o, d, te, step=step, mode="any")
            assert (last["status"] & 1).sum() > 10
            for x, y in zip(held, read()):
                assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
            assert len(held[1]) > 0 and len(held[2]) > 0 and held[6].max() >= 0
            for x, y in zip(before, on_demand()):
                assert list(x) == list(y) and all(x[k].tobytes() == y[k].tobytes() for k in x)
            _same(eng.cast_rays(o, d, te, step=step, mode="any"), last, "behind the other on-demand calls")
        runs.append((prog, eng.download(FIELDS), eng.probes_read()))
        if cast:
            want = eng.download()
            spec = {k: np.zeros_like(want[k]) for k in ("Position", "Velocity", "Acceleration", "Density", "Pressure", "ID", "Type", "GroupMarker", "GhostPoints", "Cells")}
            fbeg = eng._fn("download_begin"); fbeg.argtypes = [C.c_void_p] * 11
            eng._check(fbeg(eng._h, *[spec[k].ctypes.data_as(C.c_void_p) for k in spec]))
            mid = eng.cast_rays(o, d, te, step=step, mode="any")
            eng.advance(1e9, max_steps=3)
            eng.cast_rays(o, d, te, step=step, mode="any")
            eng.download_end()
            for k in spec:
                np.testing.assert_array_equal(spec[k], want[k], err_msg=k)
            _same(mid, last, "the call saw the state of before the three steps")
        eng.close()
    (pa, a, sa), (pb, b, sb) = runs
    assert pa == pb                                                                 # the progress blocks
    assert all(a[k].tobytes() == b[k].tobytes() for k in FIELDS)                    # the downloads
    assert len(sa["iteration"]) == sum(calls) and list(sa) == list(sb) and all(np.array_equal(sa[k], sb[k]) for k in sa)      # the probe series


def test_water_level_on_the_still_column(request):
    """At t = 0 the 2-D column stands still: one step in, the level at gauges across it is the fixture's fill height within dp."""
    p, s = request.getfixturevalue("dam_break_2d")
    eng = _engine(p, s, 8)
    eng.advance(1e9, max_steps=1)
    lo, hi = _fluid_box(p)
    dp = s.SimConstants.dx
    x = np.linspace(lo[0] + 3 * dp, hi[0] - 3 * dp, 9)
    eta = rays.water_level(eng, x, top=hi[1] + 5 * eng.cfg.H, bottom=lo[1])
    print(f"fill height {hi[1]:.4f} + dp/2, levels {eta.min():.4f} … {eta.max():.4f}, dp {dp}")
    assert np.isfinite(eta).all() and np.abs(eta - (hi[1] + 0.5 * dp)).max() <= dp
    dry = rays.water_level(eng, [hi[0] + 10 * eng.cfg.H], top=hi[1] + 5 * eng.cfg.H, bottom=hi[1] + eng.cfg.H)
    assert np.isnan(dry).all()
    eng.close()


def test_depth_image(request):
    """A 16 × 16 image of the 3-D column seen from above against the restatement."""
    eng, p, s = _start("dam_break_3d_shipped", 4, request)
    lo, hi = _fluid_box(p)
    H = eng.cfg.H
    origin = np.array([lo[0] - H, lo[1] - H, hi[2] + 4 * H])
    u = np.array([(hi[0] - lo[0] + 2 * H) / 15, 0.0, 0.0])
    v = np.array([0.0, (hi[1] - lo[1] + 2 * H) / 15, 0.0])
    t_end, step = hi[2] - lo[2] + 5 * H, 0.5 * eng.cfg.h
    img = rays.depth_image(eng, origin, u, v, (16, 16), [0.0, 0.0, -1.0], t_end, step=step)
    o = rays.pixel_origins(origin, u, v, (16, 16))
    want = rays.restate(_evaluator(eng), o, np.tile([0.0, 0.0, -1.0], (256, 1)), 0.0, t_end, step, 0.5, "enter")
    assert img["t"].shape == (16, 16) and img["point"].shape == (16, 16, 3)
    assert np.array_equal(img["t"].reshape(-1), want["bracket"][:, 1], equal_nan=True)
    assert np.array_equal(img["point"].reshape(-1, 3), want["point"], equal_nan=True)
    hit = np.isfinite(img["t"])
    assert 30 < hit.sum() < 256 and np.isnan(img["point"][~hit]).all()
    assert o[17].tolist() == (origin + 1.0 * u + 1.0 * v).tolist()
    eng.close()
