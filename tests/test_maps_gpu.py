"""Per-bin maps of crest, arrival and mean flow accumulated on the device at every step (sphmi_maps_enable / sphmi_maps_read /
sphmi_maps_disable, csrc/sphmi_maps.h) — needs a real MI355X.

Every comparison is against downloads of the SAME handle and has NO tolerance: after every executed step the test downloads Position,
Velocity and Type and runs `sphexample_amd.maps.update` — the table of the header, term for term, in float64 and int64 — and at the
end the twelve arrays, the window and the map of the last step equal the host's bit for bit (compared as int64 views).  The handles
take float64 host arrays, so a download delivers the device values widened (fp32 handles: record + low word), which is what the kernel
bins.  The step's values are integer sums and extremes, so no row order, wave or workgroup seam can change a bit: the one-bin and the
seam cases put every atomic on the same few addresses and run boundaries on wave and workgroup boundaries."""
import numpy as np
import pytest

from conftest import perturbed
from sphexample_amd import maps
from sphexample_amd._abi import ERR_ARGUMENT, ERR_STATE, SphmiError

pytestmark = pytest.mark.gpu

INF = np.inf
KEYS = ("steps", "t_begin", "t_end", "duration") + maps.FIELDS + maps.LAST


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _engine(p, s, fb, **kw):
    from sphexample_amd.engine import make_engine
    return make_engine(p, s, device_float_bytes=fb, **kw)


def _same(got, want, label):
    assert tuple(got) == KEYS and tuple(want) == KEYS, label
    for k in KEYS:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape, (label, k, a.shape, b.shape)
        if a.dtype == np.int64 or k == "steps":
            bad = np.nonzero((a != b).reshape(-1))[0]
        else:
            bad = np.nonzero(_bits(a).reshape(-1) != _bits(b).reshape(-1))[0]
        print(f"{label} {k}: {len(bad)} of {a.size} values differ" + (f", first at {bad[0]}: device {a.reshape(-1)[bad[0]]!r} host {b.reshape(-1)[bad[0]]!r}" if len(bad) else ""))
        assert len(bad) == 0, (label, k)


class Host:
    """The host restatement next to a handle."""

    def __init__(self, eng, lat, t_begin=0.0):
        self.eng, self.lat = eng, lat
        self.state = maps.start(lat, t_begin)

    def step(self):
        """one executed step on the device, then the same step on the host from the download behind it"""
        pr = self.eng.advance(1e9, max_steps=1)
        assert pr.steps_done == 1
        d = self.eng.download(("Position", "Velocity", "Type", "ID"))
        maps.update(self.state, self.lat, d["Position"], d["Velocity"], d["Type"] == 1, pr.total_time, pr.last_dt)
        return pr, d

    def check(self, label):
        r = self.eng.maps_read()
        _same(r, maps.result(self.state), label)
        wet = r["t_arrival"] < INF
        assert (r["wet"][wet] > 0).all() and (r["wet"] <= r["duration"]).all() and (r["top_max"][wet] >= r["bottom_min"][wet]).all()
        return r


def _along_x(p, speed=2.0):
    q = p.copy()
    q.Velocity[q.Type == 1, 0] = speed
    return q


def _enable(eng, lat):
    eng.maps_enable(lat["origin"], lat["spacing"], lat["counts"], lat["up_axis"])


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fb", [8, 4])
def test_restatement_2d_column_map(dam_break_2d, fb):
    """6 881 rows (no multiple of 256 or 64), the fluid at 2 m/s along x: 24 single steps move it about 3 mm, across the 1 mm columns
    of a map that is narrower than the tank and whose origin lies exactly on a particle's coordinate.  sphmi_download_permutation
    after steps 8 and 16 changes nothing: nothing here is keyed by row."""
    p0, s = dam_break_2d
    assert len(p0) == 6881
    p = _along_x(p0)
    xs = np.unique(p.Position[p.Type == 1, 0])
    origin_x = float(xs[len(xs) // 4])                                  # a particle's own coordinate: the fluid left of it lies outside
    width = 0.001
    nx = int((xs[-1] - origin_x) / 2 / width)                            # … and so does the right half of what remains
    assert nx >= 64
    lat = maps.lattice([origin_x, 0.0], [width, INF], [nx, 1], 1)
    assert (maps.bin_index(lat, p.Position[p.Type == 1]) == 0).any()     # at the upload a row sits exactly on the lower face, inside
    eng = _engine(p, s, fb)
    _enable(eng, lat)
    host = Host(eng, lat)
    first, t_first = None, None
    for step in range(1, 25):
        pr, d = host.step()
        if step == 1:
            t_first = pr.total_time
            first = dict(zip(d["ID"].tolist(), maps.bin_index(lat, d["Position"]).tolist()))
        if step in (8, 16):
            eng.download_permutation()
    r = host.check(f"2-D column map fp{8 * fb}")
    assert r["steps"] == 24 and r["t_begin"] == 0.0 and r["t_end"] == pr.total_time
    last = maps.bin_index(lat, d["Position"])
    fluid = d["Type"] == 1
    moved = sum(1 for i, b, f in zip(d["ID"].tolist(), last.tolist(), fluid.tolist()) if f and b >= 0 and first[i] >= 0 and first[i] != b)
    late = int(((r["t_arrival"] > t_first) & (r["t_arrival"] < INF)).sum())
    outside = int((fluid & (last < 0)).sum())
    print(f"fp{8 * fb}: {moved} rows changed their bin, {late} of {nx} bins got wet after the first step, {outside} fluid rows outside the lattice")
    assert moved > 0 and late > 0 and outside > 0
    assert int(r["last_n"].sum()) == int((fluid & (last >= 0)).sum())
    assert (r["flux"][:, 0][r["t_arrival"] < INF] > 0).all() and not r["flux"][:, 2].any()        # 2-D: the third axis is an exact zero
    eng.close()


# 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["floor map, up = z", "full lattice, up = x"])
def test_restatement_3d(dam_break_3d_shipped, kind):
    p0, s = dam_break_3d_shipped
    p = perturbed(p0, seed=3, vel_scale=1.0)
    assert len(p) == 17446
    f = p.Position[p.Type == 1]
    lo, hi = f.min(axis=0), f.max(axis=0)
    if kind.startswith("floor"):
        sp = 0.04
        counts = [int(np.ceil((hi[0] - lo[0]) / sp)) + 1, int(np.ceil((hi[1] - lo[1]) / sp)) + 1, 1]
        lat = maps.lattice([lo[0] - 0.01, lo[1] - 0.01, 0.0], [sp, sp, INF], counts, 2)
    else:
        sp = np.array([0.03, 0.035, 0.025])
        counts = np.maximum(((hi - lo) * 0.8 / sp).astype(int), 2)      # a part of the fluid: rows lie outside on every axis
        lat = maps.lattice(lo + 0.1 * (hi - lo), sp, counts, 0)
    eng = _engine(p, s, 4)
    _enable(eng, lat)
    host = Host(eng, lat)
    for _ in range(8):
        pr, d = host.step()
    r = host.check(kind)
    assert r["steps"] == 8
    inside = maps.bin_index(lat, d["Position"]) >= 0
    fluid = d["Type"] == 1
    assert int(r["last_n"].sum()) == int((fluid & inside).sum()) > 0
    assert r["flux"][:, 2].any() and (d["Velocity"][fluid, 2] != 0).all()          # vz took part
    wet = r["last_n"] > 0
    up = lat["up_axis"]
    assert r["last_top"][wet].max() == d["Position"][fluid & inside, up].max()      # the extremes are those of the up axis, not of another
    assert r["last_bottom"][wet].min() == d["Position"][fluid & inside, up].min()
    if not kind.startswith("floor"):
        assert (fluid & ~inside).any()
    eng.close()


# 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["dam_break_2d", "dam_break_3d_shipped"])
def test_one_bin(case, request):
    """counts all 1, every spacing +inf: every counting row of every wave and workgroup lands on the same six addresses."""
    p0, s = request.getfixturevalue(case)
    p = perturbed(p0, seed=5, vel_scale=1.0)
    D = p.Position.shape[1]
    lat = maps.lattice([0.0] * D, [INF] * D, [1] * D, D - 1)
    eng = _engine(p, s, 4)
    _enable(eng, lat)
    host = Host(eng, lat)
    for _ in range(4):
        pr, d = host.step()
    r = host.check(f"one bin, {case}")
    n_fluid = int((d["Type"] == 1).sum())
    assert r["last_n"][0] == n_fluid and r["n_max"][0] == float(n_fluid) and r["fill"][0] > 0
    assert r["last_top"][0] == d["Position"][d["Type"] == 1, D - 1].max() and r["last_bottom"][0] == d["Position"][d["Type"] == 1, D - 1].min()
    eng.close()


def _line(s, n=1024, dp=0.02):
    """n fluid rows in a line along x, uploaded in x order, and three Fixed rows behind its far end: the cell order is the x order, so
    rows 64·k … 64·k + 63 are neighbours in space — a wave — and rows 256·k … a workgroup"""
    from sphexample_amd import particles_from_arrays
    x = np.arange(n + 3) * dp
    pos = np.stack([x, np.full(n + 3, 0.5)], axis=1)
    pos[n:, 0] += 4 * dp
    rng = np.random.default_rng(7)
    ty = np.array([1] * n + [2] * 3, dtype=np.uint8)
    q = particles_from_arrays(2, pos, np.full(n + 3, s.SimConstants.rho0), ty, ty.astype(np.int64), np.arange(n + 3) + 1)
    q.Velocity[:n] = rng.normal(0.0, 0.05, (n, 2))
    return q


@pytest.mark.parametrize("rows_per_bin", [64, 256, 96])
def test_runs_that_end_on_wave_and_workgroup_seams(dam_break_2d, rows_per_bin):
    """Bins that hold 64 and 256 consecutive rows — every run of equal bins ends exactly where a wave or a workgroup ends — and 96, where
    runs straddle the seams.  The test asserts the layout from the downloads."""
    _, s = dam_break_2d
    n, dp = 1024, 0.02
    p = _line(s, n, dp)
    nb = -(-n // rows_per_bin)
    lat = maps.lattice([-0.5 * dp, 0.0], [rows_per_bin * dp, INF], [nb, 1], 1)
    eng = _engine(p, s, 4)
    _enable(eng, lat)
    host = Host(eng, lat)
    for _ in range(3):
        pr, d = host.step()
        assert (d["Type"][:n] == 1).all()
        np.testing.assert_array_equal(maps.bin_index(lat, d["Position"])[:n], np.arange(n) // rows_per_bin)      # row order = x order
    r = host.check(f"{rows_per_bin} rows per bin")
    np.testing.assert_array_equal(r["last_n"], np.bincount(np.arange(n) // rows_per_bin))
    eng.close()


# 4 ---------------------------------------------------------------------------------------------------------------------
def test_inside_a_batch(dam_break_2d):
    """One sphmi_advance of 64 steps with Δx-triggered rebuilds inside.  A handle that makes 64 single steps instead is NOT the same
    run — every sphmi_advance opens with a rebuild, the rows change their order and with it the order of the neighbour sums, and the
    two handles' states differ in their last bits (and the maps alter no state: test_no_side_effects) — so the batch is restated from what the other observers
    recorded at every step of the SAME batch: sixteen control boxes that are the sixteen columns of the map (origin 0 and a spacing
    that is a power of two: `lo + k·s <= x < lo + (k + 1)·s` and `floor((x − lo) / s) == k` are the same rule exactly) give n per
    step and column, hence t_arrival, wet, fill, n_max and the last step's n bit for bit; the budgets' extent of the fluid gives the
    highest crest and the lowest bottom of all columns.  header.steps equals the executed steps: the steps the batch queued beyond its
    64th were cancelled and left no trace."""
    p0, s = dam_break_2d
    p = perturbed(p0, seed=3, vel_scale=6.0)                # (Δx-triggered rebuilds within the first 60 of these steps)
    width, nb = 2.0 ** -3, 16
    x = p.Position[p.Type == 1, 0]
    assert 0.0 <= x.min() and x.max() < nb * width and len(np.unique(np.floor(x / width))) >= 3
    lat = maps.lattice([0.0, 0.0], [width, INF], [nb, 1], 1)
    eng = _engine(p, s, 4)
    _enable(eng, lat)
    eng.budgets_enable(capacity=256)
    eng.flow_enable([[k * width, -INF] for k in range(nb)], [[(k + 1) * width, INF] for k in range(nb)], capacity=256)
    pr0 = eng.advance(0.0, max_steps=0)
    pr = eng.advance(1e9, max_steps=64)
    assert pr.steps_done == 64
    rebuilds = pr.n_rebuilds - pr0.n_rebuilds
    print(f"rebuilds inside the batch: {rebuilds}")
    assert rebuilds >= 2
    r, fl, bg = eng.maps_read(), eng.flow_read(), eng.budgets_read()
    assert r["steps"] == 64 == len(fl["time"]) == len(bg["time"])
    t_arrival, wet, fill, n_max, duration = np.full(nb, INF), np.zeros(nb), np.zeros(nb), np.zeros(nb), np.float64(0.0)
    for k in range(64):
        n, t, dt = fl["count"][k].astype(np.float64), fl["time"][k], fl["dt"][k]
        some = n > 0
        t_arrival[some & (t_arrival == INF)] = t
        wet[some] = (wet + dt)[some]
        fill[some] = (fill + n * dt)[some]
        n_max = np.maximum(n_max, n)
        duration = duration + dt
    for key, want in (("t_arrival", t_arrival), ("wet", wet), ("fill", fill), ("n_max", n_max), ("duration", [duration]), ("t_end", [fl["time"][-1]])):
        assert (_bits(r[key]) == _bits(want)).all(), key
    np.testing.assert_array_equal(r["last_n"], fl["count"][-1])
    assert int(r["last_n"].sum()) == int(bg["count"][-1]) and (fl["count"] > 0).any(axis=0).sum() >= 3 and (fl["count"][0] != fl["count"][-1]).any()
    box = bg["box"].reshape(64, 6)                           # min x, y, z, max x, y, z of the fluid at every step
    assert r["top_max"].max() == box[:, 4].max() and r["bottom_min"].min() == box[:, 1].min()
    assert r["last_top"].max() == box[-1, 4] and r["last_bottom"].min() == box[-1, 1]
    assert np.isin(r["t_top_max"][r["t_arrival"] < INF], fl["time"]).all() and r["t_end"] == pr.total_time
    eng.close()


# 5 ---------------------------------------------------------------------------------------------------------------------
def test_no_side_effects(dam_break_2d):
    p0, s = dam_break_2d
    p = perturbed(p0, seed=3, vel_scale=6.0)
    every = ("Position", "Velocity", "Acceleration", "Density", "Pressure", "Type", "ID", "GroupMarker")
    lat = maps.lattice([0.0, 0.0], [0.02, 0.02], [60, 40], 1)
    got = {}
    for name in ("with", "without"):
        eng = _engine(p, s, 4)
        eng.budgets_enable(capacity=256)
        eng.flow_enable([[0.1, -INF]], [[0.6, INF]], capacity=256)
        eng.envelopes_enable(("Fluid",))
        if name == "with":
            _enable(eng, lat)
        assert eng.advance(1e9, max_steps=40).steps_done == 40
        got[name] = (eng.download(every), eng.budgets_read(), eng.flow_read(), eng.envelopes_read())
        if name == "with":
            r = eng.maps_read()
            assert r["steps"] == 40 and (r["t_arrival"] < INF).any()
        eng.close()
    for x, y in zip(got["with"], got["without"]):
        assert list(x) == list(y)
        for key in x:
            assert np.asarray(x[key]).tobytes() == np.asarray(y[key]).tobytes(), key


# 6 ---------------------------------------------------------------------------------------------------------------------
def _status(call):
    with pytest.raises(SphmiError) as e:
        call()
    return e.value.status


def test_contract(dam_break_2d):
    from sphexample_amd._abi import make_config
    from sphexample_amd.engine import Engine
    p0, s = dam_break_2d
    p = _along_x(p0)
    cfg = make_config(len(p), s.SimConstants, s.SimKernel, s.SimMetaData, s.SimViscosity, s.SimDensityDiffusion, device_float_bytes=4,
                      host_float_bytes=8, device=0)
    good = ([0.0, 0.0], [0.05, INF], [40, 1], 1)
    bare = Engine(cfg)
    assert bare.has_maps()
    assert _status(lambda: bare.maps_enable(*good)) == ERR_STATE                         # before the upload
    assert _status(bare.maps_read) == ERR_STATE
    bare.upload_particles(p)
    assert _status(bare.maps_read) == ERR_STATE                                          # read before enable
    for bad in (([0.0, 0.0], [0.05, 0.05], [1 << 10, (1 << 10) + 1], 1),                 # a bin product above the limit
                ([0.0, 0.0], [0.0, INF], [40, 1], 1), ([0.0, 0.0], [-0.05, INF], [40, 1], 1), ([0.0, 0.0], [np.nan, INF], [40, 1], 1),
                ([0.0, 0.0], [0.05, INF], [40, 2], 1),                                   # +inf spacing with a count above 1
                ([0.0, INF], [0.05, INF], [40, 1], 1), ([np.nan, 0.0], [0.05, INF], [40, 1], 1),
                ([0.0, 0.0], [0.05, INF], [0, 1], 1),
                ([0.0, 0.0], [0.05, INF], [40, 1], 2), ([0.0, 0.0], [0.05, INF], [40, 1], -1)):
        assert _status(lambda: bare.maps_enable(*bad)) == ERR_ARGUMENT, bad
    assert _status(bare.maps_read) == ERR_STATE                                          # … and a refused enable enables nothing
    bare.maps_enable(*good)
    r = bare.maps_read()
    assert r["steps"] == 0 and r["duration"] == 0.0 and (r["t_arrival"] == INF).all() and (r["top_max"] == -INF).all() and not r["last_n"].any()
    bare.maps_enable([0.0, 0.0], [0.05, 0.05], [1 << 10, 1 << 10], 0)                    # exactly SPHMI_MAX_MAP_BINS
    assert bare.maps_read()["top_max"].shape == (1 << 20,)
    bare.upload_particles(p)                                                             # sphmi_upload disables
    assert _status(bare.maps_read) == ERR_STATE
    bare.maps_enable(*good)
    bare.maps_disable()
    assert _status(bare.maps_read) == ERR_STATE
    bare.maps_disable()                                                                  # (twice is fine)
    bare.close()
    multi = _engine(p, s, 4, devices=[0, 0])
    assert _status(lambda: multi.maps_enable(*good)) == ERR_STATE
    assert _status(multi.maps_read) == ERR_STATE
    assert "single-device" in str(pytest.raises(SphmiError, multi.maps_disable).value)
    multi.close()

    eng = _engine(p, s, 4)
    lat = maps.lattice(*good)
    pr = eng.advance(1e9, max_steps=5)                                                   # enabling mid-run sees only later steps
    _enable(eng, lat)
    host = Host(eng, lat, t_begin=pr.total_time)
    for _ in range(4):
        host.step()
    before = host.check("mid-run")
    assert before["steps"] == 4 and before["t_begin"] == pr.total_time
    after = eng.maps_read()                                                              # read twice: the same bytes, nothing was cleared
    for key in before:
        assert np.asarray(before[key]).tobytes() == np.asarray(after[key]).tobytes(), key
    eng.forces_once()                                                                    # records nothing
    after = eng.maps_read()
    for key in before:
        assert np.asarray(before[key]).tobytes() == np.asarray(after[key]).tobytes(), key
    now = eng.advance(0.0, max_steps=0).total_time                                       # a second enable restarts the records
    lat2 = maps.lattice([0.0, 0.0], [0.05, 0.1], [40, 6], 0)
    _enable(eng, lat2)
    r = eng.maps_read()
    assert r["steps"] == 0 and r["t_begin"] == now and r["top_max"].shape == (240,) and (r["t_arrival"] == INF).all()
    host = Host(eng, lat2, t_begin=now)
    for _ in range(3):
        host.step()
    assert host.check("restarted")["steps"] == 3
    eng.close()
