"""Per-particle pressure and speed envelopes accumulated on the device at every step (sphmi_envelopes_enable / sphmi_envelopes_read,
csrc/sphmi_envelopes.h) — needs a real MI355X.

Every comparison is against downloads of the SAME handle and has NO tolerance: after every executed step the test downloads
Pressure, Velocity, ID and Type and runs `sphexample_amd.envelopes.update` — the table of the header, term for term, in float64
with every product and sum rounded on its own — on arrays keyed by ID; at the end the eight arrays and the window of the device
equal the host's bit for bit (compared as int64 views).  The handles take float64 host arrays, so a download delivers the device
values widened, which is what the kernel accumulates.  The records never move while the sort permutes rows at every rebuild: the
restatement cases assert that rows DID move (a composition of the downloaded permutations that is not the identity), the batch
case that Δx-triggered rebuilds lay inside the window."""
import numpy as np
import pytest

from conftest import perturbed
from sphexample_amd import envelopes
from sphexample_amd._abi import ERR_ARGUMENT, ERR_STATE, SphmiError

pytestmark = pytest.mark.gpu

TYPE = {"Fluid": 1, "Fixed": 2, "Moving": 3}
FIELDS = ("Pressure", "Velocity", "ID", "Type")
START = {"p_max": -np.inf, "t_p_max": 0.0, "p_min": np.inf, "impulse": 0.0, "square": 0.0, "loaded": 0.0, "speed_max": 0.0, "t_arrival": np.inf}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _engine(p, s, fb, **kw):
    from sphexample_amd.engine import make_engine
    return make_engine(p, s, device_float_bytes=fb, **kw)


class Host:
    """The host restatement next to a handle: state keyed by ID (entry k belongs to the k-th smallest ID)."""

    def __init__(self, eng, types, t_begin=0.0):
        self.eng, self.types = eng, [TYPE[t] for t in types]
        self.ids = np.sort(eng.download(("ID",))["ID"])
        assert (np.diff(self.ids) > 0).all()
        self.state = envelopes.start(len(self.ids), t_begin)

    def key(self, ids):
        k = np.searchsorted(self.ids, ids)
        assert np.array_equal(self.ids[k], ids)
        return k

    def step(self):
        """one executed step on the device, then the same step on the host from the download behind it"""
        pr = self.eng.advance(1e9, max_steps=1)
        assert pr.steps_done == 1
        d = self.eng.download(FIELDS)
        k = self.key(d["ID"])
        n = len(k)
        P, V, sel = np.empty(n), np.empty((n, d["Velocity"].shape[1])), np.zeros(n, dtype=bool)
        P[k], V[k], sel[k] = d["Pressure"], d["Velocity"], np.isin(d["Type"], self.types)
        envelopes.update(self.state, sel, P, V, pr.total_time, pr.last_dt)
        return pr, d

    def check(self, label):
        """the device's read against the host's state, bit for bit; unselected rows hold the start record"""
        r = self.eng.envelopes_read()
        d = self.eng.download(("ID", "Type"))
        k = self.key(d["ID"])
        want = envelopes.result(self.state)
        for key in ("steps", "t_begin", "t_end", "duration"):
            assert _bits([r[key]])[0] == _bits([want[key]])[0], (label, key, r[key], want[key])
        sel = np.isin(d["Type"], self.types)
        assert sel.any(), label
        for f in envelopes.FIELDS:
            got, ref = _bits(r[f]), _bits(want[f][k])
            bad = np.nonzero(got != ref)[0]
            print(f"{label} {f}: {len(bad)} of {len(got)} rows differ" + (f", first row {bad[0]}: device {r[f][bad[0]]!r} host {want[f][k][bad[0]]!r}" if len(bad) else ""))
            assert len(bad) == 0, (label, f)
            assert (_bits(r[f][~sel]) == _bits([START[f]])[0]).all(), (label, f)
        assert not np.isnan(r["impulse"]).any()
        assert (r["p_max"][sel] >= r["p_min"][sel]).all() and (r["loaded"][sel] <= r["duration"]).all()
        return r, d


def _along_x(p, speed=2.0):
    q = p.copy()
    q.Velocity[q.Type == 1, 0] = speed
    return q


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fb", [8, 4])
def test_restatement_2d_across_permutations_and_columns(dam_break_2d, fb):
    """6 881 rows (no multiple of 256), the fluid at 2 m/s along x: 24 single steps, each behind the rebuild that opens its
    sphmi_advance; sphmi_download_permutation after steps 8 and 16 (the envelopes' map is composed, the epoch restarts), two
    columns attached after step 12 (a map of their own)."""
    p, s = dam_break_2d
    eng = _engine(_along_x(p), s, fb)
    eng.envelopes_enable(("Fluid", "Fixed"))
    host = Host(eng, ("Fluid", "Fixed"))
    perms, cols = [], None
    for step in range(1, 25):
        _, d = host.step()
        if step in (8, 16):
            perms.append(eng.download_permutation())
        if step == 12:
            cols = [np.ascontiguousarray(d["ID"] * 3 + 1), np.ascontiguousarray(d["ID"].astype(np.float32) * np.float32(0.5))]
            eng.attach_columns(cols)
    composed = perms[0][perms[1]]                   # the row at upload of every row after step 16
    moved = int((composed != np.arange(len(p))).sum())
    print(f"fp{8 * fb}: {moved} rows moved within the first 16 steps, {int((perms[1] != np.arange(len(p))).sum())} between steps 8 and 16")
    assert moved > 0 and (perms[1] != np.arange(len(p))).any()          # else the indirection was never exercised
    r, d = host.check(f"2-D fp{8 * fb}")
    assert r["steps"] == 24 and r["t_begin"] == 0.0
    fluid = d["Type"] == 1
    assert (r["speed_max"][fluid] > 0.0).all() and (r["speed_max"][d["Type"] == 2] == 0.0).all()
    outs = [np.zeros_like(c) for c in cols]
    eng.download_columns(outs)                      # the columns still deliver their particles
    np.testing.assert_array_equal(outs[0], d["ID"] * 3 + 1)
    np.testing.assert_array_equal(outs[1], d["ID"].astype(np.float32) * np.float32(0.5))
    eng.attach_columns([])                          # detaching them does not disturb the envelopes
    host.step()
    host.check(f"2-D fp{8 * fb}, columns detached")
    eng.close()


# 2 ---------------------------------------------------------------------------------------------------------------------
def _cloud(s):
    """67 rows, one wave plus three: an 8 x 8 lattice of fluid at the spacing of the 2-D layout, slightly compressed in places, and
    three Fixed rows next to it"""
    from sphexample_amd import particles_from_arrays
    dp = 0.02
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), indexing="ij"), axis=-1).reshape(-1, 2) * dp
    pos = np.concatenate([g, [[-dp, 0.0], [-dp, dp], [-dp, 2 * dp]]])
    rng = np.random.default_rng(11)
    rho = s.SimConstants.rho0 + rng.uniform(-2.0, 4.0, len(pos))
    ty = np.array([1] * 64 + [2] * 3, dtype=np.uint8)
    return particles_from_arrays(2, pos, rho, ty, ty.astype(np.int64), rng.permutation(len(pos)) + 1)


@pytest.mark.parametrize("case", ["dam_break_3d_shipped", "still_wedge", "moving_square", "cloud"])
def test_restatement_over_ten_steps(case, request):
    if case == "cloud":
        _, s = request.getfixturevalue("dam_break_2d")
        p, fb, types = _cloud(s), 4, ("Fluid",)
    else:
        p0, s = request.getfixturevalue(case)
        fb, types = {"dam_break_3d_shipped": (4, ("Fluid", "Fixed")), "still_wedge": (8, ("Fluid", "Fixed")), "moving_square": (8, ("Moving",))}[case]
        p = perturbed(p0, seed=3, vel_scale=1.0) if case == "dam_break_3d_shipped" else p0
        if hasattr(p0, "geometries"):
            p.geometries = p0.geometries
    assert len(p) == {"dam_break_3d_shipped": 17446, "still_wedge": 3027, "cloud": 67}.get(case, len(p))
    eng = _engine(p, s, fb)
    eng.envelopes_enable(types)
    host = Host(eng, types)
    for step in range(1, 11):
        host.step()
        if step == 5:
            eng.download_permutation()
    r, d = host.check(case)
    sel = np.isin(d["Type"], [TYPE[t] for t in types])
    assert r["steps"] == 10
    if case == "dam_break_3d_shipped":
        v = eng.download(("Velocity",))["Velocity"]
        assert (v[d["Type"] == 1, 2] != 0).all()                 # vz took part in |v|²
    if case == "still_wedge":
        assert (r["p_max"][d["Type"] == 2] != r["p_max"][d["Type"] == 2][0]).any()      # the boundary's pressures (mDBC) differ row by row
    if case == "moving_square":
        assert int(sel.sum()) > 0 and (r["speed_max"][sel] > 0).all()
    eng.close()


# 3 ---------------------------------------------------------------------------------------------------------------------
def test_inside_a_batch_next_to_budgets_and_group_forces(dam_break_2d):
    p0, s = dam_break_2d
    p = perturbed(p0, seed=3, vel_scale=6.0)                # (the CPU oracle rebuilds twice within the first 40 of these steps)
    with_env, without = _engine(p, s, 4), _engine(p, s, 4)
    every = ("Position", "Velocity", "Acceleration", "Density", "Pressure", "Type", "ID", "GroupMarker")
    got = {}
    for name, eng in (("with", with_env), ("without", without)):
        eng.budgets_enable(capacity=256)
        eng.group_forces_enable([1, 2], capacity=256)
        if name == "with":
            eng.envelopes_enable(("Fluid",))
        pr0 = eng.advance(0.0, max_steps=0)
        pr = eng.advance(1e9, max_steps=60)
        assert pr.steps_done == 60
        got[name] = (pr.n_rebuilds - pr0.n_rebuilds, eng.budgets_read(), eng.group_forces_read(), eng.download(every))
    rebuilds, b, _, d = got["with"]
    print(f"rebuilds inside the window: {rebuilds}")
    assert rebuilds >= 2
    r = with_env.envelopes_read()
    assert r["steps"] == len(b["time"]) == 60
    duration = np.float64(0.0)
    for dt in b["dt"]:
        duration = duration + dt
    assert _bits([r["duration"]])[0] == _bits([duration])[0]
    assert r["t_end"] == b["time"][-1] and r["t_begin"] == 0.0
    fluid = d["Type"] == 1
    assert _bits([r["speed_max"].max()])[0] == _bits([b["extremes"][:, 0].max()])[0]
    assert np.isin(r["t_p_max"][fluid], b["time"]).all()
    P = d["Pressure"].astype(np.float64)
    assert (r["p_min"][fluid] <= P[fluid]).all() and (P[fluid] <= r["p_max"][fluid]).all()
    assert (r["p_max"][~fluid] == -np.inf).all() and (r["t_arrival"][~fluid] == np.inf).all()
    # the observer changes nothing: a handle without it ends in the same bytes, and records the same series
    _, b2, f2, d2 = got["without"]
    for key in every:
        assert d[key].tobytes() == d2[key].tobytes(), key
    for key in b:
        assert b[key].tobytes() == b2[key].tobytes(), key
    for x, y in zip(got["with"][2], f2):
        assert x.tobytes() == y.tobytes()
    with_env.close(); without.close()


# 4 ---------------------------------------------------------------------------------------------------------------------
def _status(call):
    with pytest.raises(SphmiError) as e:
        call()
    return e.value.status


def test_contract(dam_break_2d):
    import ctypes as C
    from sphexample_amd._abi import make_config
    from sphexample_amd.engine import Engine
    p0, s = dam_break_2d
    p = _along_x(p0)
    cfg = make_config(len(p), s.SimConstants, s.SimKernel, s.SimMetaData, s.SimViscosity, s.SimDensityDiffusion, device_float_bytes=4,
                      host_float_bytes=8, device=0)
    bare = Engine(cfg)
    assert bare.has_envelopes()
    assert _status(lambda: bare.envelopes_enable(("Fluid",))) == ERR_STATE               # before the upload
    assert _status(bare.envelopes_read) == ERR_STATE
    bare.upload_particles(p)
    assert _status(bare.envelopes_read) == ERR_STATE                                     # disabled
    f = bare._fn("envelopes_enable")
    f.argtypes = [C.c_void_p, C.c_uint32]
    assert f(bare._h, 1 << 4) == ERR_ARGUMENT and f(bare._h, 1) == ERR_ARGUMENT and f(bare._h, (1 << 1) | (1 << 31)) == ERR_ARGUMENT
    assert _status(bare.envelopes_read) == ERR_STATE                                     # … and a refused enable enables nothing
    bare.envelopes_enable(("Fluid",))
    assert bare.envelopes_read()["steps"] == 0
    bare.upload_particles(p)                                                             # sphmi_upload disables
    assert _status(bare.envelopes_read) == ERR_STATE
    bare.envelopes_enable(("Fluid",))
    bare.envelopes_enable(())                                                            # mask 0 disables
    assert _status(bare.envelopes_read) == ERR_STATE
    bare.close()
    multi = _engine(p, s, 4, devices=[0, 0])
    assert _status(lambda: multi.envelopes_enable(("Fluid",))) == ERR_STATE
    assert _status(multi.envelopes_read) == ERR_STATE
    multi.close()

    eng = _engine(p, s, 4)
    pr = eng.advance(1e9, max_steps=5)                                                   # enabling mid-run sees only later steps
    eng.envelopes_enable(("Fluid",))
    host = Host(eng, ("Fluid",), t_begin=pr.total_time)
    r = eng.envelopes_read()
    assert r["steps"] == 0 and r["t_begin"] == r["t_end"] == pr.total_time and r["duration"] == 0.0
    for key, v in START.items():
        assert (_bits(r[key]) == _bits([v])[0]).all(), key
    for _ in range(4):
        host.step()
    before, d = host.check("mid-run")
    assert before["steps"] == 4 and before["t_begin"] == pr.total_time
    # the on-demand builds leave the envelopes untouched …
    eng.particle_fields()
    eng.components()
    eng.neighbor_list()
    after = eng.envelopes_read()
    for key in before:
        assert np.asarray(before[key]).tobytes() == np.asarray(after[key]).tobytes(), key
    # … and so does sphmi_forces_once, whose rebuild may permute the rows: every particle keeps its record
    eng.forces_once()
    before, after = envelopes.by_id(before, d["ID"]), envelopes.by_id(eng.envelopes_read(), eng.download(("ID",))["ID"])
    for key in before:
        assert np.asarray(before[key]).tobytes() == np.asarray(after[key]).tobytes(), key
    # a second enable restarts: start records, steps = 0, t_begin = the TotalTime now
    now = eng.advance(0.0, max_steps=0).total_time
    eng.envelopes_enable(("Fluid", "Fixed"))
    r = eng.envelopes_read()
    assert r["steps"] == 0 and r["t_begin"] == now and r["duration"] == 0.0
    for key, v in START.items():
        assert (_bits(r[key]) == _bits([v])[0]).all(), key
    host = Host(eng, ("Fluid", "Fixed"), t_begin=now)
    for _ in range(3):
        host.step()
    ids = eng.download(("ID",))["ID"]
    keyed = envelopes.by_id(host.check("restarted")[0], ids)
    assert (np.diff(keyed["id"]) > 0).all() and keyed["steps"] == 3
    eng.close()
