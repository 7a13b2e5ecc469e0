"""Cases, one-step reference and per-particle bound shared by tests/test_fused_pair_scale_host.py and tests/test_fused_pair_parity_gpu.py.

Everything here is the reference side: numpy + KD-tree pair sums (tests/bruteforce.py, which shares no code with the oracle or the kernels)
put through the step formulas of src/SPHCellList.jl:742-802 in fp64.  Nothing here looks at what the engine computes.

ONE FUSED STEP from a state (x, v, ρ, a) with Δt of src/TimeStepping.jl:24-46 exposes the four pair sums of the two passes:
    predictor   dρ/dt₁, a₁ on (x, v, ρ, P(ρ));   ρ⁺ = limit(ρ + dρ/dt₁·Δt/2), v⁺ = v + (a₁ + g)·Δt/2·ML, x⁺ = x + v·Δt/2·ML
    corrector   dρ/dt₂, a₂ on (x⁺, v⁺, ρ⁺, P(ρ⁺)), model terms on ρ;   ε = −dρ/dt₂/ρ⁺·Δt
    Acceleration = a₂ + g        Velocity = v + Acceleration·Δt·ML        Density = limit(ρ)·(2 − ε)/(2 + ε)
    Pressure = P(ρ⁺)             Position = x + (Velocity − Acceleration·Δt·ML/2)·Δt·ML

THE SCALE S_i of a compared field is the rounding scale of the pair sums behind it (bruteforce.pair_forces: Σ_j |term_ij|·(2⁻²⁴ + …/r),
with u = 2⁻²⁴) propagated through that formula, plus ONE fp32 rounding of what the epilogue of k_neighbor_force
(sphexample_amd/csrc/sphmi_kernels.h, `PASS_PREDICTOR` / corrector branch) holds in fp32 on the way to that field:
    Acceleration_d   S₂(a_d)                                  + u·|Acceleration_d|        (accbuf is fp32)
    Velocity_d       Δt·ML·S₂(a_d)                            + u·|Velocity_d|            (pk1 is fp32)
    Density          κ·Δt·S₂(dρ/dt), κ = 4/(2+ε)²·limit(ρ)/ρ⁺  + u·|Density − limit(ρ)|    (ε is formed in fp32; ρ itself is delivered as record + low word)
    Pressure         P'(ρ⁺)·(Δt/2·S₁(dρ/dt)                   + u·ρ⁺)                     (the half-step record holds ρ⁺ in fp32; P' = c₀²(ρ⁺/ρ₀)⁶)
    Position_d       ML·(Δt²/2·S₂(a_d)                        + u·|Position_d − x_d|)     (the increment is formed in fp32; x is record + low word)
A second step of the same handle starts from a state that already differs by the first step's error: Velocity, Density and Position carry
it on (S = S_first + S_second, Position also Δt·S_first(Velocity)); Acceleration and Pressure are formed anew.

THE CONSTANT in front of S_i is measured, reference against reference: the same pair formulas in numpy.float32 on the fp32-rounded neighbour
state with sequential fp32 accumulation, and the step formulas in fp32 behind them, give Q = max_i |sum32_i − sum64_i| / S_i over the four sums
of the step and, likewise, over the five fields.  A group of sizes that is ONE
case (the ragged sizes) shares the largest Q of its members — a lone particle has no pair and measures nothing.  The engine has to stay within
FACTOR·Q·S_i for every particle and field; FACTOR = 4 covers what the restatement does not model (summation order across two lanes and several
waves, FMA contraction, hardware reciprocal and square root at 1 ulp each)."""
import functools
from types import SimpleNamespace

import numpy as np
from scipy.spatial import cKDTree

import bruteforce as bf

U = bf.FP32_ULP
FACTOR = 4.0
FIELDS = ("Acceleration", "Velocity", "Density", "Pressure", "Position")
RAGGED_3D = (1, 31, 32, 33, 63, 64, 65, 97, 128, 129, 130, 257)
RAGGED_2D = (1, 63, 65, 130)
PER_CELL = 12.0                                  # particles per cell of the sparse clouds


def setup(dims):
    from sphexample_amd.cases import setup_dam_break_3d
    from test_oracle import default_2d_setup
    return setup_dam_break_3d(0.02) if dims == 3 else default_2d_setup()


def config(s, n):
    from sphexample_amd._abi import make_config
    return make_config(n, s.SimConstants, s.SimKernel, s.SimMetaData, s.SimViscosity, s.SimDensityDiffusion)


def _spaced(draw, n, dmin):
    """n points of draw(m), none closer than dmin to an EARLIER one (a pair at 1e-3·H would own its two particles' conditioning)."""
    pos = draw(n + n // 8 + 8)
    pos = pos.astype(np.float32).astype(np.float64)            # the distance that counts is the one of the fp32 state
    close = cKDTree(pos).query_pairs(dmin, output_type="ndarray")
    keep = np.ones(len(pos), bool)
    keep[close.max(1)] = False
    pos = pos[keep][:n]
    assert len(pos) == n
    return pos


def _particles(dims, s, pos, rng, per_cell, permute_ids=False):
    """Fluid / Fixed 80 / 20 (the sign of ρ·s in the records), ρ = 1000 + U(0, 3), |v| ~ 0.1·c₀ per component at PER_CELL particles per cell
    and less in proportion on a crowd, so that a step changes ρ by about as much (a crowd at full speed drives ρ through zero in one step).
    Position, Velocity and Density are fp32-exact."""
    from sphexample_amd import particles_from_arrays
    n = len(pos)
    ty = np.where(rng.random(n) < 0.8, 1, 2)
    ids = rng.permutation(n) + 1 if permute_ids else np.arange(1, n + 1)
    p = particles_from_arrays(dims, pos, 1000.0 + rng.uniform(0, 3, n), ty, ty, ids)
    vmax = 0.1 * s.SimConstants.c0 * min(1.0, PER_CELL / per_cell)
    p.Velocity[:] = rng.uniform(-vmax, vmax, size=(n, dims))
    for f in ("Position", "Velocity", "Density"):
        getattr(p, f)[...] = getattr(p, f).astype(np.float32).astype(np.float64)
    return p


def _box(rng, n, dims, H, origin=0.6):
    side = max(1.0, (n / PER_CELL) ** (1.0 / dims))
    return lambda m: rng.uniform(origin * H, (origin + side) * H, size=(m, dims))


# name → (dims, members); a member is (label, seed, builder).  Built lazily and once: the reference is shared by every test of a session.
def _members():
    out = {}

    def ragged(dims, n):
        def make():
            s = setup(dims); H = s.SimKernel.H; rng = np.random.default_rng(100 + n)
            return _particles(dims, s, _spaced(_box(rng, n, dims, H), n, 1e-3 * H), rng, PER_CELL), s
        return make

    def crowd(dims):
        def make():
            s = setup(dims); H = s.SimKernel.H; rng = np.random.default_rng(7)
            if dims == 3:       # two cells of one row: the own row is longer than the 256-record window, the queues fill inside a chunk row
                n, draw = 3000, lambda m: np.stack([rng.uniform(0.6 * H, 2.4 * H, m), rng.uniform(0.6 * H, 1.4 * H, m), rng.uniform(0.6 * H, 1.4 * H, m)], axis=1)
                per_cell = 1500.0
            else:               # three cells of one row (tests/test_engine_gpu.py, test_half_tiles_with_several_waves_per_half_on_crowds)
                n, draw = 2300, lambda m: np.stack([rng.uniform(0.0, 0.23, m), rng.uniform(0.041, 0.119, m)], axis=1)
                per_cell = 770.0
            return _particles(dims, s, _spaced(draw, n, 1e-3 * H), rng, per_cell), s
        return make

    def box(kind, shift=(0.0, 0.0, 0.0)):
        def make():
            s = setup(3); H = s.SimKernel.H; rng = np.random.default_rng(2024)
            n = 6000
            if kind == "clusters":              # two clusters 40 box-sides apart: empty stretches of the grid, chunk skipping
                n = 3000
                half = _box(rng, n // 2, 3, H)
                side = (n / 2 / PER_CELL) ** (1.0 / 3) * H

                def draw(m):
                    x = half(m); x[1::2, 0] += 40 * side
                    return x
            elif kind == "faces":               # a fifth of the points EXACTLY on x = (n ± ½)·H (the fuzz generator's rule)
                cloud = _box(rng, n, 3, H)

                def draw(m):
                    x = cloud(m); pick = rng.random(m) < 0.2
                    x[pick, 0] = np.round(x[pick, 0] / H) * H + 0.5 * H * rng.choice([1.0, -1.0], size=int(pick.sum()))
                    return x
            else:
                draw = _box(rng, n, 3, H)
            sh = np.asarray(shift)
            pos = _spaced(lambda m: draw(m) + sh, n, 1e-3 * H)
            return _particles(3, s, pos, rng, PER_CELL, permute_ids=True), s
        return make

    out["ragged3d"] = (3, [(f"n{n}", ragged(3, n)) for n in RAGGED_3D])
    out["crowd3d"] = (3, [("crowd", crowd(3))])
    out["box"] = (3, [("box", box("box"))])
    out["clusters"] = (3, [("clusters", box("clusters"))])
    out["faces"] = (3, [("faces", box("faces"))])
    out["offset"] = (3, [("offset", box("box", OFFSET_SHIFT))])
    out["ragged2d"] = (2, [(f"n{n}", ragged(2, n)) for n in RAGGED_2D])
    out["crowd2d"] = (2, [("crowd", crowd(2))])
    return out


OFFSET_SHIFT = (-13.7, 50.0, -13.7)
CASES = ("ragged3d", "crowd3d", "box", "clusters", "faces", "offset", "second_call", "ragged2d", "crowd2d")


def members(case):
    """[(label, make)] of a case; `second_call` is the box cloud (its second step is re-based on the oracle by the tests)."""
    return _members()["box" if case == "second_call" else case][1]


@functools.lru_cache(maxsize=None)
def particles(case, label):
    return dict(members(case))[label]()


def state_of(p, acceleration=None):
    """The state a step starts from, rows as they are; in-cell order after the rebuild that opens a call = row order (a stable sort)."""
    return SimpleNamespace(pos=np.array(p.Position, float), vel=np.array(p.Velocity, float), rho=np.array(p.Density, float),
                           acc=np.zeros_like(p.Position, dtype=float) if acceleration is None else np.array(acceleration, float),
                           ml=(np.asarray(p.Type) == 1).astype(float), gf=np.where(np.asarray(p.Type) == 1, -1.0, np.where(np.asarray(p.Type) == 3, 1.0, 0.0)))


def delta_t(cfg, st):
    """src/TimeStepping.jl:24-46."""
    visc = np.abs(cfg.h * (st.vel * st.pos).sum(1) / ((st.pos * st.pos).sum(1) + cfg.eta2)).max()
    with np.errstate(divide="ignore"):
        dt1 = np.sqrt(cfg.h / np.sqrt((st.acc * st.acc).sum(1))).min()
    return cfg.CFL * min(dt1, cfg.h / (cfg.c0 + visc))


def _limit(cfg, rho, ml):
    return np.where((rho < cfg.rho0) & (ml == 0.0), cfg.rho0, rho)


def _eos(cfg, rho, f):
    """EquationOfStateGamma7 (src/SimulationEquations.jl:9-11) in the type of f."""
    r = rho / f(cfg.rho0)
    r2 = r * r; r4 = r2 * r2
    return f((cfg.c0 ** 2 * cfg.rho0) / 7) * (r4 * r2 * r - f(1))


def step(cfg, st, dtype=np.float64):
    """One step of src/SPHCellList.jl:742-802 from `st` (rows in the order the call's rebuild sorts stably).  dtype = numpy.float32 forms the
    pair sums AND the step formulas in fp32, on the state rounded to fp32; only Position and Density keep their fp64 start value and add an
    increment formed in fp32, which is what an fp32 handle's record + low word hold.  Returns the five fields (fp64 arrays), the two pair-sum
    records (bruteforce.pair_forces, detail) and the pieces the scales need."""
    n, D = st.pos.shape
    key = bf._lex_key(bf.cell_of(st.pos, cfg.H_inv))
    order = np.empty(n, np.int64); order[np.argsort(key, kind="stable")] = np.arange(n)
    f = np.dtype(dtype).type
    dt64 = delta_t(cfg, st)
    dt, dt2 = f(dt64), f(0.5 * dt64)
    grav = np.zeros((n, D), dtype); grav[:, -1] = f(cfg.g) * st.gf.astype(dtype)
    ml = st.ml.astype(dtype)[:, None]
    x, v, rho = st.pos.astype(dtype), st.vel.astype(dtype), st.rho.astype(dtype)
    lim = lambda r: np.where((r < f(cfg.rho0)) & (st.ml == 0.0), f(cfg.rho0), r)
    p1 = bf.pair_forces(cfg, x, v, rho, rho, _eos(cfg, rho, f), st.ml, order, dtype=dtype, detail=True)
    a1 = p1.acc + grav
    pos_h, vel_h = x + v * dt2 * ml, v + a1 * dt2 * ml
    rho_h = lim(rho + p1.drho * dt2)
    press = _eos(cfg, rho_h, f)
    p2 = bf.pair_forces(cfg, pos_h, vel_h, rho_h, rho, press, st.ml, order, dtype=dtype, detail=True, cell_pos=st.pos)
    a2 = p2.acc + grav
    eps = -(p2.drho / rho_h) * dt
    ad = a2 * dt * ml
    vel = v + ad
    inc = (((vel + (vel - ad)) / f(2)) * dt) * ml
    assert all(t.dtype == np.dtype(dtype) for t in (a1, pos_h, vel_h, rho_h, press, eps, vel, inc))
    rho_l = np.where((st.rho < cfg.rho0) & (st.ml == 0.0), cfg.rho0, st.rho)
    e = eps.astype(float)
    fields = {"Acceleration": a2.astype(float), "Velocity": vel.astype(float), "Density": rho_l * ((2 - e) / (2 + e)), "Pressure": press.astype(float),
              "Position": st.pos + inc.astype(float)}
    return SimpleNamespace(fields=fields, p1=p1, p2=p2, dt=dt64, rho_h=rho_h.astype(float), rho_l=rho_l, eps=e, ml=st.ml[:, None], x0=st.pos)


def _propagate(cfg, r, s1_drho, s2_drho, s2_acc):
    """Per-field image of a change of the pair sums (first order; the same map serves the rounding scales and a removed pair's terms)."""
    dt = r.dt
    kappa = 4.0 / (2.0 + r.eps) ** 2 * r.rho_l / r.rho_h
    return {"Acceleration": s2_acc, "Velocity": dt * r.ml * s2_acc, "Density": kappa * dt * s2_drho,
            "Pressure": cfg.c0 ** 2 * (r.rho_h / cfg.rho0) ** 6 * (0.5 * dt) * s1_drho, "Position": r.ml * (0.5 * dt * dt) * s2_acc}


def scales(cfg, r):
    """S_i of every field for the fp64 step record `r` (module docstring)."""
    f = r.fields
    S = _propagate(cfg, r, r.p1.scale_drho, r.p2.scale_drho, r.p2.scale_acc)
    S["Acceleration"] = S["Acceleration"] + U * np.abs(f["Acceleration"])
    S["Velocity"] = S["Velocity"] + U * np.abs(f["Velocity"])
    S["Density"] = S["Density"] + U * np.abs(f["Density"] - r.rho_l)
    S["Pressure"] = S["Pressure"] + cfg.c0 ** 2 * (r.rho_h / cfg.rho0) ** 6 * U * r.rho_h
    S["Position"] = S["Position"] + r.ml * U * np.abs(f["Position"] - r.x0)
    return S


def carried(S1, S2, dt2):
    """Scales after a second step of the same handle (module docstring)."""
    return {"Acceleration": S2["Acceleration"], "Pressure": S2["Pressure"], "Velocity": S1["Velocity"] + S2["Velocity"],
            "Density": S1["Density"] + S2["Density"], "Position": S1["Position"] + dt2 * S1["Velocity"] + S2["Position"]}


def measure_q(r64, r32, S):
    """Q of one step: the fp32 restatement against the fp64 one, over the four pair sums in units of their rounding scales and over the five
    fields in units of S (a field held in fp32 is off by its own rounding whatever its pair sums do: that belongs to the constant too)."""
    q = 0.0
    terms = [(x, y, s) for a, b in ((r64.p1, r32.p1), (r64.p2, r32.p2)) for x, y, s in ((a.drho, b.drho, a.scale_drho), (a.acc, b.acc, a.scale_acc))]
    terms += [(r64.fields[k], r32.fields[k], S[k] * np.ones_like(r64.fields[k])) for k in FIELDS]
    for x, y, s in terms:
        err = np.abs(y.astype(float) - x)
        assert (err[s == 0] == 0).all()
        if (s > 0).any():
            q = max(q, float((err[s > 0] / s[s > 0]).max()))
    return q


def visibility(cfg, r, S, q_case):
    """Which pairs a kernel could not lose unseen: a pair dropped from the PREDICTOR's sums shows in Pressure, one dropped from the CORRECTOR's in
    the other four fields (first order: what the lost half-step terms do to the corrector's other pairs is left out, which only hides pairs).
    Returns (q of the predictor's pairs, seen if lost in the predictor, seen if lost in the corrector, seen if lost in both): seen = at least one
    partner leaves FACTOR·Q·S_i in at least one field.  (A pair that enters the support only in the half step counts with the predictor's list
    as not seen by the corrector.)"""
    n = len(S["Density"])
    bound = {k: FACTOR * q_case * v for k, v in S.items()}

    def seen(pair, side_fields, pred):
        out = np.zeros(pair.npairs, bool)
        for rows, td, ta in ((pair.i, pair.t_drho_i, pair.t_acc), (pair.j, pair.t_drho_j, -pair.t_acc)):
            sub = SimpleNamespace(dt=r.dt, eps=r.eps[rows], rho_l=r.rho_l[rows], rho_h=r.rho_h[rows], ml=r.ml[rows])
            z = np.zeros_like(td)
            eff = _propagate(cfg, sub, td if pred else z, z if pred else td, np.zeros_like(ta) if pred else ta)
            for k in side_fields:
                e, b = np.abs(eff[k]), bound[k][rows]
                out |= (e > b) if e.ndim == 1 else (e > b).any(1)
        return out
    s1, s2 = seen(r.p1, ("Pressure",), True), seen(r.p2, ("Acceleration", "Velocity", "Density", "Position"), False)
    key = lambda p: np.minimum(p.i, p.j) * n + np.maximum(p.i, p.j)
    k1, k2 = key(r.p1), key(r.p2)
    o2 = np.argsort(k2)
    at = np.clip(np.searchsorted(k2[o2], k1), 0, max(len(k2) - 1, 0))
    s2_on_1 = (k2[o2][at] == k1) & s2[o2][at] if len(k2) else np.zeros(len(k1), bool)
    return r.p1.q, s1, s2_on_1, s1 | s2_on_1


@functools.lru_cache(maxsize=None)
def first_step(case, label):
    """(cfg, fp64 step record, S, Q of this member) of the step from a member's initial state."""
    p, s = particles(case, label)
    cfg = config(s, len(p))
    st = state_of(p)
    r64, r32 = step(cfg, st), step(cfg, st, np.float32)
    S = scales(cfg, r64)
    return cfg, r64, S, measure_q(r64, r32, S)


@functools.lru_cache(maxsize=None)
def case_q(case):
    """Q of a case from its first steps (the second call adds its own second step: tests)."""
    return max(first_step(case, label)[3] for label, _ in members(case))


def by_id(st):
    order = np.argsort(st["ID"], kind="stable")
    return {k: v[order] for k, v in st.items()}


def rebased_step(cfg, orc):
    """The NEXT step of an oracle handle, restated from the oracle's own state (rows in the oracle's order: the rebuild that opens the call sorts
    them stably): (fp64 step record with the oracle's rows and their `ids`, S by ID, Q, fields by ID)."""
    o = orc.download(("ID", "Position", "Velocity", "Acceleration", "Density", "Type"))
    st = state_of(SimpleNamespace(Position=o["Position"], Velocity=o["Velocity"], Density=o["Density"], Type=o["Type"]), o["Acceleration"])
    r64, r32 = step(cfg, st), step(cfg, st, np.float32)
    S = scales(cfg, r64)
    q = measure_q(r64, r32, S)
    r64.ids = o["ID"]
    back = np.argsort(o["ID"], kind="stable")
    return r64, {k: v[back] for k, v in S.items()}, q, {k: v[back] for k, v in r64.fields.items()}
