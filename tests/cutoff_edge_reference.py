"""Layouts with pairs PLANTED on the cut r = H of a kernel that has not vanished there (H = k·h, k < 2), their reference sums and the quantities
tests/test_cutoff_edge_host.py and tests/test_cutoff_edge_gpu.py accept by.  Reference side only: numpy, a KD-tree, tests/bruteforce.py and the
step restatement of tests/fused_pair_reference.py.  Nothing here looks at what the engine computes.

Phase 1 of k_neighbor_force (sphexample_amd/csrc/sphmi_kernels.h) forms |c − t|² − H²(1 + ε) in tile-local coordinates on the matrix cores, in fp32
or in hi + lo fp16 halves, and ε is a hand-derived error bound that grows with the REACH of the tile.  A short ε drops a pair just inside H before
the exact cut of the pair loop sees it.  With k = 2 the pair's term vanishes there and nobody notices; with k = 1.5 it does not.

EVERY PAIR of a layout is exactly one of
    planted inside    r²/H² = 1 − δ        planted outside   r²/H² = 1 + δ        clear   |r²/H² − 1| ≥ c
with r² evaluated in fp64 on the positions as they are uploaded (rounded to fp32 first for an fp32 handle).  "=" is to PLANT_TOL·δ: the
coordinates live on a grid, and the smallest δ of a layout is 8 × what that grid can move r² by (below), so 1/16 is half a grid step there.

δ of an fp64 handle: the decades DECADES, without those below 8 × the fp64 rounding of r² at the layout's largest coordinate (2·√D·2⁻⁵³·max|x|/H:
only the 1 000 H spray loses 1e-12).  The positions are random doubles, never fp32-representable: the mask rounds local coordinates to fp32.
δ of an fp32 handle: the relative error of r² that tests/bruteforce.py itself attributes to fp32 is e = 2·√D·delta/H with
delta = TILE_ROUNDING·H + FP32_ULP·max|x| (the formula of bruteforce.pair_forces, at the layout's largest coordinate); the smallest δ is 8·e, above
it the same decades; c ≥ 100·e, and ≥ 2e-3 for the boxes.  Derived from that model, not measured.

LAYOUTS (all k = 1.5; the 3-D box also k = √2):
    box        ≈ 3 000 random points at fused_pair_reference.PER_CELL per cell, pruned until no pair is nearer the cut than c, then satellites
               at r² = H²(1 ∓ δ) of random anchors — random directions, axis-aligned ones (other components EXACTLY equal), ones that cross a cell
               face in x (own row) and in the other axes (another row) — each accepted only if all its other distances are clear.  Rows and ids permuted.
    clusters   two such boxes 40 box-sides apart in x: the rows of the sort alternate between them, tiles and half tiles straddle both.
    spray_x/y/z  isolated stars (a centre, satellites at r² = H²(1 ∓ δ) on a randomly rotated octahedron / square: ≥ √2·H from each other) strung
               along the axis at a spacing L ≥ 3.1·H per member; members aim at tile reaches ≈ 9 H (where the fp16 scale leaves 16/H), ≈ 100 H and
               ≈ 1 000 H.  A tile holds 64 particles of ≥ 10 stars, so ONE string at L ≥ 3.1·H cannot reach less than ≈ 25 H: the near member is a
               bundle of 3 × 3 strings along the LAST axis (the most significant one of the sort: a tile is then one or two layers of nine stars),
               in 2-D three strings of octagon stars (eight satellites, neighbours 0.77 H and 1.41 H apart) — the same near member in every spray.
    stale      dropped: see stale_report().

The sort (bruteforce.cell_of, _lex_key) is restated in tiles(): tiles of 64 and half tiles of 32 of the sorted order, and the reach of each —
the largest distance from the tile's first particle, in units of H."""
import dataclasses
import functools
import math
from types import SimpleNamespace

import numpy as np
from scipy.spatial import cKDTree

import bruteforce as bf
import fused_pair_reference as fr

K_EDGE = 1.5
K_SQRT2 = math.sqrt(2.0)
DECADES = (1e-12, 1e-9, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2)
PLANT_TOL = 1.0 / 16.0
PER_BAND = 24                    # satellites per (δ, side) of a box and of a spray member
C_BOX = 2e-3
VISIBLE = 10.0                   # a planted pair moves a compared quantity by at least this many tolerances
FP64_BAR = 1e-10                 # × the field's maximum: the project's bar for fp64 handles
SPRAY_REACH = ((6.0, 12.0), (50.0, 200.0), (500.0, 2000.0))
LAYOUTS_3D = ("box", "box_sqrt2", "clusters", "spray_x", "spray_y", "spray_z")
LAYOUTS_2D = ("box2d", "spray2d_x", "spray2d_y")
LAYOUTS = LAYOUTS_3D + LAYOUTS_2D


def dims_of(name):
    return 2 if "2d" in name else 3


def setup(dims, k, viscosity=None, kernel_output=False):
    """fused_pair_reference.setup with the kernel instance replaced the way test_cutoff_other_than_2h does it (dx, k)."""
    import sphexample_amd.config as cfgm
    s = fr.setup(dims)
    s = dataclasses.replace(s, SimKernel=cfgm.SPHKernelInstance(dims, cfgm.WendlandC2(), dx=s.SimConstants.dx, k=k))
    if viscosity == "Laminar":
        consts = cfgm.SimulationConstants(**{a: getattr(s.SimConstants, a) for a in ("rho0", "dx", "m0", "alpha", "g", "c0", "gamma", "delta_phi", "CFL")},
                                          nu0=1e-3)                 # (large enough to matter: tests/test_engine_gpu.py, test_model_variants)
        s = dataclasses.replace(s, SimConstants=consts, SimViscosity=cfgm.Laminar())
    if kernel_output:
        s = dataclasses.replace(s, SimMetaData=dataclasses.replace(s.SimMetaData, KMode=cfgm.StoreKernelOutput))
    return s


# ---- the error model and the δ list -----------------------------------------------------------------------------------------------------------
def r2_error(width, D, H, xmax):
    """Relative error of r² at r = H that the coordinates' format allows: fp32 by the model of bruteforce.pair_forces, fp64 by one rounding."""
    delta = bf.TILE_ROUNDING * H + bf.FP32_ULP * xmax if width == 4 else 2.0 ** -53 * xmax
    return 2.0 * math.sqrt(D) * delta / H


def delta_list(width, D, H, xmax):
    e = r2_error(width, D, H, xmax)
    if width == 8:
        return tuple(d for d in DECADES if d >= 8 * e)
    return (8 * e,) + tuple(d for d in DECADES if d > 8 * e)


def _as_uploaded(x, width):
    return x.astype(np.float32).astype(np.float64) if width == 4 else np.asarray(x, float)


def _ratio(a, b, H):
    d = a - b
    return float((d * d).sum() / (H * H))


def _plant(anchor, u, H, target, width, tol):
    """A point at r²/H² = target from `anchor` in direction u, on the grid of the upload format; None where the grid has no such point.
    (Components of u that are exactly 0 stay exactly equal to the anchor's.)"""
    d = H * math.sqrt(target)
    for _ in range(6):
        x = _as_uploaded(anchor + d * u, width)
        x[u == 0.0] = anchor[u == 0.0]
        got = _ratio(x, anchor, H)
        if abs(got - target) <= tol:
            return x
        d *= math.sqrt(target / got)
    return None


def _bands(deltas):
    return [(d, side) for d in deltas for side in (-1, +1)]            # −1: inside (r² = H²(1 − δ)), +1: outside


# ---- the box -------------------------------------------------------------------------------------------------------------------------------------
def _pruned(pos, H, c, dmin):
    """Greedy: drop the later point of every pair that is nearer the cut than c (or nearer than dmin), until none is left."""
    while True:
        pr = cKDTree(pos).query_pairs(H * math.sqrt(1 + c), output_type="ndarray")
        d = pos[pr[:, 0]] - pos[pr[:, 1]]
        q = (d * d).sum(1) / (H * H)
        bad = pr[(np.abs(q - 1) < c) | (q < (dmin / H) ** 2)]
        if not len(bad):
            return pos
        keep = np.ones(len(pos), bool)
        for a, b in bad:                                   # the later point goes, unless its partner is gone already
            if keep[a] and keep[b]:
                keep[max(a, b)] = False
        pos = pos[keep]


def _directions(rng, D, H, anchor, kind):
    """kind 0: random; 1: along one axis; 2: random, across the anchor's cell face in x (own row); 3: across a face of another axis; 4: inside the cell."""
    if kind == 1:
        u = np.zeros(D); u[rng.integers(D)] = rng.choice([-1.0, 1.0])
        return u
    for _ in range(200):
        u = rng.normal(size=D); u /= np.linalg.norm(u)
        if kind == 0:
            return u
        ca, cs = bf.cell_of(anchor[None], 1 / H)[0], bf.cell_of((anchor + H * u)[None], 1 / H)[0]
        if kind == 2 and cs[0] != ca[0] and (cs[1:] == ca[1:]).all():
            return u
        if kind == 3 and (cs[1:] != ca[1:]).any():
            return u
        if kind == 4 and (cs == ca).all():
            return u
    return None


def _add_satellites(rng, pos, H, D, c, deltas, width, per_band, anchors=None):
    """Satellites at r²/H² = 1 ∓ δ of random anchors of `pos`; returns (positions, planted [(a, b, δ, side)])."""
    pos = [x for x in pos]
    n0 = len(pos)
    anchors = np.arange(n0) if anchors is None else anchors
    used = set()
    planted = []
    for delta, side in _bands(deltas):
        got = tries = 0
        while got < per_band:
            tries += 1
            assert tries < 4000, ("no room for satellites", delta, side)
            a = int(rng.choice(anchors))
            if a in used:
                continue
            u = _directions(rng, D, H, pos[a], (got + tries) % 5)
            if u is None:
                continue
            x = _plant(pos[a], u, H, 1 + side * delta, width, PLANT_TOL * delta)
            if x is None:
                continue
            arr = np.asarray(pos)
            dd = arr - x
            q = (dd * dd).sum(1) / (H * H)
            q[a] = 9.0
            if (np.abs(q - 1) < c).any() or (q < 1e-6).any():
                continue
            used.add(a)
            planted.append((a, len(pos), delta, side))
            pos.append(x)
            got += 1
    return np.asarray(pos), planted


def _state(dims, s, pos, rng):
    """fused_pair_reference._particles, without its rounding of the POSITIONS (an fp64 handle's are not fp32-representable; an fp32 handle's were
    rounded before the distances were taken).  ρ = 1000 + U(0, 3) and P(ρ) > 0, |v| random: pressure and continuity terms of a pair are non-zero
    (the host test holds every planted pair to that)."""
    keep = np.array(pos, float)
    p = fr._particles(dims, s, pos, rng, fr.PER_CELL, permute_ids=True)
    p.Position[...] = keep
    return p


def _box_positions(rng, n, D, H, width, c, x0=0.0):
    side = (n / fr.PER_CELL) ** (1.0 / D) * H
    pos = rng.uniform(0.6 * H, 0.6 * H + side, size=(n, D))
    pos[:, 0] += x0
    return _pruned(_as_uploaded(pos, width), H, c, 1e-3 * H), side


def _build_box(name, width):
    D = dims_of(name)
    k = K_SQRT2 if name == "box_sqrt2" else K_EDGE
    s = setup(D, k); H = s.SimKernel.H
    rng = np.random.default_rng(31 + D)
    n = 3000
    if name == "clusters":
        side = (n / 2 / fr.PER_CELL) ** (1.0 / D) * H
        xmax = 41 * side + 1.6 * H
    else:
        xmax = (n / fr.PER_CELL) ** (1.0 / D) * H + 0.6 * H + H
    e = r2_error(width, D, H, xmax)
    c = max(C_BOX, 100 * e)
    deltas = delta_list(width, D, H, xmax)
    if name == "clusters":
        a, side = _box_positions(rng, n // 2, D, H, width, c)
        b, _ = _box_positions(rng, n // 2, D, H, width, c, x0=40 * side)
        pos = np.concatenate([a, b])
        info = dict(side=side)
    else:
        pos, side = _box_positions(rng, n, D, H, width, c)
        info = dict(side=side)
    pos, planted = _add_satellites(rng, pos, H, D, c, deltas, width, PER_BAND)
    assert np.abs(pos).max() <= xmax
    return _finish(name, width, s, pos, planted, deltas, c, e, rng, info)


# ---- the sprays ----------------------------------------------------------------------------------------------------------------------------------
def _rotation(rng, D):
    q, r = np.linalg.qr(rng.normal(size=(D, D)))
    return q * np.sign(np.diag(r))


def _star(rng, centre, H, D, bands, width, octagon=False):
    """A centre and its satellites: the vertices of a randomly rotated octahedron / square (2-D near member: octagon), each at its own 1 ∓ δ."""
    if octagon:
        t0 = rng.uniform(0, 2 * math.pi)
        dirs = np.array([[math.cos(t0 + i * math.pi / 4), math.sin(t0 + i * math.pi / 4)] for i in range(8)])
    else:
        R = _rotation(rng, D)
        dirs = np.concatenate([R.T, -R.T])
    centre = _as_uploaded(centre, width)
    out, plant = [centre], []
    for u, (delta, side) in zip(dirs, bands):
        for _ in range(50):
            x = _plant(centre, u, H, 1 + side * delta, width, PLANT_TOL * delta)
            if x is not None:
                break
            w = rng.normal(size=D) * 1e-3                  # the grid has no such point in this direction: turn it a little
            u = (u + w) / np.linalg.norm(u + w)
        assert x is not None
        plant.append((0, len(out), delta, side))
        out.append(x)
    return np.asarray(out), plant


def _spray_positions(rng, D, axis, H, width, deltas, spacing):
    """Three members along `axis`: the near bundle (along the LAST axis, see the module docstring) around the origin, the ≈ 100 H string on the
    positive side, the ≈ 1 000 H string on the negative side.  spacing = (L_mid, L_far) in units of H."""
    bands = _bands(deltas)
    per_star = 2 * D
    n_star = -(-PER_BAND * len(_bands(DECADES)) // per_star)              # the fp64 count for every width: ≥ 3 tiles per member
    pos, planted, member = [], [], []
    turn = [0]

    def add(centre, m, octagon=False):
        k = 8 if octagon else per_star
        b = [bands[(turn[0] + i) % len(bands)] for i in range(k)]
        turn[0] += k
        x, pl = _star(rng, centre, H, D, b, width, octagon)
        base = sum(len(t) for t in pos)
        planted.extend((base + a, base + s_, d, sd) for a, s_, d, sd in pl)
        pos.append(x); member.extend([m] * len(x))

    other = [d for d in range(D) if d != axis]
    base = np.full(D, 5.0 * H)                                               # the centre of cell 5 on the transverse axes: three cells wide
    # near: 3 × 3 strings (2-D: 3 strings of octagon stars) along the last axis
    L = 3.1 * H
    if D == 3:
        for kz in range(-(-n_star // 9)):
            for ky in range(3):
                for kx in range(3):
                    add(base + np.array([kx, ky, kz]) * L, 0)
    else:
        for ky in range(-(-PER_BAND * len(_bands(DECADES)) // 8 // 3)):
            for kx in range(3):
                add(base + np.array([kx, ky]) * L, 0, octagon=True)
    near_top = max(t[:, axis].max() for t in pos)
    for m, (sign, Lm) in enumerate(((+1, spacing[0]), (-1, spacing[1])), start=1):
        start = near_top + 40 * H if sign > 0 else -40 * H
        for i in range(n_star):
            ctr = base.copy()
            if axis != D - 1:
                ctr[D - 1] += 12.0 * m * H                          # members on rows of their own: the sort is most significant in the last axis
            ctr[axis] = start + sign * i * Lm * H
            ctr[other] += rng.uniform(-0.3, 0.3, size=len(other)) * H
            add(ctr, m)
    return np.concatenate(pos), planted, np.asarray(member)


def _tile_reach_of_members(pos, member, H):
    t = tiles(pos, H, 64)
    mem_sorted = member[t.order]
    out = {}
    for m in range(3):
        pure = [i for i, (a, b) in enumerate(t.ranges) if (mem_sorted[a:b] == m).all()]
        out[m] = t.reach[pure]
    return out


def _build_spray(name, width):
    D = dims_of(name)
    axis = "xyz".index(name[-1])
    s = setup(D, K_EDGE); H = s.SimKernel.H
    spacing = [100.0 / 9, 1000.0 / 9]
    for it in range(8):                                                     # the spacing that puts the members' median tile reach at 100 H and 1 000 H
        rng = np.random.default_rng(77 + 10 * D + axis)
        n_star = -(-PER_BAND * len(_bands(DECADES)) // (2 * D))
        xmax = (n_star * spacing[1] + 60) * H
        e = r2_error(width, D, H, xmax)
        deltas = delta_list(width, D, H, xmax)
        pos, planted, member = _spray_positions(rng, D, axis, H, width, deltas, spacing)
        reach = _tile_reach_of_members(pos, member, H)
        want = (100.0, 1000.0)
        ok = True
        for m in (1, 2):                                                    # (rows hold different shares of a star: the tiles of a member differ in reach)
            full = reach[m][reach[m] > 0.2 * reach[m].max()]                # (not the last, partial tile of the sorted order)
            mid = math.sqrt(float(full.min()) * float(full.max()))
            if not 0.8 * want[m - 1] <= mid <= 1.25 * want[m - 1] and not (spacing[m - 1] == 3.1 and mid > want[m - 1]):
                spacing[m - 1] = max(3.1, spacing[m - 1] * want[m - 1] / mid); ok = False
        if ok:
            break
    c = max(0.05, 100 * e)
    assert len(pos) <= 4000 and np.abs(pos).max() <= xmax and min(spacing) >= 3.1
    return _finish(name, width, s, pos, planted, deltas, c, e, rng, dict(member=member, spacing=tuple(spacing)))


# ---- common ----------------------------------------------------------------------------------------------------------------------------------------
def tiles(pos, H, size):
    """The sort restated: order (sorted → row), rank (row → sorted), [a, b) of every tile of `size`, and each tile's reach in H."""
    key = bf._lex_key(bf.cell_of(pos, 1.0 / H))
    order = np.argsort(key, kind="stable")
    rank = np.empty(len(pos), np.int64); rank[order] = np.arange(len(pos))
    ranges = [(a, min(a + size, len(pos))) for a in range(0, len(pos), size)]
    sp = pos[order]
    reach = np.array([np.sqrt(((sp[a:b] - sp[a]) ** 2).sum(1)).max() / H for a, b in ranges])
    return SimpleNamespace(order=order, rank=rank, ranges=ranges, reach=reach, size=size, key=key)


def _finish(name, width, s, pos, planted, deltas, c, e, rng, info):
    D = pos.shape[1]
    # rows (= upload order, and ID − 1: particles_from_arrays keeps rows by ID) permuted: a satellite sorts before or after its anchor inside a cell
    perm = rng.permutation(len(pos))
    where = np.empty(len(pos), np.int64); where[perm] = np.arange(len(pos))
    pos = pos[perm]
    if "member" in info:
        info["member"] = info["member"][perm]
    p = _state(D, s, pos, rng)
    assert (np.asarray(p.ID) == np.arange(1, len(pos) + 1)).all()
    pl = SimpleNamespace(a=where[np.array([t[0] for t in planted])], b=where[np.array([t[1] for t in planted])],
                         delta=np.array([t[2] for t in planted]), side=np.array([t[3] for t in planted]))
    L = SimpleNamespace(name=name, width=width, dims=D, s=s, p=p, H=s.SimKernel.H, k=s.SimKernel.k, planted=pl, deltas=tuple(deltas), c=c, e=e,
                        info=info, pos=np.array(p.Position, float), redrawn=0)
    # a planted pair whose loss would not show (velocities nearly across the pair, say) gets its satellite's velocity drawn again
    # … and so does a Fluid particle of a pair that the half step leaves within the fp32 error of r² of the cut: at x⁺ the corrector of an fp32
    # handle would decide such a pair by rounding, whatever the mask does
    vmax = 0.1 * s.SimConstants.c0
    fluid = np.asarray(p.Type) == 1
    for _ in range(60):
        v = _visible_of(_forces_of(L))
        bad = np.unique(pl.b[v < 1.5 * VISIBLE])                             # (1.5: the tolerances move a little with every draw)
        ha, hb, _ = _near_cut_at_half_step(L)
        bad = np.union1d(bad, np.where(fluid[hb], hb, ha))
        if not len(bad):
            break
        L.redrawn += len(bad)
        p.Velocity[bad] = rng.uniform(-vmax, vmax, size=(len(bad), D)).astype(np.float32).astype(np.float64)
    else:
        raise AssertionError(f"{name}: the state could not be drawn")
    return L


@functools.lru_cache(maxsize=None)
def layout(name, width):
    """The layout `name` for handles of `width` bytes per float (rows in upload order; planted.a / .b are rows)."""
    return (_build_spray if name.startswith("spray") else _build_box)(name, width)


def classify(L):
    """Every pair nearer the cut than c: (rows a, b, r²/H²), from a KD-tree and fp64 differences of the uploaded positions."""
    pr = cKDTree(L.pos).query_pairs(L.H * math.sqrt(1 + L.c) * (1 + 1e-12), output_type="ndarray")
    d = L.pos[pr[:, 0]] - L.pos[pr[:, 1]]
    q = (d * d).sum(1) / (L.H * L.H)
    near = np.abs(q - 1) < L.c
    return pr[near, 0], pr[near, 1], q[near]


def partner_class(L):
    """0 same cell, 1 x-adjacent cell of the own row, 2 another row — per planted pair."""
    cells = bf.cell_of(L.pos, 1.0 / L.H)
    ca, cb = cells[L.planted.a], cells[L.planted.b]
    same = (ca == cb).all(1)
    own_row = (ca[:, 1:] == cb[:, 1:]).all(1)
    return np.where(same, 0, np.where(own_row, 1, 2))


# ---- reference sums ------------------------------------------------------------------------------------------------------------------------------
class _Wider:
    """cfg with the support widened for the PAIR LIST only (cells, and with them the orientation, stay): the terms a planted outside pair would add."""
    def __init__(self, cfg, f2):
        self._c = cfg
        self.H2 = cfg.H2 * f2
        self.H = math.sqrt(self.H2)

    def __getattr__(self, k):
        return getattr(self._c, k)


def sorted_state(L):
    """The state forces_once() works on: rows in sorted order (a stable sort of the upload order), P = P(ρ)."""
    cfg = fr.config(L.s, len(L.pos))
    t = tiles(L.pos, L.H, 64)
    o = t.order
    st = SimpleNamespace(pos=L.pos[o], vel=np.array(L.p.Velocity, float)[o], rho=np.array(L.p.Density, float)[o],
                         ml=(np.asarray(L.p.Type)[o] == 1).astype(float), ids=np.asarray(L.p.ID)[o], order=o, rank=t.rank)
    st.press = bf.eos(cfg, st.rho)
    return cfg, st


@functools.lru_cache(maxsize=None)
def forces(name, width):
    return _forces_of(layout(name, width))


def _forces_of(L):
    """forces_once restated: the sums by ID, their rounding scales, Q (numpy.float32 against fp64 on this layout), the per-particle tolerance,
    and the signed terms of every planted pair (inside: what it contributes; outside: what it would)."""
    width = L.width
    cfg, st = sorted_state(L)
    args = (st.pos, st.vel, st.rho, st.rho, st.press, st.ml)
    r64 = bf.pair_forces(cfg, *args, detail=True)
    r32 = bf.pair_forces(cfg, *args, dtype=np.float32, detail=True)
    wide = bf.pair_forces(_Wider(cfg, 1 + 1.2 * max(L.deltas)), *args, detail=True)
    q = 0.0
    for x, y, sc in ((r64.drho, r32.drho, r64.scale_drho), (r64.acc, r32.acc, r64.scale_acc)):
        err = np.abs(y.astype(float) - x)
        assert (err[sc == 0] == 0).all()
        q = max(q, float((err[sc > 0] / sc[sc > 0]).max()))
    if width == 8:
        tol_d = np.full(len(st.pos), FP64_BAR * np.abs(r64.drho).max())
        tol_a = np.full(r64.acc.shape, FP64_BAR * np.abs(r64.acc).max())
    else:
        tol_d, tol_a = fr.FACTOR * q * r64.scale_drho, fr.FACTOR * q * r64.scale_acc
    # the planted pairs' terms, looked up in the wide list by (sorted row, sorted row)
    n = len(st.pos)
    ra, rb = st.rank[L.planted.a], st.rank[L.planted.b]
    key = np.minimum(wide.i, wide.j) * n + np.maximum(wide.i, wide.j)
    o = np.argsort(key)
    at = np.searchsorted(key[o], np.minimum(ra, rb) * n + np.maximum(ra, rb))
    assert (key[o][np.clip(at, 0, len(key) - 1)] == np.minimum(ra, rb) * n + np.maximum(ra, rb)).all(), "a planted pair is missing from the wide list"
    w = o[at]
    terms = SimpleNamespace(i=wide.i[w], j=wide.j[w], t_drho_i=wide.t_drho_i[w], t_drho_j=wide.t_drho_j[w], t_acc=wide.t_acc[w], q=wide.q[w])
    back = np.argsort(st.ids, kind="stable")
    return SimpleNamespace(cfg=cfg, st=st, r64=r64, q=q, tol_drho=tol_d, tol_acc=tol_a, terms=terms, back=back, npairs=r64.npairs,
                           inside_listed=np.isin(np.minimum(ra, rb) * n + np.maximum(ra, rb),
                                                 np.minimum(r64.i, r64.j) * n + np.maximum(r64.i, r64.j)))


def visible(name, width):
    """Per planted pair: the largest |term| / tolerance over drho and the components of acc of its two particles (forces_once quantities)."""
    return _visible_of(forces(name, width))


def _visible_of(f):
    t = f.terms
    out = np.zeros(len(t.i))
    for rows, td, ta in ((t.i, t.t_drho_i, t.t_acc), (t.j, t.t_drho_j, -t.t_acc)):
        for term, tol in ((np.abs(td), f.tol_drho[rows]), (np.abs(ta), f.tol_acc[rows])):
            with np.errstate(divide="ignore", invalid="ignore"):           # (a particle with no pair at all has tolerance 0: any term shows)
                ratio = np.where(tol > 0, term / tol, np.where(term > 0, np.inf, 0.0))
            out = np.maximum(out, ratio if ratio.ndim == 1 else ratio.max(1))
    return out


@functools.lru_cache(maxsize=None)
def one_step(name, width):
    """One fused step restated (fused_pair_reference.step) from the layout's initial state: (cfg, fp64 record, S, Q)."""
    L = layout(name, width)
    cfg = fr.config(L.s, len(L.pos))
    st = fr.state_of(L.p)
    r64 = fr.step(cfg, st)
    S = fr.scales(cfg, r64)
    q = fr.measure_q(r64, fr.step(cfg, st, np.float32), S) if width == 4 else float("nan")        # (an fp64 handle is held to FP64_BAR, not to Q)
    return cfg, r64, S, q


def half_step_near_cut(name, width):
    """(number of pairs of the CORRECTOR's positions x⁺ nearer the cut than the fp32 error e of r², e): the builder leaves none."""
    a, b, e = _near_cut_at_half_step(layout(name, width))
    return len(a), e


def _near_cut_at_half_step(L):
    """x⁺ = x + v·Δt/2·ML with Δt of the first step (no acceleration yet: the CFL term alone); pairs of two Fixed particles do not move and are
    planted or clear as before."""
    cfg = fr.config(L.s, len(L.pos))
    st = fr.state_of(L.p)
    xh = st.pos + st.vel * (0.5 * fr.delta_t(cfg, st)) * st.ml[:, None]
    e = r2_error(4, L.dims, L.H, float(np.abs(xh).max()))
    pr = cKDTree(xh).query_pairs(L.H * (1 + e), output_type="ndarray")
    d = xh[pr[:, 0]] - xh[pr[:, 1]]
    q = (d * d).sum(1) / (L.H * L.H)
    near = (np.abs(q - 1) < e) & ((st.ml[pr[:, 0]] > 0) | (st.ml[pr[:, 1]] > 0))
    return pr[near, 0], pr[near, 1], e


def stale_report(width=8):
    """The `stale` member — the box after one step — is dropped: one step moves a particle by |v|·Δt, and r² of a pair by 2·r·|Δv|·Δt, about the
    largest δ and many times c.  Returns (smallest move of r²/H² of a planted pair in units of PLANT_TOL·δ of that pair, pairs that are still
    planted in their band after the step, pairs nearer the cut than c after the step that nobody planted, median move)."""
    L = layout("box", width)
    x1 = one_step("box", width)[1].fields["Position"]
    P = L.planted
    d0, d1 = L.pos[P.a] - L.pos[P.b], x1[P.a] - x1[P.b]
    q0, q1 = (d0 * d0).sum(1) / (L.H * L.H), (d1 * d1).sum(1) / (L.H * L.H)
    still = int((np.abs(q1 - (1 + P.side * P.delta)) <= PLANT_TOL * P.delta).sum())
    after = SimpleNamespace(pos=x1, H=L.H, c=L.c)
    a, b, _ = classify(after)
    n = len(x1)
    strangers = int((~np.isin(np.minimum(a, b) * n + np.maximum(a, b), np.minimum(P.a, P.b) * n + np.maximum(P.a, P.b))).sum())
    return float((np.abs(q1 - q0) / (PLANT_TOL * P.delta)).min()), still, strangers, float(np.median(np.abs(q1 - q0)))


def describe(L, row):
    """The planted pairs of a row, for a failure message: δ, side, partner class and the reach of the row's tile and half tile."""
    t64, t32 = tiles(L.pos, L.H, 64), tiles(L.pos, L.H, 32)
    cls = partner_class(L)
    out = []
    for m in np.nonzero((L.planted.a == row) | (L.planted.b == row))[0]:
        out.append(f"planted {'inside' if L.planted.side[m] < 0 else 'outside'} pair rows ({L.planted.a[m]}, {L.planted.b[m]}) δ={L.planted.delta[m]:.3g} "
                   f"class={('same cell', 'own row', 'other row')[cls[m]]} tile reach {t64.reach[t64.rank[row] // 64]:.1f} H, half tile {t32.reach[t32.rank[row] // 32]:.1f} H")
    return out
