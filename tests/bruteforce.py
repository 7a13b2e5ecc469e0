"""Independent numpy/scipy pair enumeration used to pin the oracle (and, on the GPU box, the engine).

It shares no code with oracle/sph_oracle.c: pairs come from a KD-tree over the positions (valid right
after a cell-list rebuild, when {adjacent cells ∧ r ≤ H} == {r ≤ H}), the physics
is written in vector form from the formulas of /root/reference/src/SPHCellList.jl:273-309,
src/SPHKernels.jl:85-86, src/SPHViscosityModels.jl:64-70, src/SPHDensityDiffusionModels.jl:116-133.
"""
from types import SimpleNamespace

import numpy as np
from scipy.spatial import cKDTree


def cell_of(x, H_inv):
    return (np.sign(x) * np.trunc(np.abs(x) * H_inv + 0.5)).astype(np.int64)


def _lex_key(cells):
    """Total order of CartesianIndex: last axis most significant."""
    D = cells.shape[1]
    c = cells - cells.min(0)
    span = c.max(0) + 1
    key = np.zeros(len(c), dtype=np.int64)
    mult = 1
    for d in range(D):
        key += c[:, d] * mult
        mult *= int(span[d])
    return key


FP32_ULP = 2.0 ** -24          # one fp32 rounding, relative
TILE_ROUNDING = 8 * 6e-8       # × H / r: a coordinate difference formed tile-relative and rounded once (tests/test_fuzz_gpu.py)


def pair_forces(cfg, pos, vel, rho, rho_n, press, ml, order_index=None, dtype=np.float64, detail=False, cell_pos=None):
    """Returns (drhodt, acc, number of pairs) for the state given in *sorted* particle order.

    order_index: position of each particle in the reference's sorted order (defaults to arange) — only
    used for the i/j orientation of the density-diffusion term (quirk Q4).  cell_pos: the positions the cell list was built
    from, where they are not `pos` (the corrector runs on x⁺ with the cells of x: the orientation follows the cells).

    dtype: np.float32 evaluates the SAME formulas on the state rounded to fp32, every intermediate in fp32, the sums
    accumulated sequentially in fp32 (np.add.at is unbuffered and in pair order).  The pair list itself is the fp64 one.

    detail=True returns a namespace instead: the signed sums (drho, acc), the pair list (i, j, q, r), the signed pair terms
    (t_drho_i, t_drho_j: what the pair adds to dρ/dt of i and of j; t_acc: what it adds to the acceleration of i, −t_acc to j),
    the absolute sums abs_drho / abs_acc and the rounding scales scale_drho / scale_acc, always in fp64.  A pair's ABSOLUTE
    term is its term with every operand that is one fp32 rounding of the state (what a neighbour record holds:
    sphexample_amd/csrc/sphmi_kernels.h, pk0 = {x, ρ·s}, pk1 = {v, P}) entering with its magnitude instead of cancelling:
      continuity   ρᵢ (m₀/ρⱼ) Σ_d (|vᵢ| + |vⱼ|)_d |∇W_d|                       (vᵢ − vⱼ: two rounded velocities)
      diffusion    δᵩ h c₀ (m₀/ρⁿⱼ) 2 (|ρⁿⱼ − ρⁿᵢ| + |ρᴴ|) |x·∇W| / (r² + η²)      (ρⁿ is the step's exact start state)
      pressure     m₀ (|Pᵢ| + |Pⱼ| + c₀² (ρᵢ + ρⱼ)) / (ρᵢ ρⱼ) |∇W_d|           (P comes from a rounded ρ: c₀²·ρ·2⁻²⁴, not |P|·2⁻²⁴)
      viscosity    m₀ α c₀ h Σ_e (|vᵢ| + |vⱼ|)_e |x_e| / (r² + η²) / ρ̄ |∇W_d|    (only where the signed v·x < 0)
    Its rounding scale is that term with |∇W_d| = |F|·|x_d| replaced by 2⁻²⁴·|F|·|x_d| + δ·(|F| + |F'|·|x_d|), δ = 8·H·6e-8 + 2⁻²⁴·max_d(|xᵢ| + |xⱼ|)_d:
    one rounding of the operands, and a coordinate difference that is off by δ — the kernels form it tile-relative and round it once, and the
    records hold ABSOLUTE coordinates rounded once (what makes a cloud far from the origin coarse).  That is the term times (2⁻²⁴ + c·H/r) for
    a pair in general position; written per component it also holds for pairs with x_d = 0 exactly (particles on one cell face), whose
    ∇W_d is off by δ·|F| all the same.  scale_* are the per-particle sums of those."""
    N, D = pos.shape
    if order_index is None:
        order_index = np.arange(N)
    tree = cKDTree(pos)
    pairs = tree.query_pairs(cfg.H * (1 + 1e-9), output_type="ndarray")
    a, b = pairs[:, 0], pairs[:, 1]
    x = pos[a] - pos[b]
    r2 = (x * x).sum(1)
    keep = r2 <= cfg.H2
    a, b, x, r2 = a[keep], b[keep], x[keep], r2[keep]
    # orientation: "i" = lower sorted index inside a cell, the particle of the LATER cell otherwise
    cells = cell_of(pos if cell_pos is None else cell_pos, cfg.H_inv)
    key = _lex_key(cells)
    same = key[a] == key[b]
    a_is_i = np.where(same, order_index[a] < order_index[b], key[a] > key[b])
    i = np.where(a_is_i, a, b)
    j = np.where(a_is_i, b, a)
    r64 = np.sqrt(r2)
    q64 = np.clip(r64 * cfg.h_inv, 0.0, 2.0)
    f = np.dtype(dtype).type
    pos, vel, rho, rho_n, press, ml = (np.asarray(v).astype(dtype) for v in (pos, vel, rho, rho_n, press, ml))
    xij = pos[i] - pos[j]
    r2 = (xij * xij).sum(1)
    q = np.clip(np.sqrt(r2) * f(cfg.h_inv), f(0), f(2))
    fac = f(cfg.alphaD) * f(5) * (q - f(2)) ** 3 / (f(8) * f(cfg.h) * f(cfg.h))
    gW = fac[:, None] * xij
    vij = vel[i] - vel[j]
    sym = -(vij * gW).sum(1)
    t_drho_i = -rho[i] * (f(cfg.m0) / rho[j]) * sym
    t_drho_j = -rho[j] * (f(cfg.m0) / rho[i]) * sym
    linear = cfg.density_diffusion == 2
    if linear:
        rhoH = f(cfg.rho0) * f(-cfg.g) * -xij[:, -1] * ((f(1) / (f(cfg.Cb) * f(cfg.gamma))) * f(cfg.rho0))
        psi = f(2) * ((rho_n[j] - rho_n[i]) - rhoH)[:, None] * (-xij) / (r2 + f(cfg.eta2))[:, None]
        Di = f(cfg.delta_phi) * f(cfg.h) * f(cfg.c0) * (f(cfg.m0) / rho_n[j]) * (psi * gW).sum(1) * ml[i] * ml[j]
        t_drho_i = t_drho_i + Di
        t_drho_j = t_drho_j - Di
    drho = np.zeros(N, dtype=dtype)
    acc = np.zeros((N, D), dtype=dtype)
    np.add.at(drho, i, t_drho_i)
    np.add.at(drho, j, t_drho_j)
    Pfac = (press[i] + press[j]) / (rho[i] * rho[j])
    um = f(-cfg.m0) * Pfac[:, None] * gW
    artificial = cfg.viscosity == 1
    if artificial:
        vdx = (vij * xij).sum(1)
        mu = f(cfg.h) * vdx / (r2 + f(cfg.eta2))
        rbar = f(0.5) * (rho_n[i] + rho_n[j])
        k = np.where(vdx < 0, f(-cfg.m0) * (f(-cfg.alpha) * f(cfg.c0) * mu) / rbar, f(0))
        um = um + k[:, None] * gW
    np.add.at(acc, i, um)
    np.add.at(acc, j, -um)
    assert drho.dtype == acc.dtype == np.dtype(dtype)
    if not detail:
        return drho, acc, len(a)
    # the absolute terms, in fp64 whatever dtype the sums were formed in
    pos, vel, rho, rho_n, press, ml = (v.astype(np.float64) for v in (pos, vel, rho, rho_n, press, ml))
    xij = pos[i] - pos[j]
    ax = np.abs(xij)
    r2 = (xij * xij).sum(1)
    afac = np.abs(cfg.alphaD * 5 * (q64 - 2) ** 3 / (8 * cfg.h * cfg.h))                 # |F|,  ∇W = F(q)·x
    adfac = np.abs(cfg.alphaD * 15 * (q64 - 2) ** 2 / (8 * cfg.h * cfg.h)) * cfg.h_inv   # |dF/dr|
    xabs = (np.abs(pos[i]) + np.abs(pos[j])).max(1)
    delta = TILE_ROUNDING * cfg.H + FP32_ULP * xabs                                      # δ: what a coordinate difference is off by
    # |∇W_d| and its rounding scale: u·|F|·|x_d| + δ·(|F| + |F'|·|x_d|) — the difference itself is off by δ in EVERY component, also where x_d = 0
    agW = afac[:, None] * ax
    sgW = FP32_ULP * agW + delta[:, None] * (afac[:, None] + adfac[:, None] * ax)
    vabs = np.abs(vel[i]) + np.abs(vel[j])
    cont = np.stack([(vabs * agW).sum(1), (vabs * sgW).sum(1)])                          # [absolute, scale]
    a_i = rho[i] * (cfg.m0 / rho[j]) * cont
    a_j = rho[j] * (cfg.m0 / rho[i]) * cont
    if linear:
        arhoH = np.abs(cfg.rho0 * cfg.g * xij[:, -1] * ((1 / (cfg.Cb * cfg.gamma)) * cfg.rho0))
        aD = cfg.delta_phi * cfg.h * cfg.c0 * (cfg.m0 / rho_n[j]) * 2 * (np.abs(rho_n[j] - rho_n[i]) + arhoH) * (r2 / (r2 + cfg.eta2)) * ml[i] * ml[j]
        aD = aD * np.stack([afac, FP32_ULP * afac + delta * adfac])
        a_i, a_j = a_i + aD, a_j + aD
    aP = cfg.m0 * (np.abs(press[i]) + np.abs(press[j]) + cfg.c0 ** 2 * (rho[i] + rho[j])) / (rho[i] * rho[j])
    if artificial:
        avdx = (vabs * ax).sum(1)
        aP = aP + np.where((((vel[i] - vel[j]) * xij).sum(1)) < 0,
                           cfg.m0 * cfg.alpha * cfg.c0 * cfg.h * avdx / (r2 + cfg.eta2) / (0.5 * (rho_n[i] + rho_n[j])), 0.0)
    out = {}
    for k, (name, g) in enumerate((("abs", agW), ("scale", sgW))):
        sd, sa = np.zeros(N), np.zeros((N, D))
        np.add.at(sd, i, a_i[k]); np.add.at(sd, j, a_j[k])
        np.add.at(sa, i, aP[:, None] * g); np.add.at(sa, j, aP[:, None] * g)
        out[name + "_drho"], out[name + "_acc"] = sd, sa
    return SimpleNamespace(drho=drho, acc=acc, npairs=len(a), i=i, j=j, q=q64, r=r64, t_drho_i=t_drho_i, t_drho_j=t_drho_j, t_acc=um, **out)


def eos(cfg, rho):
    return ((cfg.c0 ** 2 * cfg.rho0) / 7) * ((rho / cfg.rho0) ** 7 - 1)
