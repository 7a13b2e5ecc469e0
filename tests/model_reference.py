"""Independent numpy reference of EVERY model the C ABI covers, per particle and per term, with its rounding scale.

Written from the Julia sources (src/…, cited per formula), sharing no code with oracle/sph_oracle.c or the kernels.  From tests/bruteforce.py it
takes the pair list (KD-tree, r² ≤ H², valid right after a rebuild), the i/j orientation rule and cell_of / _lex_key; nothing else.

    forces(cfg, st, dtype)      one force evaluation (src/SPHCellList.jl:268-317): the sums drho / acc, every term's share of them
                                (`terms`: continuity, diffusion → dρ/dt; pressure, tensile, viscosity, sps → acceleration), ΣW and Σ∇W
                                (KernelOutput!, :106-116), ∇C and ∇◌r (add_shifting_terms!, :73-88), and next to every signed sum its
                                ABSOLUTE sum A_i (`A[...]`).
    mdbc(cfg, st, dtype)        the boundary densities of ApplyMDBCBeforeHalf! (:219-266, :319-365, :598-622) with the branch per node.
    step(cfg, st, dtype)        one predictor-corrector step (:742-802) with either FullTimeStep (:640-677), shaped like
                                fused_pair_reference.step.

dtype = numpy.longdouble evaluates the same statements wide.  THE SCALE of a compared value is S_i = 2⁻⁵³·A_i: A_i is the sum of the pair terms
with every COMPUTED operand that cancels entering with its magnitude —
    q − 2, 1 − q/2 and the polynomial branches of the kernels        |q| + 2 …: ∇W = F·x gets |F| + what one rounding of q and of 2 − q does to F
    P = Cb((ρ/ρ₀)⁷ − 1)                                              |P| + c₀²ρ: seven roundings of a number near 1 in front of Cb
    ρ₀·(root − 1) of the Complex diffusion                           ρ₀·(|root| + 1)
    the dot products v·∇W, x·∇W, ψ·∇W, τ·∇W                          Σ_d |·|_d |·|_d
    the mDBC solve                                                   |c|ᵀ|A⁻¹|(|A|ₐ|x| + |b|ₐ)·(D+1) + |c|ᵀ|x| with the absolute sums |A|ₐ, |b|ₐ
— while a difference of two numbers of the exact start state (xᵢ − xⱼ, vᵢ − vⱼ, ρⱼ − ρᵢ) is exact up to its own rounding and enters as it
is.  The corrector of a step runs on a COMPUTED state: there xᵢ − xⱼ is off by 2⁻⁵³(|xᵢ| + |xⱼ|) (∇W_d gets (|xᵢ|+|xⱼ|)·(|F| + √D|F'||x_d|)),
v⁺ by 2⁻⁵³(Δt/2·A(a₁) + |v⁺|), ρ⁺ by 2⁻⁵³(Δt/2·A(dρ/dt₁) + ρ⁺) (`computed=` of forces).

THE BAR (profiles/fused_pair_parity.md's method): Q = max_i |ref64 − ref_wide|_i / S_i per layout, field and term, measured here, reference
against reference; a compared value has to lie within FACTOR·Q·S_i of the wide reference, FACTOR = 4 for another summation order.  An isolated
term (variant − base of two runs) uses the term's A_i plus the full field's A_i, the rounding of the two sums that are subtracted.
No allowance for fast-math forms is applied anywhere: the engine's fp64 kernels stay inside the bar without one.

MUTANTS: named misreadings of the formulas here (`mutant=`), which tests/test_model_reference_host.py shows to move at least one particle by
more than 10 bars — what the bar can see, without touching a kernel."""
import functools
from types import SimpleNamespace

import numpy as np
from scipy.spatial import cKDTree

import bruteforce as bf

assert np.finfo(np.longdouble).eps < 2.0 ** -60, "numpy.longdouble is no wider than float64 here: no wide reference"

U = 2.0 ** -53
FACTOR = 4.0

MUTANTS = ("sps_trace_over_D", "no_blin", "cubic_outer_branch", "tensile_W_of_dx_over_h", "divr_rho_swapped", "no_mlcond_shifting",
           "no_mlcond_linear", "laminar_brackets", "complex_as_linear", "mdbc_shepard_rho0", "mdbc_signed_det")

WENDLAND, CUBIC = 0, 1
V_ZERO, V_ARTIFICIAL, V_LAMINAR, V_SPS = 0, 1, 2, 3
D_ZERO, D_ZEROGRAV, D_LINEAR, D_COMPLEX = 0, 1, 2, 3
SKIPPED, SOLVE, SHEPARD, UNTOUCHED = 0, 1, 2, 3


# ------------------------------------------------------------------------------------------------------------------ kernels
def kernel_W(cfg, q, f, mutant=None):
    """Wᵢⱼ: src/SPHKernels.jl:75-78 (WendlandC2), :89-92 (CubicSpline)."""
    aD = f(cfg.alphaD)
    if cfg.kernel == WENDLAND:
        t = f(1) - q / f(2)
        return aD * t ** 4 * (f(2) * q + f(1))
    inner = (f(1) - f(1.5) * q ** 2 + f(0.75) * q ** 3) * ((q >= 0) & (q <= 1))
    outer = f(0.25) * (f(2) - q) ** 3 * ((q > 1) & (q <= 2))
    return aD * (inner + outer)


def kernel_W_abs(cfg, q):
    if cfg.kernel == WENDLAND:
        t = 1 - q / 2
        return cfg.alphaD * (t ** 4 * (2 * q + 1) + 4 * t ** 3 * (1 + q / 2) * (2 * q + 1))
    return cfg.alphaD * np.where(q <= 1, 1 + 1.5 * q ** 2 + 0.75 * q ** 3, 0.25 * ((2 - q) ** 3 + 3 * (2 - q) ** 2 * (q + 2)))


def kernel_F(cfg, q, r, f, mutant=None):
    """∇Wᵢⱼ = F·xᵢⱼ: src/SPHKernels.jl:80-87 (WendlandC2: αD·5(q−2)³/(8h·h)), :94-110 (CubicSpline: dW/dq·h⁻¹/(|xᵢⱼ| + η²), both branches)."""
    aD = f(cfg.alphaD)
    if cfg.kernel == WENDLAND:
        return aD * f(5) * (q - f(2)) ** 3 / (f(8) * f(cfg.h) * f(cfg.h))
    outer = aD * f(-0.75) * (f(2) - q) ** 2
    inner = aD * (f(-3) * q + f(2.25) * q ** 2)
    dWdq = outer if mutant == "cubic_outer_branch" else np.where(q <= 1, inner, outer)
    return dWdq * f(cfg.h_inv) / (r + f(cfg.eta2))


def kernel_F_abs(cfg, q, r):
    """(|F| with q, 2 − q and the branch polynomial entering by magnitude, |dF/dr|)."""
    if cfg.kernel == WENDLAND:
        c = cfg.alphaD * 5 / (8 * cfg.h * cfg.h)
        return c * ((2 - q) ** 3 + 3 * (2 - q) ** 2 * (q + 2)), c * 3 * (2 - q) ** 2 * cfg.h_inv
    a = cfg.alphaD * np.where(q <= 1, 3 * q + 2.25 * q ** 2, 0.75 * ((2 - q) ** 2 + 2 * (2 - q) * (q + 2)))
    da = cfg.alphaD * np.where(q <= 1, 3 + 4.5 * q, 1.5 * (2 - q)) * cfg.h_inv
    g = cfg.h_inv / (r + cfg.eta2)
    return a * g, da * g + a * g / (r + cfg.eta2)


def eos(cfg, rho, f):
    """EquationOfStateGamma7, src/SimulationEquations.jl:9-11 (@fastpow: the seventh power by multiplication)."""
    r = rho / f(cfg.rho0)
    r2 = r * r; r4 = r2 * r2
    return ((f(cfg.c0) * f(cfg.c0) * f(cfg.rho0)) / f(7)) * (r4 * r2 * r - f(1))


def seventh_root(x, f):
    """Estimate7thRoot, src/SimulationEquations.jl:49-61: the bit pattern of the Float64 x gives the start value, two steps of the iteration
    follow in the type of f."""
    x64 = np.abs(np.asarray(x, dtype=np.float64))
    t = np.copysign((np.uint64(0x36cd000000000000) + x64.view(np.uint64) // np.uint64(7)).view(np.float64), np.asarray(x, dtype=np.float64)).astype(f)
    for _ in range(2):
        t2 = t * t; t3 = t2 * t; t4 = t2 * t2; xot4 = x / t4
        t = t - t * (t3 - xot4) / (f(4) * t3 + f(3) * xot4)
    return t


# ------------------------------------------------------------------------------------------------------------------ pairs
def pair_list(cfg, pos, cell_pos=None, order_index=None):
    """(i, j) of every pair with r² ≤ H², oriented as the reference's cell loop meets it (bruteforce.pair_forces)."""
    n = len(pos)
    if order_index is None:
        order_index = np.arange(n)
    if n < 2:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    pairs = cKDTree(pos).query_pairs(cfg.H * (1 + 1e-9), output_type="ndarray")
    a, b = pairs[:, 0], pairs[:, 1]
    x = pos[a] - pos[b]
    keep = (x * x).sum(1) <= cfg.H2
    a, b = a[keep], b[keep]
    key = bf._lex_key(bf.cell_of(pos if cell_pos is None else cell_pos, cfg.H_inv))
    a_is_i = np.where(key[a] == key[b], order_index[a] < order_index[b], key[a] > key[b])
    return np.where(a_is_i, a, b), np.where(a_is_i, b, a)


def _scatter(n, shape, dtype, *adds):
    out = np.zeros((n, *shape), dtype=dtype)
    for rows, vals in adds:
        np.add.at(out, rows, vals)
    return out


def forces(cfg, st, dtype=np.float64, mutant=None, rho_n=None, vel_n=None, press=None, cell_pos=None, computed=None, pos_wide=None):
    """One NeighborLoop! over the state st = (pos, vel, rho, ml) in row order (= in-cell order of the stable sort).  rho_n / vel_n:
    SimParticles.Density / .Velocity where they are not the loop's arguments (the corrector: the diffusion models, ρ̄ of the artificial and
    the denominators of the Laminar viscosity and the whole SPS stress read them, src/SPHViscosityModels.jl:61-62,82-83,96-100,
    src/SPHDensityDiffusionModels.jl:72-73,118-119,166-167).  press: Pressure where it is not P(rho) (after mDBC, :771-772).
    computed = (dvel [N, D], drho [N]): the state is a half-step state known to these absolute errors ÷ 2⁻⁵³ (module docstring);
    pos_wide: its positions in dtype, where st.pos is their fp64 image (the pair list is always the fp64 one)."""
    f = np.dtype(dtype).type
    n, D = st.pos.shape
    i, j = pair_list(cfg, st.pos, cell_pos)
    pos, vel, rho, ml = (np.asarray(v).astype(dtype) for v in (st.pos if pos_wide is None else pos_wide, st.vel, st.rho, st.ml))
    rn = rho if rho_n is None else np.asarray(rho_n).astype(dtype)
    vn = vel if vel_n is None else np.asarray(vel_n).astype(dtype)
    P = eos(cfg, rho, f) if press is None else np.asarray(press).astype(dtype)
    m0, h, eta2 = f(cfg.m0), f(cfg.h), f(cfg.eta2)
    # src/SPHCellList.jl:273-281
    xij = pos[i] - pos[j]
    r2 = (xij * xij).sum(1)
    r = np.sqrt(np.abs(r2))
    q = np.clip(r * f(cfg.h_inv), f(0), f(2))
    F = kernel_F(cfg, q, r, f, mutant)
    gW = F[:, None] * xij
    ri, rj, vij = rho[i], rho[j], vel[i] - vel[j]
    mlc = ml[i] * ml[j]
    # :289-291
    sym = (-vij * gW).sum(1)
    cont_i, cont_j = -ri * (m0 / rj) * sym, -rj * (m0 / ri) * sym
    # density diffusion
    dd = cfg.density_diffusion
    Di = np.zeros(len(i), dtype)
    rhoH = np.zeros(len(i), dtype)
    root = None
    if dd != D_ZERO:
        if dd in (D_LINEAR, D_COMPLEX):
            PH = f(cfg.rho0) * f(-cfg.g) * -xij[:, -1]                                         # src/SPHDensityDiffusionModels.jl:121, :172
            if dd == D_LINEAR or mutant == "complex_as_linear":
                rhoH = PH * ((f(1) / (f(cfg.Cb) * f(cfg.gamma))) * f(cfg.rho0))                # :116, :122
            else:
                root = seventh_root(f(1) + PH * (f(1) / f(cfg.Cb)), f)                         # :173, src/SimulationEquations.jl:63 (Cb⁻¹ = 1/Cb)
                rhoH = f(cfg.rho0) * (root - f(1))
        psi = f(2) * ((rn[j] - rn[i]) - rhoH)[:, None] * (-xij) * (f(1) / (r2 + eta2))[:, None]  # :77-80, :125-128, :177-180
        Di = f(cfg.delta_phi) * h * f(cfg.c0) * (m0 / rn[j]) * (psi * gW).sum(1)               # :82, :132, :184
        if dd != D_ZEROGRAV and not (dd == D_LINEAR and mutant == "no_mlcond_linear"):
            Di = Di * mlc                                                                      # :130-132, :182-184 (not in :56-87)
    # :299-303 and src/SPHKernels.jl:115-126
    Pfac = (P[i] + P[j]) / (ri * rj)
    f_ab = np.zeros(len(i), dtype)
    if cfg.kernel == CUBIC:
        W_ref = kernel_W(cfg, np.asarray(f(cfg.dx) / h if mutant == "tensile_W_of_dx_over_h" else f(cfg.dx)), f)      # Wᵢⱼ(instance, dx), as written
        f_ab = f(cfg.cubic_eps) * ((P[i] / ri ** 2 + P[j] / rj ** 2) * (kernel_W(cfg, q, f) / W_ref) ** 4)
    t_press, t_tens = -m0 * Pfac[:, None] * gW, -m0 * f_ab[:, None] * gW
    um = -m0 * (Pfac + f_ab)[:, None] * gW
    # viscosity
    visc = cfg.viscosity
    t_visc, t_sps = np.zeros_like(gW), np.zeros_like(gW)
    if visc == V_ARTIFICIAL:                                                                   # src/SPHViscosityModels.jl:56-74
        vdx = (vij * xij).sum(1)
        mu = h * vdx / (r2 + eta2)
        k = np.where(vdx < 0, -m0 * (f(-cfg.alpha) * f(cfg.c0) * mu) / (f(0.5) * (rn[i] + rn[j])), f(0))
        t_visc = k[:, None] * gW
    elif visc in (V_LAMINAR, V_SPS):                                                           # :77-87, brackets as written
        xdg = (xij * gW).sum(1)
        den = (rn[i] + rn[j]) * (r2 + eta2) if mutant == "laminar_brackets" else (rn[i] + rn[j]) + (r2 + eta2)
        t_visc = ((f(4) * m0 * f(cfg.nu0) * xdg) / den)[:, None] * vij
        if visc == V_SPS:                                                                      # :90-126
            I = np.eye(D, dtype=dtype)
            third = f(1) / f(D) if mutant == "sps_trace_over_D" else f(1) / f(3)
            blin = f(0) if mutant == "no_blin" else f(cfg.blin_constant)
            dx2, cs2 = f(cfg.dx) ** 2, (f(cfg.smagorinsky_constant) * f(cfg.dx)) ** 2

            def tau(S, rho_):
                norm = np.sqrt(f(2) * (S ** 2).sum((1, 2)))
                nut = cs2 * norm
                tr = np.trace(S, axis1=1, axis2=2)
                return ((f(2) * nut * rho_)[:, None, None] * (S - (third * tr)[:, None, None] * I)
                        - ((f(2) / f(3)) * rho_ * blin * dx2 * norm ** 2)[:, None, None] * I)
            Si = (m0 / rn[j])[:, None, None] * ((vn[j] - vn[i])[:, :, None] * gW[:, None, :])
            Sj = (m0 / rn[i])[:, None, None] * ((vn[i] - vn[j])[:, :, None] * -gW[:, None, :])
            t_sps = (m0 / (rn[j] * rn[i]))[:, None] * np.einsum("pab,pb->pa", tau(Si, rn[i]) + tau(Sj, rn[j]), gW)
    um = um + (t_visc + t_sps)
    W = kernel_W(cfg, q, f)
    # add_shifting_terms!, src/SPHCellList.jl:78-86
    smlc = np.ones_like(mlc) if mutant == "no_mlcond_shifting" else mlc
    xdg = (xij * gW).sum(1)
    ra, rb = (ri, rj) if mutant == "divr_rho_swapped" else (rj, ri)
    out = SimpleNamespace(i=i, j=j, q=q.astype(float), r=r.astype(float), npairs=len(i), pressure=P)
    out.drho = _scatter(n, (), dtype, (i, cont_i + Di), (j, cont_j - Di))                      # :295-296
    out.acc = _scatter(n, (D,), dtype, (i, um), (j, -um))                                      # :307-309
    out.terms = {"continuity": _scatter(n, (), dtype, (i, cont_i), (j, cont_j)), "diffusion": _scatter(n, (), dtype, (i, Di), (j, -Di)),
                 "pressure": _scatter(n, (D,), dtype, (i, t_press), (j, -t_press)), "tensile": _scatter(n, (D,), dtype, (i, t_tens), (j, -t_tens)),
                 "viscosity": _scatter(n, (D,), dtype, (i, t_visc), (j, -t_visc)), "sps": _scatter(n, (D,), dtype, (i, t_sps), (j, -t_sps))}
    out.kernel = _scatter(n, (), dtype, (i, W), (j, W))                                        # :110-114
    out.kernel_gradient = _scatter(n, (D,), dtype, (i, gW), (j, -gW))
    out.gradC = _scatter(n, (D,), dtype, (i, (m0 / ri)[:, None] * gW), (j, (m0 / rj)[:, None] * -gW))
    out.divr = _scatter(n, (), dtype, (i, (m0 / ra) * (-xdg) * smlc), (j, (m0 / rb) * (-xdg) * smlc))
    out.A = _absolute(cfg, st, i, j, rn, vn, P, root, computed)
    return out


def _absolute(cfg, st, i, j, rn, vn, P, root, computed):
    """The absolute sums A of every sum of `forces`, in fp64 (module docstring)."""
    n, D = st.pos.shape
    pos, vel, rho, ml = (np.asarray(v, dtype=np.float64) for v in (st.pos, st.vel, st.rho, st.ml))
    rn, vn, P = np.abs(np.asarray(rn, dtype=np.float64)), np.asarray(vn, dtype=np.float64), np.asarray(P, dtype=np.float64)
    rho = np.abs(rho)                                                   # (a magnitude: the A_FSC < 0 layout plants negative densities)
    m0, h, eta2 = cfg.m0, cfg.h, cfg.eta2
    xij = pos[i] - pos[j]; ax = np.abs(xij)
    r2 = (xij * xij).sum(1); r = np.sqrt(r2); q = np.clip(r * cfg.h_inv, 0, 2)
    aF, adF = kernel_F_abs(cfg, q, r)
    F = np.abs(kernel_F(cfg, q, r, np.float64))
    agW = aF[:, None] * ax
    if computed is None:
        vabs, drho_i, drho_j = np.abs(vel[i] - vel[j]), rho[i], rho[j]
    else:
        dvel, drho = computed
        xabs = (np.abs(pos[i]) + np.abs(pos[j])).max(1)
        agW = agW + xabs[:, None] * (F[:, None] + np.sqrt(D) * adF[:, None] * ax)
        vabs, drho_i, drho_j = dvel[i] + dvel[j], drho[i], drho[j]
    ri, rj = rho[i], rho[j]
    mlc = ml[i] * ml[j]
    a_cont = (vabs * agW).sum(1)
    a_ci, a_cj = ri * (m0 / rj) * a_cont, rj * (m0 / ri) * a_cont
    aD = np.zeros(len(i))
    dd = cfg.density_diffusion
    if dd != D_ZERO:
        aH = np.zeros(len(i))
        if dd in (D_LINEAR, D_COMPLEX):
            aH = np.abs(cfg.rho0 * cfg.g * xij[:, -1] * ((1 / (cfg.Cb * cfg.gamma)) * cfg.rho0))
            if root is not None:
                aH = cfg.rho0 * (np.abs(np.asarray(root, dtype=np.float64)) + 1)
        aD = cfg.delta_phi * h * cfg.c0 * (m0 / rn[j]) * 2 * (np.abs(rn[j] - rn[i]) + aH) * (ax * agW).sum(1) / (r2 + eta2)
        if dd != D_ZEROGRAV:
            aD = aD * mlc
    c2 = cfg.c0 ** 2
    aPfac = (np.abs(P[i]) + np.abs(P[j]) + c2 * (drho_i + drho_j)) / (ri * rj)
    a_press = m0 * aPfac[:, None] * agW
    a_tens = np.zeros_like(agW)
    if cfg.kernel == CUBIC:
        Wq, aWq = kernel_W(cfg, q, np.float64), kernel_W_abs(cfg, q)
        Wr = kernel_W(cfg, np.asarray(cfg.dx), np.float64)
        ratio4 = (Wq / Wr) ** 4 + 4 * (Wq / Wr) ** 3 * (aWq / Wr)
        a_tens = m0 * (np.abs(cfg.cubic_eps) * ((np.abs(P[i]) + c2 * drho_i) / ri ** 2 + (np.abs(P[j]) + c2 * drho_j) / rj ** 2) * ratio4)[:, None] * agW
    a_visc, a_sps = np.zeros_like(agW), np.zeros_like(agW)
    if cfg.viscosity == V_ARTIFICIAL:
        neg = ((vel[i] - vel[j]) * xij).sum(1) < 0
        a_visc = np.where(neg, m0 * cfg.alpha * cfg.c0 * h * (vabs * ax).sum(1) / (r2 + eta2) / (0.5 * (rn[i] + rn[j])), 0.0)[:, None] * agW
    elif cfg.viscosity in (V_LAMINAR, V_SPS):
        a_visc = ((4 * m0 * cfg.nu0 * (ax * agW).sum(1)) / ((rn[i] + rn[j]) + (r2 + eta2)))[:, None] * vabs
        if cfg.viscosity == V_SPS:
            dv = np.abs(vn[i] - vn[j])
            dx2, cs2 = cfg.dx ** 2, (cfg.smagorinsky_constant * cfg.dx) ** 2
            for c_, rho_ in ((m0 / rn[j], rn[i]), (m0 / rn[i], rn[j])):
                S = c_[:, None, None] * dv[:, :, None] * agW[:, None, :]
                norm = np.sqrt(2 * (S ** 2).sum((1, 2)))
                tau = (2 * cs2 * norm * rho_)[:, None, None] * (S + (np.trace(S, axis1=1, axis2=2) / 3)[:, None, None] * np.eye(D)) \
                    + ((2 / 3) * rho_ * abs(cfg.blin_constant) * dx2 * norm ** 2)[:, None, None] * np.eye(D)
                a_sps = a_sps + (m0 / (rn[j] * rn[i]))[:, None] * np.einsum("pab,pb->pa", tau, agW)
    a_um = a_press + a_tens + a_visc + a_sps
    aW = kernel_W_abs(cfg, q)
    if computed is not None:
        aW = aW + xabs * np.sqrt(D) * F * r                                   # |dW/dr| = |F|·r: W of a computed position difference
    axdg = (ax * agW).sum(1)
    A = {"drho": _scatter(n, (), float, (i, a_ci + aD), (j, a_cj + aD)), "acc": _scatter(n, (D,), float, (i, a_um), (j, a_um)),
         "continuity": _scatter(n, (), float, (i, a_ci), (j, a_cj)), "diffusion": _scatter(n, (), float, (i, aD), (j, aD)),
         "pressure": _scatter(n, (D,), float, (i, a_press), (j, a_press)), "tensile": _scatter(n, (D,), float, (i, a_tens), (j, a_tens)),
         "viscosity": _scatter(n, (D,), float, (i, a_visc), (j, a_visc)), "sps": _scatter(n, (D,), float, (i, a_sps), (j, a_sps)),
         "kernel": _scatter(n, (), float, (i, aW), (j, aW)), "kernel_gradient": _scatter(n, (D,), float, (i, agW), (j, agW)),
         "gradC": _scatter(n, (D,), float, (i, (m0 / ri)[:, None] * agW), (j, (m0 / rj)[:, None] * agW)),
         "divr": _scatter(n, (), float, (i, (m0 / rj) * axdg), (j, (m0 / ri) * axdg))}
    return A


# ------------------------------------------------------------------------------------------------------------------ mDBC
def _solve_wide(A, b):
    """Gaussian elimination with partial pivoting on a stack of small systems in the type of A (numpy.linalg has no longdouble);
    returns (det, x)."""
    A, b = A.copy(), b.copy()
    m, n, _ = A.shape
    det = np.ones(m, A.dtype)
    rows = np.arange(m)
    for k in range(n):
        p = k + np.abs(A[:, k:, k]).argmax(1)
        swap = p != k
        Ak, Ap = A[rows, k].copy(), A[rows, p].copy()
        A[rows, k], A[rows, p] = Ap, Ak
        bk, bp = b[rows, k].copy(), b[rows, p].copy()
        b[rows, k], b[rows, p] = bp, bk
        det = det * np.where(swap, -1, 1) * A[:, k, k]
        piv = np.where(A[:, k, k] == 0, 1, A[:, k, k])
        for r_ in range(k + 1, n):
            fct = A[:, r_, k] / piv
            A[:, r_] = A[:, r_] - fct[:, None] * A[:, k]
            b[:, r_] = b[:, r_] - fct * b[:, k]
    x = np.zeros_like(b)
    for k in range(n - 1, -1, -1):
        piv = np.where(A[:, k, k] == 0, 1, A[:, k, k])
        x[:, k] = (b[:, k] - (A[:, k, k + 1:] * x[:, k + 1:]).sum(1)) / piv
    return det, x


def mdbc(cfg, st, dtype=np.float64, mutant=None):
    """NeighborLoopMDBC! + ComputeInteractionsMDBC! + ApplyMDBCCorrection.  st carries `type` (1 = Fluid) and `ghost` [N, D].  Returns the
    densities after the correction, the branch per row (SKIPPED: zero ghost vector, SOLVE, SHEPARD, UNTOUCHED), det, the moment sums
    (Amat [N, D+1, D+1], bvec) and the absolute term A of the density."""
    f = np.dtype(dtype).type
    n, D = st.pos.shape
    P_ = D + 1
    ghost = np.asarray(st.ghost, dtype=np.float64)
    nodes = np.nonzero((ghost != 0).any(1))[0]                                                   # src/SPHCellList.jl:231, :610
    fluid = np.nonzero(np.asarray(st.type) == 1)[0]                                              # :331
    Amat, bvec = np.zeros((n, P_, P_), dtype), np.zeros((n, P_), dtype)
    Aabs, babs = np.zeros((n, P_, P_)), np.zeros((n, P_))
    if len(nodes) and len(fluid):
        hits = cKDTree(st.pos[fluid]).query_ball_point(ghost[nodes], cfg.H * (1 + 1e-9))
        gi = np.repeat(np.arange(len(nodes)), [len(h_) for h_ in hits]).astype(np.int64)
        fj = fluid[np.concatenate([np.asarray(h_, dtype=np.int64) for h_ in hits])] if len(gi) else np.zeros(0, np.int64)
        x64 = ghost[nodes][gi] - st.pos[fj]
        keep = (x64 * x64).sum(1) <= cfg.H2                                                       # :336
        gi, fj = nodes[gi[keep]], fj[keep]
        xij = ghost.astype(dtype)[gi] - st.pos.astype(dtype)[fj]                                  # :333
        r2 = (xij * xij).sum(1); r = np.sqrt(np.abs(r2))
        q = np.clip(r * f(cfg.h_inv), f(0), f(2))                                                 # :337-338
        W = kernel_W(cfg, q, f)                                                                   # :343
        gW = kernel_F(cfg, q, r, f)[:, None] * xij                                                # :345
        V = f(cfg.m0) / st.rho.astype(dtype)[fj]                                                  # :347
        fc = np.concatenate([(V * W)[:, None], V[:, None] * gW], axis=1)                          # :355
        bD = np.concatenate([(f(cfg.m0) * W)[:, None], f(cfg.m0) * gW], axis=1)                   # :351
        AD = np.concatenate([fc[:, :, None], fc[:, :, None] * (-xij)[:, None, :]], axis=2)        # :354-359 (column-major fill)
        np.add.at(Amat, gi, AD); np.add.at(bvec, gi, bD)
        q64, r64 = q.astype(float), r.astype(float)
        aF, _ = kernel_F_abs(cfg, q64, r64)
        afc = np.concatenate([kernel_W_abs(cfg, q64)[:, None], aF[:, None] * np.abs(xij.astype(float))], axis=1) * np.abs(V.astype(float))[:, None]
        np.add.at(Aabs, gi, np.concatenate([afc[:, :, None], afc[:, :, None] * np.abs(xij.astype(float))[:, None, :]], axis=2))
        np.add.at(babs, gi, afc / np.abs(V.astype(float))[:, None] * cfg.m0)
    rho = st.rho.astype(dtype).copy()
    branch = np.full(n, SKIPPED)
    det = np.zeros(n, dtype)
    Aden = np.abs(st.rho.astype(float))
    if len(nodes):
        An, bn = Amat[nodes], bvec[nodes]
        if np.dtype(dtype) == np.float64:
            det[nodes] = np.linalg.det(An)
        else:
            det[nodes] = _solve_wide(An, bn)[0]
        big = (det[nodes] >= 1e-3) if mutant == "mdbc_signed_det" else (np.abs(det[nodes]) >= 1e-3)          # :611
        shep = ~big & (An[:, 0, 0] > 0)                                                           # :616
        branch[nodes] = np.where(big, SOLVE, np.where(shep, SHEPARD, UNTOUCHED))
        s = nodes[big]
        if len(s):
            x = np.linalg.solve(Amat[s], bvec[s][:, :, None])[:, :, 0] if np.dtype(dtype) == np.float64 else _solve_wide(Amat[s], bvec[s])[1]   # :612
            diff = st.pos.astype(dtype)[s] - ghost.astype(dtype)[s]                               # :613
            v1 = x[:, 0] + (x[:, 1:] * diff).sum(1)                                               # :614
            rho[s] = np.where(np.isnan(v1), f(cfg.rho0), v1)                                      # :615
            c = np.concatenate([np.ones((len(s), 1)), np.abs(diff.astype(float))], axis=1)
            inv = np.abs(np.linalg.inv(Amat[s].astype(float)))
            x64 = np.abs(x.astype(float))
            e = np.einsum("nab,nb->na", inv, np.einsum("nab,nb->na", Aabs[s], x64) + babs[s])
            Aden[s] = (c * e).sum(1) * P_ + (c * x64).sum(1)
        t = nodes[shep]
        if len(t):
            v = bvec[t, 0] / Amat[t, 0, 0]                                                        # :617
            rho[t] = f(cfg.rho0) if mutant == "mdbc_shepard_rho0" else np.where(np.isnan(v), f(cfg.rho0), v)   # :618
            Aden[t] = 2 * np.abs(v.astype(float))
    return SimpleNamespace(rho=rho, branch=branch, det=det, Amat=Amat, bvec=bvec, A=Aden, nodes=nodes)


def forces_mdbc(cfg, st, dtype=np.float64, mutant=None):
    """forces_once(apply_mdbc=True): Pressure! runs on the densities BEFORE the correction (src/SPHCellList.jl:771-774)."""
    f = np.dtype(dtype).type
    m = mdbc(cfg, st, dtype, mutant)
    st2 = SimpleNamespace(**{**vars(st), "rho": m.rho})
    return m, forces(cfg, st2, dtype, mutant, press=eos(cfg, st.rho.astype(dtype), f))


# ------------------------------------------------------------------------------------------------------------------ one step
FIELDS = ("Position", "Velocity", "Density")


def step(cfg, st, dtype=np.float64, mutant=None):
    """One step of src/SPHCellList.jl:742-802 from st (zero Acceleration, no motion, no mDBC) with FullTimeStep :640-652 or, with
    cfg.shifting, :654-677.  The shape of fused_pair_reference.step: fields, the two pair-sum records p1 / p2, and the scales' pieces."""
    import fused_pair_reference as fr
    f = np.dtype(dtype).type
    n, D = st.pos.shape
    st0 = SimpleNamespace(pos=st.pos, vel=st.vel, acc=np.zeros_like(st.pos))
    dt64 = fr.delta_t(cfg, st0)                                                                   # src/TimeStepping.jl:24-46
    dt, dt2 = f(dt64), f(dt64) * f(0.5)
    ml = st.ml.astype(dtype)[:, None]
    grav = np.zeros((n, D), dtype); grav[:, -1] = f(cfg.g) * st.gf.astype(dtype)
    x, v, rho = st.pos.astype(dtype), st.vel.astype(dtype), st.rho.astype(dtype)
    lim = lambda r_: np.where((r_ < f(cfg.rho0)) & (st.ml == 0.0), f(cfg.rho0), r_)              # src/SimulationEquations.jl:36-42
    p1 = forces(cfg, st, dtype, mutant)
    a1 = p1.acc + grav                                                                            # :630
    x_h, v_h = x + v * dt2 * ml, v + a1 * dt2 * ml                                                # :631-632
    rho_h = lim(rho + p1.drho * dt2)                                                              # :633, :781
    sth = SimpleNamespace(pos=x_h.astype(float), vel=v_h, rho=rho_h, ml=st.ml)
    dvel = 0.5 * dt64 * st.ml[:, None] * (p1.A["acc"] + np.abs(a1.astype(float))) + np.abs(v_h.astype(float))
    drho = 0.5 * dt64 * p1.A["drho"] + np.abs(rho_h.astype(float))
    # the pair list of the corrector is the one of x⁺ in fp64 whatever dtype: the positions themselves are carried in dtype
    p2 = forces(cfg, sth, dtype, mutant, pos_wide=x_h, rho_n=rho, vel_n=v, cell_pos=st.pos, computed=(dvel, drho))
    rho_l = lim(rho)                                                                              # :794
    eps = -(p2.drho / rho_h) * dt                                                                 # :28-33
    dens = rho_l * ((f(2) - eps) / (f(2) + eps))
    a2 = p2.acc + grav                                                                            # :647 / :664
    ad = a2 * dt * ml
    vel = v + ad                                                                                  # :648 / :665
    shift = np.zeros((n, D), dtype)
    if cfg.shifting:
        afsc = (p2.divr - f(0)) / (f(D) - f(0))                                                   # :667
        vnorm = np.sqrt((vel * vel).sum(1))
        shift = np.where((afsc < 0)[:, None], f(0), (-afsc * f(2) * f(cfg.h) * vnorm * dt)[:, None] * p2.gradC)   # :668-672
    posn = x + (((vel + (vel - ad)) / f(2)) * dt + shift) * ml                                    # :649 / :674
    out = SimpleNamespace(fields={"Position": posn, "Velocity": vel, "Density": dens}, p1=p1, p2=p2, dt=dt64, afsc=(p2.divr / f(D)).astype(float), p2_pos=sth.pos)
    # absolute terms of the fields
    e = eps.astype(float); m_ = st.ml[:, None]
    A_a2 = p2.A["acc"] + np.abs(a2.astype(float))
    kappa = np.abs(4.0 / (2.0 + e) ** 2 * rho_l.astype(float) / rho_h.astype(float))
    A_shift = np.zeros((n, D))
    if cfg.shifting:
        af, vn_, gC = np.abs(out.afsc), vnorm.astype(float), np.abs(p2.gradC.astype(float))
        A_vn = dt64 * np.sqrt((A_a2 ** 2).sum(1)) + vn_
        A_shift = 2 * cfg.h * dt64 * ((p2.A["divr"] / D * vn_)[:, None] * gC + (af * A_vn)[:, None] * gC + (af * vn_)[:, None] * p2.A["gradC"])
        A_shift = np.where((out.afsc < 0)[:, None] & (p2.A["divr"] / D * U < np.abs(out.afsc))[:, None], 0.0, A_shift)
    out.A = {"Velocity": dt64 * m_ * A_a2 + np.abs(vel.astype(float)),
             "Density": kappa * dt64 * (p2.A["drho"] + np.abs(p2.drho.astype(float))) + np.abs(dens.astype(float)),
             "Position": m_ * (0.5 * dt64 * dt64 * A_a2 + dt64 * np.abs(vel.astype(float)) + A_shift) + np.abs(posn.astype(float))}
    return out


# ------------------------------------------------------------------------------------------------------------------ layouts
DX = 0.02
RAGGED = (1, 63, 65, 130, 257)
K_VARIANTS = (1.5, float(np.sqrt(2.0)), 2.5)
VISCOSITIES = ("ZeroViscosity", "ArtificialViscosity", "Laminar", "LaminarSPS")
DIFFUSIONS = ("ZeroDensityDiffusion", "ZeroGravityLinearDensityDiffusion", "LinearDensityDiffusion", "ComplexDensityDiffusion")


def make_setup(dims, viscosity="ArtificialViscosity", diffusion="LinearDensityDiffusion", kernel="WendlandC2", k=2.0, eps=0.3, shifting=False,
               kernel_output=False, mdbc=False):
    """dx with h = 1.2·dx, H = k·h; ν₀ = 1e-3 for the Laminar models (tests/test_engine_gpu.py, test_model_variants)."""
    import sphexample_amd.config as c
    from sphexample_amd.cases import CaseSetup
    consts = c.SimulationConstants(dx=DX, m0=1000.0 * DX ** dims, c0=40.0, alpha=0.05, nu0=1e-3 if "Laminar" in viscosity else 1e-6)
    kern = c.SPHKernelInstance(dims, c.CubicSpline(eps) if kernel == "CubicSpline" else c.WendlandC2(), h=1.2 * DX, k=k)
    meta = c.SimulationMetaData(Dimensions=dims, SMode=c.PlanarShifting if shifting else c.NoShifting,
                                KMode=c.StoreKernelOutput if kernel_output else c.NoKernelOutput, BMode=c.SimpleMDBC if mdbc else c.NoMDBC)
    return CaseSetup("model_reference", consts, kern, meta, getattr(c, viscosity)(), getattr(c, diffusion)())


def config(s, n):
    from sphexample_amd._abi import make_config
    return make_config(n, s.SimConstants, s.SimKernel, s.SimMetaData, s.SimViscosity, s.SimDensityDiffusion, device_float_bytes=8)


def _lattice(dims, n, width, rng, jitter):
    """The first n nodes of a lattice `width` wide (x fastest, the up axis slowest: the rows fill from the bottom), jittered, origin clear of 0."""
    idx = np.arange(n)
    coords = []
    for d in range(dims - 1):
        coords.append(idx % width); idx = idx // width
    coords.append(idx)
    grid = np.stack(coords, axis=1).astype(float)
    return (grid + 15.3) * DX + rng.uniform(-jitter, jitter, size=grid.shape) * DX, grid[:, -1]


@functools.lru_cache(maxsize=None)
def block(dims, n=None, jitter=0.25, seed=11, negative=0):
    """The jittered block: two layers of Fixed rows below, Fluid above with a free surface on top; random fluid velocities, ρ = ρ₀(1 ± 1 %).
    The full block (n = None) also has 24 lone Fluid rows above the surface, more than H from every Fluid row: ∇◌r = 0 exactly.
    negative: that many interior Fluid rows get ρ = −5, the only way to A_FSC < 0 (∇◌r sums (m₀/ρⱼ)·(−x·∇W) ≥ 0 for ρ > 0)."""
    from sphexample_amd import particles_from_arrays
    width = 50 if dims == 2 else 12
    lone = 0
    if n is None:
        n = 50 * 30 if dims == 2 else 12 * 12 * 11
        lone = 24
    elif n < 600:
        width = max(1, int(np.ceil((n / 1.5) ** (1.0 / dims))))
    rng = np.random.default_rng(seed + 1000 * dims + n)
    pos, layer = _lattice(dims, n, width, rng, jitter)
    ty = np.where(layer < 2, 2, 1) if n > 1 else np.array([1])
    if lone:
        top = pos[:, -1].max()
        extra = np.zeros((lone, dims)); extra[:, 0] = pos[:, 0].min() + 4.1 * DX * np.arange(lone) * (width / 50 if dims == 2 else 0.5)
        if dims == 3:
            extra[:, 0] = pos[:, 0].min() + 4.1 * DX * (np.arange(lone) % 6); extra[:, 1] = pos[:, 1].min() + 4.1 * DX * (np.arange(lone) // 6)
        else:
            extra[:, 0] = pos[:, 0].min() + 4.1 * DX * np.arange(lone)
        extra[:, -1] = top + 5.3 * DX
        extra += rng.uniform(-0.2, 0.2, size=extra.shape) * DX
        pos, ty, n = np.concatenate([pos, extra]), np.concatenate([ty, np.ones(lone, ty.dtype)]), n + lone
    p = particles_from_arrays(dims, pos, 1000.0 * (1 + rng.uniform(-0.01, 0.01, n)), ty, ty, np.arange(1, n + 1))
    p.Velocity[:] = rng.uniform(-0.5, 0.5, size=(n, dims)) * (ty == 1)[:, None]
    if negative:
        inner = np.nonzero((ty == 1) & (np.abs(pos - np.median(pos, 0)) < 6 * DX).all(1))[0]
        p.Density[inner[:: max(1, len(inner) // negative)][:negative]] = -5.0
    return p


@functools.lru_cache(maxsize=None)
def mdbc_block(dims, seed=5, negative=False):
    """A fluid block on two Fixed layers whose rows carry PLANTED ghost nodes of four kinds, in turn: full support (inside the fluid), thin
    one-sided support (beyond the free surface, the kernel's outer rim only: |det| < 1e-3, A₁₁ > 0), no Fluid row within H, the zero vector.
    negative: Fluid densities below zero, the only way to det ≤ −1e-3 (what tells |det| ≥ 1e-3 of src/SPHCellList.jl:611 from det ≥ 1e-3) —
    2-D: every Fluid row ρ → −ρ, the determinant of the 3 × 3 system changes sign with the volumes m₀/ρ; 3-D (4 × 4: it would not): three
    Fluid rows in ten at ρ = −300.  Reference and oracle only: the engine keeps the Fluid flag in the sign of ρ."""
    p = block(dims, 50 * 22 if dims == 2 else 12 * 12 * 8, seed=seed).copy()
    rng = np.random.default_rng(seed)
    if negative:
        fl = np.nonzero(p.Type == 1)[0]
        if dims == 2:
            p.Density[fl] = -p.Density[fl]
        else:
            p.Density[fl[np.random.default_rng(3).random(len(fl)) < 0.3]] = -300.0
    fixed = np.nonzero(p.Type == 2)[0]
    fluid = p.Position[p.Type == 1]
    lo, hi = fluid.min(0), fluid.max(0)
    H = 2 * 1.2 * DX
    g = np.zeros_like(p.Position)
    for n_, row in enumerate(fixed):
        kind = n_ % 4
        inner = lo + (hi - lo) * rng.uniform(0.25, 0.75, dims)
        if kind == 0:
            g[row] = inner
        elif kind == 1:
            g[row] = inner; g[row, -1] = hi[-1] + rng.uniform(0.45, 0.7) * H
        elif kind == 2:
            g[row] = inner; g[row, -1] = hi[-1] + rng.uniform(3, 4) * H
    p.GhostPoints[:] = g
    return p


def state_of(p):
    ty = np.asarray(p.Type)
    return SimpleNamespace(pos=np.array(p.Position, float), vel=np.array(p.Velocity, float), rho=np.array(p.Density, float), ml=(ty == 1).astype(float),
                           gf=np.where(ty == 1, -1.0, np.where(ty == 3, 1.0, 0.0)), type=ty, ghost=np.array(p.GhostPoints, float))


def clear_of_cut(cfg, st, mdbc_too=False):
    """Smallest |r²/H² − 1| over every pair the evaluation could meet (particle pairs and, for mDBC, node–Fluid pairs)."""
    worst = np.inf
    sets = [(st.pos, st.pos)]
    if mdbc_too:
        sets.append((st.ghost[(st.ghost != 0).any(1)], st.pos[st.type == 1]))
    for a, b in sets:
        if len(a) == 0 or len(b) == 0:
            continue
        ta, tb = cKDTree(a), cKDTree(b)
        m = ta.sparse_distance_matrix(tb, cfg.H * 1.01, output_type="ndarray")
        if len(m):
            d = m["v"][m["v"] > 0]
            if len(d):
                worst = min(worst, float(np.abs(d * d / cfg.H2 - 1).min()))
    return worst


# ------------------------------------------------------------------------------------------------------------------ the bar
def ratio(err, S):
    """max |err| / S over the entries with S > 0; entries with S = 0 must agree exactly."""
    err, S = np.abs(np.asarray(err, dtype=np.float64)), np.asarray(S, dtype=np.float64)
    S = np.broadcast_to(S, err.shape)
    assert (err[S == 0] == 0).all(), "a value without a scale differs"
    return float((err[S > 0] / S[S > 0]).max()) if (S > 0).any() else 0.0


FORCE_FIELDS = ("drho", "acc")
TERMS = ("continuity", "diffusion", "pressure", "tensile", "viscosity", "sps")
EXTRA = ("kernel", "kernel_gradient", "gradC", "divr")


def record_fields(r):
    return {"drho": r.drho, "acc": r.acc, **r.terms, "kernel": r.kernel, "kernel_gradient": r.kernel_gradient, "gradC": r.gradC, "divr": r.divr}


@functools.lru_cache(maxsize=None)
def reference(key):
    """(cfg, fp64 record, wide record, Q per field) of a case key = (kind, dims, n, viscosity, diffusion, kernel, k, eps, shifting, kernel output)."""
    kind, dims, n, visc, ddt, kernel, k, eps, shifting, kout = key
    s = make_setup(dims, visc, ddt, kernel, k, eps, shifting, kernel_output=kout, mdbc=kind.startswith("mdbc"))
    p = (mdbc_block(dims, negative=(kind == "mdbc-negative")) if kind.startswith("mdbc") else block(dims, negative=6) if kind == "step-negative"
         else block(dims, n))
    kind = kind.split("-")[0]
    cfg = config(s, len(p))
    st = state_of(p)
    if kind == "forces":
        r64, rw = forces(cfg, st), forces(cfg, st, np.longdouble)
        f64, fw, A = record_fields(r64), record_fields(rw), r64.A
    elif kind == "step":
        r64, rw = step(cfg, st), step(cfg, st, np.longdouble)
        f64, fw, A = dict(r64.fields), dict(rw.fields), dict(r64.A)
        for name in ("kernel", "kernel_gradient"):                 # ΣW, Σ∇W of the LAST neighbour pass: the corrector's, on the half-step state
            f64[name], fw[name], A[name] = getattr(r64.p2, name), getattr(rw.p2, name), r64.p2.A[name]
    else:
        r64, rw = mdbc(cfg, st), mdbc(cfg, st, np.longdouble)
        assert np.array_equal(r64.branch, rw.branch)
        f64, fw, A = {"Density": r64.rho}, {"Density": rw.rho}, {"Density": r64.A}
    Q = {name: ratio(f64[name] - fw[name], U * A[name]) for name in f64}
    return SimpleNamespace(cfg=cfg, s=s, p=p, st=st, r64=r64, wide=rw, fields=fw, A=A, Q=Q)


def key(kind, dims, n=None, visc="ArtificialViscosity", ddt="LinearDensityDiffusion", kernel="WendlandC2", k=2.0, eps=0.3, shifting=False, kout=True):
    return (kind, dims, n, visc, ddt, kernel, float(k), float(eps), bool(shifting), bool(kout))


# the isolated terms: term → (what the variant's key changes in the base's, the full field the two runs deliver)
ISOLATION_BASE = {"viscosity": (dict(visc="ZeroViscosity"), "acc"), "sps": (dict(visc="Laminar"), "acc"), "tensile": (dict(eps=0.0), "acc"),
                  "diffusion": (dict(ddt="ZeroDensityDiffusion"), "drho")}


def isolated(dims, term, **kw):
    """The bar of an ISOLATED term, (variant − base) of two runs: (variant record, base record, full field's name, A = the term's A_i plus the
    full field's, Q measured on the compared quantity itself: variant − base of the float64 reference against the wide term, over that A)."""
    change, field = ISOLATION_BASE[term]
    V, B = reference(key("forces", dims, **kw)), reference(key("forces", dims, **{**kw, **change}))
    assert not np.any(B.fields[term]) and np.any(V.fields[term])
    A = V.A[term] + V.A[field]
    ref64 = record_fields(V.r64)[field] - record_fields(B.r64)[field]
    return V, B, field, A, ratio(ref64 - V.fields[term], U * A)


def group_q(keys, name):
    """Q of a group of layouts that is ONE case (the ragged sizes: a lone particle measures nothing)."""
    return max(reference(k_).Q[name] for k_ in keys)


def check(name, got, ref, A, Q, extra_A=0.0, label=""):
    """A compared value against the wide reference: returns the largest normalised error, asserting it within FACTOR·Q."""
    S = U * (np.asarray(A) + extra_A)
    e = ratio(np.asarray(got, dtype=np.longdouble) - ref, S)
    print(f"{label:60s} {name:16s} Q={Q:7.3f} 4Q={FACTOR * Q:7.3f} err/S={e:8.3f} margin={(FACTOR * Q / e) if e else np.inf:7.1f}")
    assert e <= FACTOR * Q, (label, name, e, FACTOR * Q)
    return e
