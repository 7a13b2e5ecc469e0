"""The CPU oracle held to tests/model_reference.py per particle, for every model the C ABI covers; the layouts' conditions; what the bar sees.

The reference is numpy written from the Julia sources and shares no code with oracle/sph_oracle.c.  Bar: every compared value within
FACTOR·Q·S_i of the wide (numpy.longdouble) reference, Q measured float64 against longdouble on the same layout (model_reference docstring).
`pytest -s` prints Q, 4·Q and the largest normalised error per case and field: profiles/model_reference.md."""
import numpy as np
import pytest

import model_reference as mr

DIMS = (2, 3)
# every model alone, the WendlandC2 cut-offs, and the two combinations the examples use
MODELS = ([("visc-" + v, dict(visc=v, ddt="ZeroDensityDiffusion")) for v in mr.VISCOSITIES]
          + [("ddt-" + d, dict(visc="ZeroViscosity", ddt=d)) for d in mr.DIFFUSIONS[1:]]
          + [("cubic", dict(visc="ZeroViscosity", ddt="ZeroDensityDiffusion", kernel="CubicSpline"))]
          + [(f"k{k:.3f}", dict(k=k)) for k in mr.K_VARIANTS]
          + [("sps+linear+shifting", dict(visc="LaminarSPS", ddt="LinearDensityDiffusion", shifting=True)),
             ("cubic+artificial+linear", dict(kernel="CubicSpline"))])
MODEL_IDS = [m for m, _ in MODELS]
STEP_MODELS = [m for m in MODELS if m[0] in ("sps+linear+shifting", "cubic+artificial+linear", "visc-ArtificialViscosity")]


def oracle_of(R):
    from oracle.oracle import Oracle
    o = Oracle(R.cfg)
    o.upload_particles(R.p)
    return o


def by_id(o, *arrays):
    order = np.argsort(o.download(("ID",))["ID"], kind="stable")
    return [a[order] for a in arrays]


def sizes_keys(kind, dims, **kw):
    return [mr.key(kind, dims, n, **kw) for n in mr.RAGGED]


@pytest.mark.parametrize("dims", DIMS)
def test_layout_conditions(dims):
    """§2 of the issue, reference-side: both CubicSpline branches populated, no pair at the cut, MotionLimiter products 0 and 1 among the
    pairs, both signs of v·x, rows on both sides of A_FSC < 0, at least 20 mDBC nodes per branch and no determinant at the threshold."""
    R = mr.reference(mr.key("forces", dims, kernel="CubicSpline"))
    q = R.r64.q
    assert (q <= 1).mean() >= 0.10 and ((q > 1) & (q <= 2)).mean() >= 0.10, (q <= 1).mean()
    mlc = R.st.ml[R.r64.i] * R.st.ml[R.r64.j]
    assert (mlc == 0).sum() > 100 and (mlc == 1).sum() > 100
    vdx = ((R.st.vel[R.r64.i] - R.st.vel[R.r64.j]) * (R.st.pos[R.r64.i] - R.st.pos[R.r64.j])).sum(1)
    assert (vdx < 0).mean() > 0.2 and (vdx > 0).mean() > 0.2
    assert abs(R.st.rho / 1000 - 1).max() > 0.009
    for k in (2.0,) + mr.K_VARIANTS:
        for n in (None,) + mr.RAGGED:
            L = mr.reference(mr.key("forces", dims, n, k=k))
            assert mr.clear_of_cut(L.cfg, L.st) > 1e-9, (k, n)
    S = mr.reference(mr.key("step", dims, visc="LaminarSPS", shifting=True))
    fluid = S.st.ml == 1
    # A_FSC < 0 cannot occur with positive densities (∇◌r sums (m₀/ρⱼ)(−x·∇W)·MLcond, and −x·∇W ≥ 0 for both kernels): the block holds rows
    # ON the edge (lone Fluid rows, ∇◌r = 0 exactly) and above it; the branch itself is taken by the layout with planted negative densities,
    # which the engine cannot represent (its records carry the Fluid flag in the sign of ρ): reference against oracle only.
    assert (S.r64.afsc[fluid] == 0).sum() >= 20 and (S.r64.afsc[fluid] > 0).sum() >= 20 and (S.r64.afsc >= 0).all()
    Sn = mr.reference(mr.key("step-negative", dims, visc="LaminarSPS", ddt="ZeroDensityDiffusion", shifting=True))
    assert (Sn.r64.afsc[fluid] < 0).sum() >= 20 and (Sn.r64.afsc[fluid] > 0).sum() >= 20
    assert mr.clear_of_cut(Sn.cfg, mr.SimpleNamespace(pos=Sn.r64.p2_pos)) > 1e-9
    assert mr.clear_of_cut(S.cfg, mr.SimpleNamespace(pos=S.r64.p2_pos, ghost=None, type=None)) > 1e-9
    M = mr.reference(mr.key("mdbc", dims))
    assert mr.clear_of_cut(M.cfg, M.st, mdbc_too=True) > 1e-9
    Mn = mr.reference(mr.key("mdbc-negative", dims))                       # (same positions and nodes; densities below zero)
    detn = Mn.r64.det[Mn.r64.nodes].astype(float)
    assert (detn <= -1e-3).sum() >= 20 and (np.abs(np.abs(detn) / 1e-3 - 1) > 1e-6).all()
    for b in (mr.SKIPPED, mr.SOLVE, mr.SHEPARD, mr.UNTOUCHED):
        assert (M.r64.branch[M.st.type != 1] == b).sum() >= 20, b
    det = np.abs(M.r64.det[M.r64.nodes].astype(float))
    assert (np.abs(det / 1e-3 - 1) > 1e-6).all()
    print(f"\nD={dims} mdbc |det|: solve min {det[det >= 1e-3].min():.3g}, below threshold max {det[det < 1e-3].max():.3g}")


@pytest.mark.parametrize("dims", DIMS)
@pytest.mark.parametrize("model", MODEL_IDS)
def test_oracle_forces(model, dims):
    """forces_once (and ΣW, Σ∇W) of the oracle against the wide reference, every particle, block and ragged sizes."""
    kw = dict(MODELS)[model]
    ragged = sizes_keys("forces", dims, **kw)
    for n in (None,) + mr.RAGGED:
        K = mr.key("forces", dims, n, **kw)
        R = mr.reference(K)
        o = oracle_of(R)
        drho, acc = o.forces_once()
        kern, kgrad = o.kernel_output()
        drho, acc, kern, kgrad = by_id(o, drho, acc, kern, kgrad)
        o.close()
        for name, got in (("drho", drho), ("acc", acc), ("kernel", kern), ("kernel_gradient", kgrad)):
            Q = R.Q[name] if n is None else mr.group_q(ragged, name)
            mr.check(name, got, R.fields[name], R.A[name], Q, label=f"oracle forces D={dims} {model} n={len(R.p)}")


@pytest.mark.parametrize("dims", DIMS)
@pytest.mark.parametrize("model", [m for m, _ in STEP_MODELS] + ["negative-density"])
def test_oracle_step(model, dims):
    """One predictor-corrector step of the oracle (the shifted FullTimeStep for the first combination) against the wide reference;
    `negative-density`: the layout whose planted rows put 20 and more Fluid rows on the A_FSC < 0 side of :668."""
    R = mr.reference(mr.key("step-negative", dims, visc="LaminarSPS", ddt="ZeroDensityDiffusion", shifting=True) if model == "negative-density"
                     else mr.key("step", dims, **dict(MODELS)[model]))
    o = oracle_of(R)
    pr = o.advance(1e9, max_steps=1)
    assert pr.last_dt == pytest.approx(R.r64.dt, rel=1e-14)
    st = o.download(("ID", "Position", "Velocity", "Density"))
    st["kernel"], st["kernel_gradient"] = o.kernel_output()
    order = np.argsort(st["ID"], kind="stable")
    o.close()
    for name in mr.FIELDS + ("kernel", "kernel_gradient"):
        mr.check(name, st[name][order], R.fields[name], R.A[name], R.Q[name], label=f"oracle step D={dims} {model}")


@pytest.mark.parametrize("dims", DIMS)
@pytest.mark.parametrize("kind", ["mdbc", "mdbc-negative"])
def test_oracle_mdbc(kind, dims):
    """The boundary densities after forces_once(apply_mdbc=True): which branch of ApplyMDBCCorrection every node took, and its value.
    `mdbc-negative`: the layout with 20 and more nodes at det ≤ −1e-3, which :611 sends through the solve."""
    R = mr.reference(mr.key(kind, dims))
    o = oracle_of(R)
    o.forces_once(apply_mdbc=True)
    rho, = by_id(o, o.download(("Density",))["Density"])
    o.close()
    b = R.r64.branch
    for code in (mr.SKIPPED, mr.UNTOUCHED):
        assert np.array_equal(rho[b == code], R.st.rho[b == code])
    assert (rho[(b == mr.SOLVE) | (b == mr.SHEPARD)] != R.st.rho[(b == mr.SOLVE) | (b == mr.SHEPARD)]).all()
    mr.check("Density", rho, R.fields["Density"], R.A["Density"], R.Q["Density"], label=f"oracle {kind} D={dims}")
    print(f"branch shares D={dims}: " + ", ".join(f"{n_}={int((b[R.st.type != 1] == c).sum())}" for n_, c in
                                                  (("skipped", mr.SKIPPED), ("solve", mr.SOLVE), ("shepard", mr.SHEPARD), ("untouched", mr.UNTOUCHED))))


# mutant → (kind, what it is shown on, the compared field, the dims it can show in)
MUTANT_CASES = {
    "sps_trace_over_D": ("forces", dict(visc="LaminarSPS", ddt="ZeroDensityDiffusion"), "sps", (2,)),          # 1/D = 1/3 in 3-D
    "no_blin": ("forces", dict(visc="LaminarSPS", ddt="ZeroDensityDiffusion"), "sps", DIMS),
    "cubic_outer_branch": ("forces", dict(visc="ZeroViscosity", ddt="ZeroDensityDiffusion", kernel="CubicSpline"), "drho", DIMS),
    "tensile_W_of_dx_over_h": ("forces", dict(visc="ZeroViscosity", ddt="ZeroDensityDiffusion", kernel="CubicSpline"), "tensile", DIMS),
    "divr_rho_swapped": ("step", dict(visc="LaminarSPS", ddt="LinearDensityDiffusion", shifting=True), "Position", DIMS),
    "no_mlcond_shifting": ("step", dict(visc="LaminarSPS", ddt="LinearDensityDiffusion", shifting=True), "Position", DIMS),
    "no_mlcond_linear": ("forces", dict(visc="ZeroViscosity", ddt="LinearDensityDiffusion"), "diffusion", DIMS),
    "laminar_brackets": ("forces", dict(visc="Laminar", ddt="ZeroDensityDiffusion"), "viscosity", DIMS),
    "complex_as_linear": ("forces", dict(visc="ZeroViscosity", ddt="ComplexDensityDiffusion"), "diffusion", DIMS),
    "mdbc_shepard_rho0": ("mdbc", {}, "Density", DIMS),
    "mdbc_signed_det": ("mdbc-negative", {}, "Density", DIMS),
}


@pytest.mark.parametrize("mutant", mr.MUTANTS)
def test_mutants_leave_the_bar(mutant):
    """Every named misreading moves at least one particle of its layout by more than 10 × the bar the tests apply to that term."""
    kind, kw, name, dims_ = MUTANT_CASES[mutant]
    for dims in dims_:
        R = mr.reference(mr.key(kind, dims, **kw))
        fn = {"forces": mr.forces, "step": mr.step, "mdbc": mr.mdbc}[kind.split("-")[0]]
        m = fn(R.cfg, R.st, mutant=mutant)
        got = {"forces": lambda: mr.record_fields(m)[name], "step": lambda: m.fields[name], "mdbc": lambda: m.rho}[kind.split("-")[0]]()
        A, Q = R.A[name], R.Q[name]
        if name in mr.ISOLATION_BASE:                          # the bar tests/test_model_reference_gpu.py applies to an ISOLATED term
            _, _, _, A, Q = mr.isolated(dims, name, **kw)
        moved = mr.ratio(got - R.fields[name], mr.U * A)
        bar = mr.FACTOR * Q
        rows = int((np.abs(np.asarray(got - R.fields[name], dtype=float)) > 10 * bar * mr.U * np.broadcast_to(A.T, np.shape(got)[::-1]).T).reshape(len(A), -1).any(1).sum())
        print(f"\nmutant {mutant:24s} D={dims} {name:12s} moved/S={moved:10.3g} bar 4Q={bar:7.3f} ratio={moved / bar:10.3g} rows beyond 10 bars={rows}")
        assert bar > 0 and moved > 10 * bar, (mutant, dims, moved, bar)


@pytest.mark.parametrize("dims", DIMS)
def test_q_table(dims):
    """Q per layout, field and term (printed with -s).  A term is a chain of some ten operations of half an ulp each at the worst: a Q beyond 4
    would mean the absolute terms miss an operand that cancels."""
    for model, kw in MODELS:
        R = mr.reference(mr.key("forces", dims, **kw))
        print(f"\nQ forces D={dims} {model:24s} " + " ".join(f"{k}={v:.3f}" for k, v in R.Q.items() if v > 0))
        assert all(v <= 4.0 for v in R.Q.values()), R.Q
        assert R.Q["drho"] > 0 and R.Q["acc"] > 0
    for model, kw in STEP_MODELS:
        R = mr.reference(mr.key("step", dims, **kw))
        print(f"Q step   D={dims} {model:24s} " + " ".join(f"{k}={v:.3f}" for k, v in R.Q.items()))
        assert all(0 < v <= 4.0 for v in R.Q.values()), R.Q
    for kind in ("mdbc", "mdbc-negative"):
        R = mr.reference(mr.key(kind, dims))
        print(f"Q {kind:13s} D={dims} Density={R.Q['Density']:.3f}")
        # (volumes of both signs make some 4 × 4 systems of the 3-D negative layout ill-conditioned beyond what the componentwise A_i of the
        # solve carries: its Q is what it measures, 30 … 50, and only the ordinary layouts are held to the sanity limit)
        assert 0 < R.Q["Density"] and (kind == "mdbc-negative" or R.Q["Density"] <= 4.0)
