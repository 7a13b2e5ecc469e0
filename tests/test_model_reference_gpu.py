"""The fp64 kernels held to tests/model_reference.py per particle, for every model the C ABI covers (k_neighbor_force<…, MODEL = run time>,
k_mdbc, k_mdbc_group), directly: no oracle in between.

Bar: every compared value within FACTOR·Q·S_i of the wide (numpy.longdouble) reference, Q measured float64 against longdouble on the same
layout, reference against reference (tests/model_reference.py, tests/test_model_reference_host.py).  An isolated term — (variant − base) of two
engine runs — is held to the reference's term with the term's A_i plus the full field's.  `pytest -s` prints the figures of
profiles/model_reference.md."""
import numpy as np
import pytest

import model_reference as mr
from test_model_reference_host import DIMS, MODELS, MODEL_IDS, STEP_MODELS

pytestmark = pytest.mark.gpu

WPT = (None, "1", "2", "4", "8")


@pytest.fixture(autouse=True)
def _launch_shape(monkeypatch):
    for k in ("SPHMI_WPT", "SPHMI_WPT2_BELOW", "SPHMI_TPB", "SPHMI_TPB2", "SPHMI_MDBC_GROUP"):
        monkeypatch.delenv(k, raising=False)


def engine_of(R):
    from sphexample_amd.engine import Engine
    e = Engine(R.cfg)
    assert R.cfg.device_float_bytes == 8
    e.upload_particles(R.p)
    return e


def by_id(e, *arrays):
    order = np.argsort(e.download(("ID",))["ID"], kind="stable")
    return [a[order] for a in arrays]


def run_forces(R, kernel_output=True):
    e = engine_of(R)
    try:
        drho, acc = e.forces_once()
        out = {"drho": drho, "acc": acc}
        if kernel_output:
            out["kernel"], out["kernel_gradient"] = e.kernel_output()
        return dict(zip(out, by_id(e, *out.values())))
    finally:
        e.close()


@pytest.mark.parametrize("dims", DIMS)
@pytest.mark.parametrize("model", MODEL_IDS)
@pytest.mark.parametrize("kout", [False, True], ids=["no-kernel-output", "kernel-output"])
def test_forces(model, dims, kout):
    """forces_once of the full block, every particle, on handles without kernel output (the `!P.kout` path of the run-time-model kernel)
    and with it: then ΣW and Σ∇W of that pass from the download as well."""
    R = mr.reference(mr.key("forces", dims, kout=kout, **dict(MODELS)[model]))
    assert R.cfg.kernel_output == int(kout)
    got = run_forces(R, kernel_output=kout)
    for name in ("drho", "acc") + (("kernel", "kernel_gradient") if kout else ()):
        mr.check(name, got[name], R.fields[name], R.A[name], R.Q[name], label=f"engine forces D={dims} {model} kout={int(kout)} n={len(R.p)}")


@pytest.mark.parametrize("dims", DIMS)
@pytest.mark.parametrize("wpt", WPT)
@pytest.mark.parametrize("model", ["sps+linear+shifting", "cubic+artificial+linear", "k1.500"])
def test_forces_for_every_launch_shape(model, wpt, dims, monkeypatch):
    """The block and the ragged sizes for every $SPHMI_WPT, forces_once only: the reference does not depend on the setting."""
    if wpt is not None:
        monkeypatch.setenv("SPHMI_WPT", wpt)
    kw = dict(MODELS)[model]
    ragged = [mr.key("forces", dims, n, **kw) for n in mr.RAGGED]
    for n in (None,) + mr.RAGGED:
        R = mr.reference(mr.key("forces", dims, n, **kw))
        got = run_forces(R, kernel_output=False)
        for name in ("drho", "acc"):
            Q = R.Q[name] if n is None else mr.group_q(ragged, name)
            mr.check(name, got[name], R.fields[name], R.A[name], Q, label=f"engine wpt={wpt} D={dims} {model} n={len(R.p)}")


@pytest.mark.parametrize("dims", DIMS)
@pytest.mark.parametrize("model", [m for m, _ in STEP_MODELS])
def test_one_step(model, dims):
    """One predictor-corrector step (the shifted FullTimeStep for the first combination): Position, Velocity, Density, and the kernel output
    of its last neighbour pass from the download."""
    R = mr.reference(mr.key("step", dims, **dict(MODELS)[model]))
    e = engine_of(R)
    try:
        pr = e.advance(1e9, max_steps=1)
        st = e.download(("ID", "Position", "Velocity", "Density"))
        st["kernel"], st["kernel_gradient"] = e.kernel_output()
    finally:
        e.close()
    assert pr.last_dt == pytest.approx(R.r64.dt, rel=1e-14)
    order = np.argsort(st["ID"], kind="stable")
    for name in mr.FIELDS + ("kernel", "kernel_gradient"):
        mr.check(name, st[name][order], R.fields[name], R.A[name], R.Q[name], label=f"engine step D={dims} {model}")


@pytest.mark.parametrize("dims", DIMS)
@pytest.mark.parametrize("group", [None, "0", "1"])
def test_mdbc_densities(group, dims, monkeypatch):
    """The boundary densities after forces_once(apply_mdbc=True) for the engine's choice of kernel, k_mdbc ($SPHMI_MDBC_GROUP=0) and the
    sixteen-lane k_mdbc_group (=1): the branch of ApplyMDBCCorrection per node (skipped and untouched rows keep their bits) and the value."""
    if group is not None:
        monkeypatch.setenv("SPHMI_MDBC_GROUP", group)
    R = mr.reference(mr.key("mdbc", dims))
    e = engine_of(R)
    try:
        e.forces_once(apply_mdbc=True)
        rho, = by_id(e, e.download(("Density",))["Density"])
    finally:
        e.close()
    b = R.r64.branch
    for code in (mr.SKIPPED, mr.UNTOUCHED):
        assert np.array_equal(rho[b == code], R.st.rho[b == code]), code
    mr.check("Density", rho, R.fields["Density"], R.A["Density"], R.Q["Density"], label=f"engine mdbc group={group} D={dims}")


ISOLATED = [("Laminar/Zero", "viscosity", dict(visc="Laminar", ddt="ZeroDensityDiffusion")),
            ("LaminarSPS/Laminar", "sps", dict(visc="LaminarSPS", ddt="ZeroDensityDiffusion")),
            ("CubicSpline eps 0.3/0", "tensile", dict(visc="ZeroViscosity", ddt="ZeroDensityDiffusion", kernel="CubicSpline", eps=0.3))] + \
           [(d + "/Zero", "diffusion", dict(visc="ZeroViscosity", ddt=d)) for d in mr.DIFFUSIONS[1:]]


@pytest.mark.parametrize("dims", DIMS)
@pytest.mark.parametrize("case", ISOLATED, ids=[c[0] for c in ISOLATED])
def test_isolated_terms(case, dims):
    """(variant − base) of two engine runs against the reference's term for that variant, with the bar of the TERM: its own A_i plus the full
    field's (the rounding of the two sums that are subtracted) — a small term is not hidden behind the pressure gradient.  Q is measured on the
    compared quantity itself: (variant − base) of the float64 reference against the wide term, over the same S (model_reference.isolated)."""
    label, term, kw = case
    V, B, field, A, Q = mr.isolated(dims, term, kout=False, **kw)
    got = run_forces(V, False)[field] - run_forces(B, False)[field]
    mr.check(term, got, V.fields[term], A, Q, label=f"engine isolated D={dims} {label}")
