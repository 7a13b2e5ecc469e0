"""The fused predictor / corrector kernels at pair level: ONE step of an fp32 handle against the fp64 oracle, per particle.

`forces_once()` never launches the fused instantiations of k_neighbor_force (the own-row window, `NeighborLds::kWindow`, needs a predictor or a
corrector pass), and the K-step tests that do run them use lattices and a max-norm of 1e-5.  Here $SPHMI_WPT forces every fused instantiation
— "2" is the window kernel in 3-D, "1" the one-wave kernels, "4" and "8" the multi-wave half tiles, unset the engine's own choice — onto small,
nasty clouds (tests/fused_pair_reference.py: ragged sizes, a crowd in one cell row, a random box with permuted ids, two far clusters, particles
on cell faces, a cloud far from the origin, a second call, and the 2-D counterparts), mixed Fluid / Fixed, fp32-exact inputs.  One step shows
all four pair sums: Acceleration, Velocity and Density carry the corrector's, Pressure = Pressure!(ρₙ⁺) the predictor's dρ/dt, Position what is
left of the predictor's acceleration.

Every field of every particle has to stay within FACTOR·Q·S_i of the oracle: S_i from the absolute pair sums of the numpy reference, Q measured
reference against reference (module docstring of tests/fused_pair_reference.py; tests/test_fused_pair_scale_host.py shows that the bound bites).
No particle is exempt.  Measured figures: profiles/fused_pair_parity.md."""
import numpy as np
import pytest

import bruteforce as bf
import fused_pair_reference as fr

pytestmark = pytest.mark.gpu

WPT_3D = (None, "1", "2", "4", "8")
WPT_2D = ("2", "4", "8")
FIELDS = ("ID",) + fr.FIELDS


@pytest.fixture(autouse=True)
def _launch_shape(monkeypatch):
    for k in ("SPHMI_WPT", "SPHMI_WPT2_BELOW", "SPHMI_TPB", "SPHMI_TPB2"):
        monkeypatch.delenv(k, raising=False)


def _force(monkeypatch, wpt):
    if wpt is not None:
        monkeypatch.setenv("SPHMI_WPT", wpt)


def _within(e, ref, S, q_case, what):
    """Every field of every particle within FACTOR·Q·S_i; prints the largest normalised error per field first."""
    worst = {}
    for k in fr.FIELDS:
        s = S[k] * np.ones_like(ref[k])
        err = np.abs(e[k] - ref[k])
        assert (err[s == 0] == 0).all(), f"{what} {k}: differs where the scale is zero"
        worst[k] = float((err[s > 0] / s[s > 0]).max()) if (s > 0).any() else 0.0
    print(f"{what} Q={q_case:.3f} bound={fr.FACTOR * q_case:.3f}  " + "  ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= fr.FACTOR * q_case, f"{what} {k}: {v:.3f}·S_i against {fr.FACTOR:g}·Q = {fr.FACTOR * q_case:.3f}"


def _one_step(case, label, wpt, monkeypatch):
    from oracle.oracle import make_oracle
    from sphexample_amd.engine import make_engine
    _force(monkeypatch, wpt)
    p, s = fr.particles(case, label)
    cfg, r, S, _ = fr.first_step(case, label)
    eng, orc = make_engine(p, s, device_float_bytes=4), make_oracle(p, s)
    try:
        pe, po = eng.advance(1e9, max_steps=1), orc.advance(1e9, max_steps=1)
        assert (pe.iteration, pe.n_rebuilds) == (po.iteration, po.n_rebuilds)
        assert pe.last_dt == pytest.approx(po.last_dt, rel=1e-6)
        e, o = fr.by_id(eng.download(FIELDS)), fr.by_id(orc.download(FIELDS))
        np.testing.assert_array_equal(e["ID"], o["ID"])
        half = np.empty(len(p)); half[orc.download(("ID",))["ID"] - 1] = orc.half_step_density()
        np.testing.assert_allclose(o["Pressure"], bf.eos(cfg, half), rtol=1e-8, atol=1e-6)      # the oracle's Pressure IS Pressure!(ρₙ⁺)
        o["Pressure"] = bf.eos(cfg, half)
        _within(e, o, S, fr.case_q(case), f"{case} {label} wpt={wpt}")
    finally:
        eng.close(); orc.close()


@pytest.mark.parametrize("wpt", WPT_3D)
@pytest.mark.parametrize("n", fr.RAGGED_3D)
def test_ragged_sizes(n, wpt, monkeypatch):
    """The last tile with no target, one target or a partial set in its second half; the window clipped at 0 and at N; a workgroup whose second tile does not exist."""
    _one_step("ragged3d", f"n{n}", wpt, monkeypatch)


@pytest.mark.parametrize("wpt", WPT_3D)
@pytest.mark.parametrize("case", ["crowd3d", "box", "clusters", "faces", "offset"])
def test_clouds(case, wpt, monkeypatch):
    """crowd3d: 3 000 particles in two cells of one row (an own row longer than the 256-record window, queues that fill inside one chunk row);
    box: 6 000 random points, ≈ 94 tiles, ids a random permutation; clusters: 2 × 1 500 points 40 box-sides apart; faces: a fifth of the box
    on x = (n ± ½)·H; offset: the box shifted by (−13.7, 50, −13.7) m."""
    _one_step(case, fr.members(case)[0][0], wpt, monkeypatch)


@pytest.mark.parametrize("wpt", WPT_3D)
def test_a_second_call(wpt, monkeypatch):
    """Two calls of one step each on the box cloud: the second opens with a rebuild, the window follows a new sort.  The bound of the second
    step is re-based on the ORACLE's state after the first (the numpy reference is fed the oracle's state, never the engine's)."""
    from oracle.oracle import make_oracle
    from sphexample_amd.engine import make_engine
    _force(monkeypatch, wpt)
    p, s = fr.particles("second_call", "box")
    cfg, r1, S1, q1 = fr.first_step("second_call", "box")
    eng, orc = make_engine(p, s, device_float_bytes=4), make_oracle(p, s)
    try:
        pe, po = eng.advance(1e9, max_steps=1), orc.advance(1e9, max_steps=1)
        r2, S2, q2, _ = fr.rebased_step(cfg, orc)
        pe, po = eng.advance(1e9, max_steps=1), orc.advance(1e9, max_steps=1)
        assert (pe.iteration, pe.n_rebuilds) == (po.iteration, po.n_rebuilds) == (2, 2)
        assert pe.last_dt == pytest.approx(po.last_dt, rel=1e-6)
        e, o = fr.by_id(eng.download(FIELDS)), fr.by_id(orc.download(FIELDS))
        np.testing.assert_array_equal(e["ID"], o["ID"])
        half = np.empty(len(p)); half[orc.download(("ID",))["ID"] - 1] = orc.half_step_density()
        o["Pressure"] = bf.eos(cfg, half)
        _within(e, o, fr.carried(S1, S2, r2.dt), max(q1, q2), f"second_call box wpt={wpt}")
    finally:
        eng.close(); orc.close()


@pytest.mark.parametrize("wpt", WPT_2D)
@pytest.mark.parametrize("n", fr.RAGGED_2D)
def test_ragged_sizes_2d(n, wpt, monkeypatch):
    """The fused 2-D fp32 kernels have no window, and the same hole in the suite."""
    _one_step("ragged2d", f"n{n}", wpt, monkeypatch)


@pytest.mark.parametrize("wpt", WPT_2D)
def test_crowd_2d(wpt, monkeypatch):
    """2 300 particles in three cells of one row."""
    _one_step("crowd2d", "crowd", wpt, monkeypatch)
