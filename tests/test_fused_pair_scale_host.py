"""The per-particle bound of tests/test_fused_pair_parity_gpu.py has to BITE: checked here from the reference side alone (numpy pair sums in fp64 and
in fp32, tests/fused_pair_reference.py; the fp64 oracle where a second step is re-based on it), before any kernel is asked.

For every case: Q, the constant measured reference against reference; the share of the pairs with q ≤ 1.5 whose loss from the sums would put at
least one partner outside FACTOR·Q·S_i in at least one field (≥ 95 %); the smallest q from which on a single pair can go unseen.  The figures
are printed (pytest -s) and recorded in profiles/fused_pair_parity.md."""
import numpy as np
import pytest

import fused_pair_reference as fr

MIN_SHARE = 0.95
Q_NEAR = 1.5


def _report(case, label, q_case, cfg, r, S):
    q, s1, s2, su = fr.visibility(cfg, r, S, q_case)
    near = q <= Q_NEAR
    share = lambda s: float(s[near].mean()) if near.any() else 1.0          # noqa: E731
    unseen = float(q[~su].min()) if (~su).any() else float("nan")
    print(f"{case:12s} {label:9s} N={len(S['Density']):5d} Q_case={q_case:.3f} pairs(q<=1.5)={int(near.sum()):8d} seen: predictor {share(s1):.4f} "
          f"corrector {share(s2):.4f} either {share(su):.4f}  smallest unseen q {unseen:.3f}")
    return int(su[near].sum()), int(near.sum())


@pytest.mark.parametrize("case", [c for c in fr.CASES if c != "second_call"])
def test_a_lost_pair_leaves_the_bound(case):
    q_case = fr.case_q(case)
    assert np.isfinite(q_case) and q_case > 0
    seen = total = 0
    for label, _ in fr.members(case):
        cfg, r, S, q = fr.first_step(case, label)
        assert q <= q_case
        assert (r.fields["Density"] > 0).all() and (r.rho_h > 0).all()            # the step is one the engine does not refuse
        a, b = _report(case, label, q_case, cfg, r, S)
        seen += a; total += b
    assert total > 0 and seen >= MIN_SHARE * total, (case, seen, total)


def test_a_lost_pair_leaves_the_bound_of_a_second_call():
    """The box cloud after one step of the oracle: the second call's step restated from the oracle's state, its scale added to the first's."""
    from oracle.oracle import make_oracle
    p, s = fr.particles("second_call", "box")
    cfg, r1, S1, q1 = fr.first_step("second_call", "box")
    orc = make_oracle(p, s)
    try:
        po = orc.advance(1e9, max_steps=1)
        assert po.last_dt == pytest.approx(r1.dt, rel=1e-12)
        o = fr.by_id(orc.download())
        for k in ("Velocity", "Density", "Position", "Acceleration"):              # the restatement IS the oracle's step, to fp64 rounding
            np.testing.assert_allclose(r1.fields[k], o[k], rtol=0, atol=1e-9 * np.abs(o[k]).max(), err_msg=k)
        np.testing.assert_allclose(r1.fields["Pressure"], o["Pressure"], rtol=0, atol=1e-9 * np.abs(o["Pressure"]).max() + 1e-6)
        r2, S2, q2, _ = fr.rebased_step(cfg, orc)
    finally:
        orc.close()
    q_case = max(q1, q2)
    S = fr.carried(S1, S2, r2.dt)
    # the second step's pairs against the carried scales; r2's rows are the oracle's, the scales are by ID (IDs are 1 … N)
    st_ids = r2.ids
    S_rows = {k: v[st_ids - 1] for k, v in S.items()}
    seen, total = _report("second_call", "box", q_case, cfg, r2, S_rows)
    print(f"second_call  Q first step {q1:.3f}, second step {q2:.3f}")
    assert seen >= MIN_SHARE * total
    assert q2 <= 10 * q1
