"""What the layouts of tests/cutoff_edge_reference.py must be before any kernel is asked — conditions on the reference, not measurements.

Classification (every pair planted or clear; an fp32 cut that agrees with fp64), coverage (pairs per δ and side, partner classes, tile reaches) and
visibility (the loss of any planted inside pair, or the gain of any planted outside pair, moves a compared quantity of one of its particles by at
least ten tolerances).  The figures are printed (pytest -s) and recorded in profiles/cutoff_edge.md."""
import numpy as np
import pytest

import cutoff_edge_reference as ce

CASES = [(n, w) for n in ce.LAYOUTS for w in (8, 4)]


@pytest.mark.parametrize("name,width", CASES)
def test_every_pair_is_planted_or_clear(name, width):
    L = ce.layout(name, width)
    P = L.planted
    d = L.pos[P.a] - L.pos[P.b]
    q = (d * d).sum(1) / (L.H * L.H)
    assert (np.abs(q - (1 + P.side * P.delta)) <= ce.PLANT_TOL * P.delta).all()
    assert ((q < 1) == (P.side < 0)).all()
    if width == 4:
        assert (L.pos == L.pos.astype(np.float32)).all() and L.deltas[0] == pytest.approx(8 * L.e) and L.c >= 100 * L.e
    else:
        assert (L.pos != L.pos.astype(np.float32)).any(1).all()               # no position is fp32-representable
    assert set(np.unique(P.delta)) == set(L.deltas)
    a, b, qn = ce.classify(L)                                                  # every pair nearer the cut than c …
    n = len(L.pos)
    key = lambda x, y: np.minimum(x, y) * n + np.maximum(x, y)                 # noqa: E731
    assert np.isin(key(a, b), key(P.a, P.b)).all(), "a pair near the cut that nobody planted"
    assert len(np.unique(key(P.a, P.b))) == len(P.a)


@pytest.mark.parametrize("name", ce.LAYOUTS)
def test_the_fp32_cut_agrees_with_fp64(name):
    """r² ≤ H² in numpy.float32 — from absolute coordinates, and from differences to the first particle of the tile and of the half tile, each rounded
    once — decides every pair within 1.2 H as fp64 does."""
    from scipy.spatial import cKDTree
    L = ce.layout(name, 4)
    x32 = L.pos.astype(np.float32)
    H2 = np.float32(L.H * L.H)
    pr = cKDTree(L.pos).query_pairs(1.2 * L.H, output_type="ndarray")
    d = L.pos[pr[:, 0]] - L.pos[pr[:, 1]]
    inside = (d * d).sum(1) <= L.H * L.H
    r2 = lambda e: (e * e).sum(1, dtype=np.float32)                            # noqa: E731
    assert r2(x32[pr[:, 0]] - x32[pr[:, 1]]).dtype == np.float32
    np.testing.assert_array_equal(r2(x32[pr[:, 0]] - x32[pr[:, 1]]) <= H2, inside)
    for size in (64, 32):
        t = ce.tiles(L.pos, L.H, size)
        first = t.order[(t.rank // size) * size]                               # row of the first particle of every row's tile
        for tgt, oth in ((0, 1), (1, 0)):
            o = x32[first[pr[:, tgt]]]
            e = (x32[pr[:, tgt]] - o) - (x32[pr[:, oth]] - o)
            assert e.dtype == np.float32
            np.testing.assert_array_equal(r2(e) <= H2, inside)


@pytest.mark.parametrize("name,width", CASES)
def test_coverage(name, width):
    L = ce.layout(name, width)
    P = L.planted
    for delta in L.deltas:
        for side in (-1, 1):
            assert ((P.delta == delta) & (P.side == side)).sum() >= 20, (delta, side)
    cls = ce.partner_class(L)
    t64, t32 = ce.tiles(L.pos, L.H, 64), ce.tiles(L.pos, L.H, 32)
    print(f"{name} fp{8 * width} N={len(L.pos)} δ={['%.3g' % d for d in L.deltas]} c={L.c:.3g} e={L.e:.3g} pairs/band={len(P.a) // (2 * len(L.deltas))} "
          f"classes={np.bincount(cls, minlength=3).tolist()} reach64={np.sort(t64.reach).round(1).tolist()}")
    if name.startswith("box"):
        for side in (-1, 1):
            assert (np.bincount(cls[P.side == side], minlength=3) >= 5).all(), np.bincount(cls[P.side == side], minlength=3)
        assert 3.0 <= np.median(t64.reach) <= 7.0
    if name.startswith("spray"):
        for lo, hi in ce.SPRAY_REACH:
            assert ((t64.reach >= lo) & (t64.reach <= hi)).sum() >= 3, (lo, hi)
        assert len(L.pos) <= 4000
    if name == "clusters":
        far = 30 * L.info["side"] / L.H
        assert (t64.reach > far).any() and (t32.reach > far).any()
        in_far = t64.reach[t64.rank[np.concatenate([P.a, P.b])] // 64] > far
        assert in_far.any()                                                    # planted pairs among the particles of a straddling tile


@pytest.mark.parametrize("name,width", CASES)
def test_a_planted_pair_cannot_go_unseen(name, width):
    f = ce.forces(name, width)
    L = ce.layout(name, width)
    assert (f.inside_listed == (L.planted.side < 0)).all()                    # the reference takes the inside pairs and leaves the outside ones
    t = f.terms
    assert (t.t_drho_i != 0).all() and (t.t_drho_j != 0).all() and (np.abs(t.t_acc).max(1) > 0).all()        # continuity and pressure terms are there
    v = ce.visible(name, width)
    print(f"{name} fp{8 * width} Q(forces)={f.q:.3f} least visible planted pair: {v.min():.3g} tolerances, velocities drawn again: {L.redrawn}")
    assert (v >= ce.VISIBLE).all()


@pytest.mark.parametrize("name", ce.LAYOUTS)
def test_an_fp32_step_can_be_held_on_every_layout(name):
    """The CORRECTOR runs on x⁺: no pair with a Fluid particle lies within the fp32 error of r² of the cut there (such a pair would be decided by
    rounding, whatever the mask does), and Q of the step — the fp32 restatement against the fp64 one on this layout — is measured and finite."""
    n, e = ce.half_step_near_cut(name, 4)
    cfg, r64, S, q = ce.one_step(name, 4)
    print(f"{name} fp32: pairs of x⁺ within {e:.3g} of the cut: {n}; corrector pairs {r64.p2.npairs}; Q(step) = {q:.3f}")
    assert n == 0
    assert np.isfinite(q) and q > 0
    assert (r64.fields["Density"] > 0).all() and (r64.rho_h > 0).all()        # a step the engine does not refuse


@pytest.mark.parametrize("name,width", CASES)
def test_rows_are_permuted(name, width):
    """A satellite comes before its anchor in upload order (and so inside a cell, and in the i/j orientation) about as often as after it."""
    L = ce.layout(name, width)
    first = (L.planted.b < L.planted.a).mean()
    assert 0.3 < first < 0.7


def test_why_there_is_no_stale_member():
    """The box after one step: the pairs of two Fixed particles stay planted, every other planted pair leaves its band, and pairs that nobody
    planted land nearer the cut than c — the stepped state cannot be classified into planted and clear.  (tests/test_cutoff_edge_gpu.py still runs
    a second step on it with fp64 handles, where a pair decided by rounding is a 1e-16 event.)"""
    L = ce.layout("box", 8)
    least, still, strangers, median = ce.stale_report()
    fixed_pairs = int(((np.asarray(L.p.Type)[L.planted.a] != 1) & (np.asarray(L.p.Type)[L.planted.b] != 1)).sum())
    print(f"stale: planted pairs still in their band after one step: {still} (pairs of two Fixed particles: {fixed_pairs}); "
          f"unplanted pairs nearer the cut than c: {strangers}; median move of r²/H²: {median:.3g}")
    assert still == fixed_pairs
    assert strangers > 0
