"""Host side of the moment sampler (sphmi_sample_point_moments, csrc/sphmi_point_moments.h): the reference enumeration
`brute_force_point_moments` pinned by closed forms; `linear_fit` of sphexample_amd/fields.py — exact for a linear field on one-sided,
irregular supports where the Shepard quotient is not, and falling back where the support cannot carry a plane; the prototype, its
export and its bindings; the RunSimulation plumbing with a stand-in backend; and what the built code object says about the kernel.
No GPU.

The sums, per point x, over the rows j with Type == Fluid and r² = ((dx² + dy²) + dz²) ≤ H², w_j = (m0 / ρ_j) W(r), e_j = x_j − x:
    n = rows    S = Σ w    SP = Σ w P    Sρ = Σ w ρ    Sv[a] = Σ w v[a]
    M1[b] = Σ w e[b]    M2[b][c] = Σ w e[b] e[c]    P1[b] = Σ w P e[b]    R1[b] = Σ w ρ e[b]    V1[a][b] = Σ w v[a] e[b]
(W as in tests/test_point_gradients_host.py.)

Bars of the linear-exactness test: the fitted value and the fitted gradient (times h) within 1e-9 of the field's range over the
point's support — fp64 solves of systems whose reciprocal condition number the test asserts to be above LINEAR_FIT_MIN_RCOND; the
Shepard quotient on the same inputs misses by more than 100 times that."""
import copy
import ctypes as C
import os
import re
import sys
import types

import numpy as np
import pytest

from sphexample_amd import _abi
from test_field_grid_host import _StandIn, _backend, _prototype
from test_point_gradients_host import ROW, _cfg, _closed_form, gradient_cloud, kernel_w_dw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SUMS = ("S", "SP", "Srho", "Sv", "M1", "M2", "P1", "R1", "V1")
# the keys of Backend.sample_point_moments → the names of the sums
KEYS = {"weight": "S", "count": "n", "sum_pressure": "SP", "sum_density": "Srho", "sum_velocity": "Sv", "moment1": "M1", "moment2": "M2",
        "moment_pressure": "P1", "moment_density": "R1", "moment_velocity": "V1"}


# ---- the reference --------------------------------------------------------------------------------------------------------------
def brute_force_point_moments(cfg, points, pos, vel, rho, press, typ):
    """Every point against every row, O(M·N), in fp64; never calls the library.  Returns n [M] int64, S, SP, Srho [M], Sv, M1, P1,
    R1 [M, 3], M2, V1 [M, 3, 3] (M2 symmetric) and near [M]: a Fluid row of the point lies within 1e-6·H of the cut."""
    points, pos, vel = np.asarray(points, np.float64), np.asarray(pos, np.float64), np.asarray(vel, np.float64)
    M, D = points.shape
    fluid = np.asarray(typ) == 1
    x, v, d, p = pos[fluid], vel[fluid], np.asarray(rho, np.float64)[fluid], np.asarray(press, np.float64)[fluid]
    out = {"n": np.zeros(M, np.int64), "S": np.zeros(M), "SP": np.zeros(M), "Srho": np.zeros(M), "Sv": np.zeros((M, 3)), "M1": np.zeros((M, 3)),
           "M2": np.zeros((M, 3, 3)), "P1": np.zeros((M, 3)), "R1": np.zeros((M, 3)), "V1": np.zeros((M, 3, 3)), "near": np.zeros(M, bool)}
    for k in range(M):
        e = x - points[k][None, :]                                                 # x_j − x
        r2 = e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]
        if D == 3:
            r2 = r2 + e[:, 2] * e[:, 2]
        dist = np.sqrt(r2)
        out["near"][k] = (np.abs(dist - cfg.H) <= 1e-6 * cfg.H).any()
        sel = r2 <= cfg.H2
        e, dist = e[sel], dist[sel]
        w = cfg.m0 / d[sel] * kernel_w_dw(cfg, dist)[0]
        P, R, U = p[sel], d[sel], v[sel]
        out["n"][k] = sel.sum()
        out["S"][k] = w.sum(); out["SP"][k] = (w * P).sum(); out["Srho"][k] = (w * R).sum()
        out["Sv"][k, :D] = (w[:, None] * U).sum(0)
        out["M1"][k, :D] = (w[:, None] * e).sum(0)
        out["M2"][k, :D, :D] = (w[:, None, None] * e[:, :, None] * e[:, None, :]).sum(0)
        out["P1"][k, :D] = ((w * P)[:, None] * e).sum(0)
        out["R1"][k, :D] = ((w * R)[:, None] * e).sum(0)
        out["V1"][k, :D, :D] = (w[:, None, None] * U[:, :, None] * e[:, None, :]).sum(0)
    return out


def as_sums(ref, cfg, dims):
    """The enumeration's result under the keys of Backend.sample_point_moments: what `linear_fit` takes."""
    return {**{key: ref[name] for key, name in KEYS.items()}, "h": cfg.h, "dims": dims}


def _one_row(cfg, dims, point, row_at, typ=1):
    return brute_force_point_moments(cfg, np.array([point[:dims]]), np.array([row_at[:dims]]), ROW["v"][None, :dims], [ROW["rho"]], [ROW["P"]], [typ])


def _z_slots_are_zero(got):
    assert (got["Sv"][:, 2] == 0).all() and (got["M1"][:, 2] == 0).all() and (got["P1"][:, 2] == 0).all() and (got["R1"][:, 2] == 0).all()
    for q in ("M2", "V1"):
        assert (got[q][:, 2, :] == 0).all() and (got[q][:, :, 2] == 0).all(), q


@pytest.mark.parametrize("dims", [2, 3])
@pytest.mark.parametrize("kernel", [0, 1])
def test_one_row_equals_the_closed_form(dims, kernel):
    """One Fluid row at a known offset from one point: every sum is one term, written out by hand."""
    cfg = _cfg(kernel, dims)
    x = np.array([0.31, -0.12, 0.055])
    u = np.array([0.6, -0.48, 0.64])[:dims]
    u = np.pad(u / np.sqrt((u * u).sum()), (0, 3 - dims))
    for frac in (0.13, 0.4, 0.5, 0.77, 0.99):                                      # q = 0.26 … 1.98: both branches of the spline
        xj = x + frac * cfg.H * u
        got = _one_row(cfg, dims, x, xj)
        e = np.pad((xj - x)[:dims], (0, 3 - dims))
        rr = float(np.sqrt(sum(float(c) * float(c) for c in e)))
        w = cfg.m0 / ROW["rho"] * _closed_form(cfg, rr)[0]
        v = np.pad(ROW["v"][:dims], (0, 3 - dims))
        want = {"S": w, "SP": w * ROW["P"], "Srho": w * ROW["rho"], "Sv": w * v, "M1": w * e, "M2": w * e[:, None] * e[None, :],
                "P1": w * ROW["P"] * e, "R1": w * ROW["rho"] * e, "V1": w * v[:, None] * e[None, :]}
        assert got["n"].tolist() == [1] and not got["near"][0]
        for q in SUMS:
            np.testing.assert_allclose(got[q][0], want[q], rtol=4e-15, atol=0, err_msg=f"{q} at r = {frac} H")
        assert got["M1"][0] @ u > 0                                                # e points from the point to the row
        if dims == 2:
            _z_slots_are_zero(got)
    # r = 0 is legal: it counts in n and the zeroth sums and adds nothing to the moments
    got = _one_row(cfg, dims, x, x)
    assert got["n"].tolist() == [1] and got["S"][0] == pytest.approx(cfg.m0 / ROW["rho"] * cfg.alphaD, rel=1e-15)
    assert all((got[q] == 0).all() for q in ("M1", "M2", "P1", "R1", "V1"))
    # the cut is inclusive, and a row of another Type does not count
    step = np.array([1.0, 0.0, 0.0])
    assert _one_row(cfg, dims, np.zeros(3), cfg.H * step)["n"].tolist() == [1]
    assert _one_row(cfg, dims, np.zeros(3), np.nextafter(cfg.H, 1.0) * step)["n"].tolist() == [0]
    other = _one_row(cfg, dims, x, x + 0.4 * cfg.H * u, typ=2)
    assert other["n"][0] == 0 and all((other[q] == 0).all() for q in SUMS)


@pytest.mark.parametrize("dims", [2, 3])
@pytest.mark.parametrize("kernel", [0, 1])
def test_a_symmetric_pair_has_no_first_moment(dims, kernel):
    """Two equal rows at x ± d: M1 is exactly zero, M2 = 2 w d ⊗ d; with P_± = P0 ± g·d the pair gives P1 = 2 w (g·d) d."""
    cfg = _cfg(kernel, dims)
    x = np.array([0.25, -0.5, 0.125])[:dims]                                       # dyadic: x ± d is exact
    d = np.array([0.0625, 0.125, -0.03125])[:dims]
    pos = np.stack([x + d, x - d])
    assert ((pos[0] - x) == d).all() and ((pos[1] - x) == -d).all()
    gd = 40.0
    got = brute_force_point_moments(cfg, x[None, :], pos, np.zeros((2, dims)), [1000.0, 1000.0], [500.0 + gd, 500.0 - gd], [1, 1])
    w = cfg.m0 / 1000.0 * _closed_form(cfg, float(np.sqrt((d * d).sum())))[0]
    assert got["n"].tolist() == [2] and (got["M1"] == 0).all() and (got["R1"] == 0).all()
    np.testing.assert_allclose(got["M2"][0, :dims, :dims], 2 * w * d[:, None] * d[None, :], rtol=4e-15)
    assert (got["M2"][0] == got["M2"][0].T).all()
    np.testing.assert_allclose(got["P1"][0, :dims], 2 * w * gd * d, rtol=4e-15)
    np.testing.assert_allclose(got["SP"][0], 2 * w * 500.0, rtol=4e-15)
    if dims == 2:
        _z_slots_are_zero(got)


# ---- linear_fit -------------------------------------------------------------------------------------------------------------------
def _fixture(dims):
    from conftest import load_dam_break_2d, load_dam_break_3d_shipped
    p, s = load_dam_break_2d() if dims == 2 else load_dam_break_3d_shipped()
    cfg = _cfg(0, dims, h=s.SimKernel.h, k=s.SimKernel.k, dp=s.SimConstants.dx)
    return np.asarray(p.Position, np.float64)[np.asarray(p.Type) == 1][:, :dims], cfg


def _one_sided(dims, seed, count=40):
    """The Fluid rows of the shipped fixture on ONE side of an oblique plane, and `count` points ON the plane inside the fluid: every
    support is cut through its point.  Returns rows [N, D], points [count, D], the plane's unit normal (into the empty side), cfg."""
    F, cfg = _fixture(dims)
    rng = np.random.default_rng(seed)
    nrm = np.array([0.8, 0.5, 0.33166247903554])[:dims]
    nrm = nrm / np.sqrt((nrm * nrm).sum())
    mid = 0.5 * (F.min(0) + F.max(0))
    keep = F[(F - mid) @ nrm <= 0.0]
    # points on the plane: rows near it, projected onto it, moved off the lattice along it
    close = keep[np.abs((keep - mid) @ nrm) < cfg.dx]
    pts = close[rng.choice(len(close), count, replace=False)]
    pts = pts - ((pts - mid) @ nrm)[:, None] * nrm[None, :]
    return keep, pts, nrm, cfg


@pytest.mark.parametrize("linear_density", [False, True])
@pytest.mark.parametrize("dims", [2, 3])
def test_linear_fit_is_exact_for_a_linear_field_where_the_shepard_mean_is_not(dims, linear_density):
    """One-sided supports of the shipped fixtures with random volumes; f_j = a + b·x_j on P and every velocity component and — in the
    second case, where the volumes m0 / ρ_j then follow ρ instead of being random — on ρ.  The fit returns a + b·x and b; the Shepard
    quotient returns the field at the centroid of the half support."""
    from sphexample_amd.fields import LINEAR_FIT_MIN_RCOND, linear_fit
    rows, pts, nrm, cfg = _one_sided(dims, seed=5 + dims)
    rng = np.random.default_rng(41)
    coef = {"P": (2300.0, 9810.0 * (nrm + 0.3 * rng.standard_normal(dims))), "rho": (1000.0, 35.0 * (nrm + 0.3 * rng.standard_normal(dims)))}
    for a in range(dims):
        coef[f"v{a}"] = (0.4 * (a + 1), 3.0 * (nrm + 0.3 * rng.standard_normal(dims)))
    field = lambda name, X: coef[name][0] + X @ coef[name][1]                      # noqa: E731
    press = field("P", rows)
    vel = np.stack([field(f"v{a}", rows) for a in range(dims)], axis=1)
    rho = field("rho", rows) if linear_density else cfg.m0 / (cfg.dx ** dims * rng.uniform(0.5, 1.5, len(rows)))      # random volumes
    ref = brute_force_point_moments(cfg, pts, rows, vel, rho, press, np.ones(len(rows), np.uint8))
    fit = linear_fit(as_sums(ref, cfg, dims))
    assert ref["n"].min() > dims + 1 and fit["linear"].all()
    assert fit["rcond"].min() > LINEAR_FIT_MIN_RCOND                              # the conditioning the bar below relies on
    # one-sided: the centroid of every support lies a fraction of h behind the plane
    off = (ref["M1"][:, :dims] / ref["S"][:, None]) @ nrm
    assert (off < -0.15 * cfg.h).all(), off.max() / cfg.h
    got = {"P": (fit["pressure"], fit["pressure_gradient"]), "rho": (fit["density"], fit["density_gradient"])}
    for a in range(dims):
        got[f"v{a}"] = (fit["velocity"][:, a], fit["velocity_gradient"][:, a, :])
    shepard = {"P": ref["SP"] / ref["S"], "rho": ref["Srho"] / ref["S"], **{f"v{a}": ref["Sv"][:, a] / ref["S"] for a in range(dims)}}
    names = [k for k in coef if linear_density or k != "rho"]
    worst = {}
    for name in names:
        a0, b = coef[name]
        # the range of the field over every point's support
        span = np.array([np.ptp(field(name, rows[((rows - x) ** 2).sum(1) <= cfg.H2])) for x in pts])
        assert (span > 0).all()
        value, grad = got[name]
        ev = np.abs(value - field(name, pts)) / span
        eg = np.abs(grad[:, :dims] - b[None, :]).max(1) * cfg.h / span
        es = np.abs(shepard[name] - field(name, pts)) / span
        worst[name] = (ev.max(), eg.max(), es.min())
        assert ev.max() <= 1e-9 and eg.max() <= 1e-9, (name, ev.max(), eg.max())
        assert es.min() > 100 * 1e-9, (name, es.min())                             # the Shepard quotient misses, at every point
        if dims == 2:
            assert (grad[:, 2] == 0).all()
    print(f"{dims}-D, {'linear' if linear_density else 'random'} density: rcond {fit['rcond'].min():.3g} … {fit['rcond'].max():.3g}; "
          + "; ".join(f"{k}: fit {v[0]:.2g}, gradient·h {v[1]:.2g}, Shepard misses by ≥ {v[2]:.2g} of the range" for k, v in worst.items()))
    if not linear_density:
        # ρ is not linear here: the fit still reproduces a constant — and with constant weights Σ w ρ = m0 Σ W the value is S-free
        assert np.isfinite(fit["density"]).all()
    if dims == 2:
        assert (fit["velocity"][:, 2] == 0).all() and (fit["velocity_gradient"][:, 2, :] == 0).all() and (fit["velocity_gradient"][:, :, 2] == 0).all()


def _hand_support(dims, offsets, kernel=0):
    """The sums of ONE point at the origin over rows at `offsets` (in units of h), P = 100 + 7 x − 3 y (+ 2 z), ρ = 1000, v = 0."""
    cfg = _cfg(kernel, dims)
    X = np.asarray(offsets, np.float64).reshape(-1, dims) * cfg.h
    P = 100.0 + X @ np.array([7.0, -3.0, 2.0])[:dims]
    ref = brute_force_point_moments(cfg, np.zeros((1, dims)), X, np.zeros((len(X), dims)), np.full(len(X), 1000.0), P, np.ones(len(X), np.uint8))
    return ref, cfg


def test_linear_fit_falls_back_where_the_support_cannot_carry_a_plane():
    from sphexample_amd.fields import LINEAR_FIT_MIN_RCOND, MIN_GRADIENT_WEIGHT, linear_fit, linear_fit_rcond

    def fallen_back(ref, cfg, dims, **kw):
        f = linear_fit(as_sums(ref, cfg, dims), **kw)
        assert not f["linear"][0]
        for k in ("pressure_gradient", "density_gradient", "velocity_gradient"):
            assert (f[k] == 0).all(), k
        S = ref["S"][0]
        want = ref["SP"][0] / S if ref["n"][0] > 0 and S > 0 else 0.0
        assert f["pressure"][0] == want and f["density"][0] == (ref["Srho"][0] / S if want else 0.0)
        return f

    t = np.linspace(-1.5, 1.4, 9)
    # n < D + 1: three rows in 3-D, two in 2-D — however well placed
    fallen_back(*_hand_support(3, [[0.5, 0.1, 0.0], [-0.3, 0.6, 0.2], [0.1, -0.4, 0.7]]), 3)
    fallen_back(*_hand_support(2, [[0.5, 0.1], [-0.3, 0.6]]), 2)
    # all rows on one line (2-D) / in one plane (3-D), through the point or beside it: rounding noise for a smallest eigenvalue
    line = np.stack([t, 0.3 + 0.5 * t], axis=1)
    plane = np.array([[a, b, 0.2 + 0.5 * a - 0.25 * b] for a in t[::2] for b in t[1::2]])
    for dims, sup in ((2, line), (2, np.stack([t, 0.5 * t], axis=1)), (3, plane), (3, plane - [0.0, 0.0, 0.2]), (3, np.stack([t, 0.4 * t, 0.1 + 0.2 * t], axis=1))):
        ref, cfg = _hand_support(dims, sup)
        assert len(sup) >= ref["n"][0] > dims + 3 and ref["S"][0] > MIN_GRADIENT_WEIGHT
        f = fallen_back(ref, cfg, dims)
        assert f["rcond"][0] < 1e-3 * LINEAR_FIT_MIN_RCOND, f["rcond"][0]          # far below the threshold, not next to it
    # the same line with one row off it carries a plane again
    ref, cfg = _hand_support(2, np.concatenate([line, [[0.2, -0.6]]]))
    f = linear_fit(as_sums(ref, cfg, 2))
    assert f["linear"][0] and f["pressure"][0] == pytest.approx(100.0, rel=1e-12)
    np.testing.assert_allclose(f["pressure_gradient"][0], [7.0, -3.0, 0.0], rtol=1e-10)
    # S below the weight floor: a full-rank support far out, where W is small
    ring = 1.9 * np.array([[np.cos(a), np.sin(a)] for a in (0.1, 1.3, 2.9, 4.1, 5.5)])
    ref, cfg = _hand_support(2, ring)
    assert ref["n"][0] == 5 and 0 < ref["S"][0] < MIN_GRADIENT_WEIGHT and linear_fit_rcond(as_sums(ref, cfg, 2))[0] > LINEAR_FIT_MIN_RCOND
    fallen_back(ref, cfg, 2)
    # n == 0: zeros
    ref, cfg = _hand_support(2, [[3.0, 0.0], [0.0, -2.5]])
    assert ref["n"][0] == 0
    f = fallen_back(ref, cfg, 2)
    assert f["pressure"][0] == 0 and (f["velocity"] == 0).all() and f["rcond"][0] == 0
    # either side of min_rcond: the same sums, the threshold a hair above and a hair below the point's own figure
    ref, cfg = _hand_support(3, [[0.5, 0.1, 0.0], [-0.3, 0.6, 0.2], [0.1, -0.4, 0.7], [-0.6, -0.2, -0.5], [0.4, 0.5, -0.3]])
    sums = as_sums(ref, cfg, 3)
    rc = linear_fit_rcond(sums)[0]
    assert rc > LINEAR_FIT_MIN_RCOND
    above, below = linear_fit(sums, min_rcond=rc * (1 + 1e-12)), linear_fit(sums, min_rcond=rc * (1 - 1e-12))
    assert not above["linear"][0] and below["linear"][0] and linear_fit(sums, min_rcond=rc)["linear"][0]      # rcond ≥ min_rcond fits
    assert above["pressure"][0] == ref["SP"][0] / ref["S"][0] and (above["pressure_gradient"] == 0).all()
    np.testing.assert_allclose(below["pressure_gradient"][0], [7.0, -3.0, 2.0], rtol=1e-9)
    assert below["pressure"][0] == pytest.approx(100.0, rel=1e-12)
    # min_count: the caller may ask for more rows than D + 1
    assert not linear_fit(sums, min_count=6)["linear"][0] and linear_fit(sums, min_count=5)["linear"][0]


def test_the_helpers_on_the_fitted_velocity_gradient():
    from sphexample_amd.fields import divergence_linear, linear_fit, strain_rate_linear, surface_load_linear, vorticity_linear
    cfg = _cfg(0, 3)
    rng = np.random.default_rng(3)
    X = rng.uniform(-1.0, 1.0, (60, 3)) * cfg.H
    X = X[X[:, 2] <= 0.0]                                                           # one-sided
    L = np.array([[0.5, -1.5, 0.25], [2.0, 0.125, -0.75], [1.0, 0.5, -0.625]])
    vel = np.array([0.3, -0.2, 0.1]) + X @ L.T
    pts = np.array([[0.0, 0.0, 0.0], [5.0, 5.0, 5.0]])                              # the second sees nothing
    ref = brute_force_point_moments(cfg, pts, X, vel, np.full(len(X), 1000.0), 10.0 - 9810.0 * X[:, 2], np.ones(len(X), np.uint8))
    sums = as_sums(ref, cfg, 3)
    np.testing.assert_allclose(vorticity_linear(sums)[0], [L[2, 1] - L[1, 2], L[0, 2] - L[2, 0], L[1, 0] - L[0, 1]], rtol=1e-9)
    assert divergence_linear(sums)[0] == pytest.approx(np.trace(L), rel=1e-9)
    np.testing.assert_allclose(strain_rate_linear(sums)[0], 0.5 * (L + L.T), rtol=1e-9, atol=1e-12)
    assert vorticity_linear(sums).shape == (2, 3) and divergence_linear(sums).shape == (2,) and strain_rate_linear(sums).shape == (2, 3, 3)
    assert np.isnan(vorticity_linear(sums)[1]).all() and np.isnan(divergence_linear(sums)[1]) and np.isnan(strain_rate_linear(sums)[1]).all()
    np.testing.assert_array_equal(vorticity_linear(linear_fit(sums)), vorticity_linear(sums))      # the result of linear_fit is taken as it is

    class _Sampler:
        def sample_point_moments(self, positions):
            self.positions = np.array(positions)
            r = brute_force_point_moments(cfg, positions, X, vel, np.full(len(X), 1000.0), 10.0 - 9810.0 * X[:, 2], np.ones(len(X), np.uint8))
            return as_sums(r, cfg, 3)

    # one small panel in the plane z = 0 around the origin, normal +z (out of the water below it): the fitted pressure there is 10
    s = 0.05 * cfg.h
    verts, tris = np.array([[-s, -s, 0.0], [2 * s, -s, 0.0], [-s, 2 * s, 0.0]]), np.array([[0, 1, 2]])
    be = _Sampler()
    force = surface_load_linear(verts, tris, be)
    np.testing.assert_allclose(be.positions, [[0.0, 0.0, 0.0]], atol=1e-18)
    np.testing.assert_allclose(force, [0.0, 0.0, -10.0 * 4.5 * s * s], rtol=1e-9, atol=1e-12)
    force, moment = surface_load_linear(verts, tris, be, about=[0.0, 0.0, 0.0])
    assert moment.shape == (3,)


# ---- the symbol -------------------------------------------------------------------------------------------------------------------
def test_header_library_and_bindings_agree():
    text = open(os.path.join(ROOT, "include", "sphmi.h")).read()
    assert re.search(r"#define\s+SPHMI_ABI_VERSION\s+5\b", text) and _abi.ABI_VERSION == 5      # append-only: the version stays
    proto = _prototype("sphmi_sample_point_moments")
    assert proto == ["sphmi_handle*", "int64_t", "const double*", "double*", "int64_t*"] + ["double*"] * 8
    assert _prototype("sphmi_sample_points")[:5] == proto[:5] == _prototype("sphmi_sample_point_gradients")[:5]      # the calling convention of the siblings
    assert "sample_point_moments" in _abi.PROTOTYPES and _abi.PROTOTYPES["sample_point_moments"][:2] == _abi.PROTOTYPES["sample_point_gradients"][:2]
    from sphexample_amd.engine import load_library
    assert hasattr(load_library(), "sphmi_sample_point_moments")
    b = _backend(3)
    b.cfg = types.SimpleNamespace(h=0.02)
    out = b.sample_point_moments(np.arange(15.0).reshape(5, 3))
    fn = b._lib.fns["sphmi_sample_point_moments"]
    assert fn.argtypes == [C.c_void_p, C.c_int64] + [C.c_void_p] * 11 and len(fn.argtypes) == len(proto)
    assert len(fn.calls) == 1 and len(fn.calls[0]) == len(proto) and fn.calls[0][1] == 5
    assert list(out) == list(KEYS) + ["h", "dims"] and list(KEYS) == list(_abi.Backend.MOMENT_FIELDS) and (out["h"], out["dims"]) == (0.02, 3)
    assert out["weight"].shape == out["count"].shape == out["sum_pressure"].shape == out["sum_density"].shape == (5,)
    assert out["sum_velocity"].shape == out["moment1"].shape == out["moment_pressure"].shape == out["moment_density"].shape == (5, 3)
    assert out["moment2"].shape == out["moment_velocity"].shape == (5, 3, 3) and out["count"].dtype == np.int64 and out["moment2"].dtype == np.float64
    assert all(a.flags.c_contiguous for k, a in out.items() if k in KEYS)
    # the six entries xx, xy, xz, yy, yz, zz fill the symmetric matrix
    six = np.array([[11.0, 12.0, 13.0, 22.0, 23.0, 33.0]])
    np.testing.assert_array_equal(six[:, _abi.Backend._SYMMETRIC][0], [[11, 12, 13], [12, 22, 23], [13, 23, 33]])
    b2 = _backend(2)
    b2.cfg = types.SimpleNamespace(h=0.02)
    out = b2.sample_point_moments(np.zeros((0, 2)), fields=("moment2", "weight"))      # an empty cloud travels as n = 0
    assert set(out) == {"moment2", "weight", "h", "dims"} and out["moment2"].shape == (0, 3, 3)
    call = b2._lib.fns["sphmi_sample_point_moments"].calls[0]
    assert call[1] == 0 and [a is None for a in call[3:]] == [False, True, True, True, True, True, False, True, True, True]
    for bad in (lambda: b2.sample_point_moments(np.zeros((4, 3))), lambda: b2.sample_point_moments(np.zeros(4)),
                lambda: b2.sample_point_moments(np.zeros((4, 2)), fields=("vorticity",))):
        with pytest.raises(ValueError):
            bad()


def test_the_julia_shim_binds_the_symbol():
    from test_julia_shim import c_prototypes, shim_ccalls
    calls = [c for c in shim_ccalls() if c[0] == "sphmi_sample_point_moments"]
    assert len(calls) == 1 and len(calls[0][2]) == len(c_prototypes()["sphmi_sample_point_moments"][1]) == 13
    shim = open(os.path.join(ROOT, "julia", "SPHExampleMI355X.jl"), encoding="utf-8").read()
    assert shim.index("function sample_point_gradients(") < shim.index("function sample_point_moments(") < shim.index("function particle_fields(")


# ---- RunSimulation ----------------------------------------------------------------------------------------------------------------
class _MomentStandIn(_StandIn):
    def sample_point_gradients(self, positions):
        self.log.append(("sample_point_gradients", self.iteration))
        return {"weight": np.zeros(len(positions))}

    def sample_point_moments(self, positions):
        self.log.append(("sample_point_moments", self.iteration))
        n = len(positions)
        return {"weight": np.full(n, float(self.iteration)), "moment2": np.zeros((n, 3, 3)), "positions": np.array(positions)}


def test_run_simulation_hands_the_sums_to_the_callback():
    from conftest import load_dam_break_2d
    from sphexample_amd import simulation
    p, s = load_dam_break_2d()
    cloud = [[0.1, 0.2], [0.3, 0.4], [0.5, 0.6]]

    def run(**kw):
        meta = copy.deepcopy(s.SimMetaData)
        meta.SimulationTime, meta.OutputTimes = 0.002, 0.001
        got = []
        _StandIn.instances.clear()
        steps = simulation.RunSimulation(SimGeometry=None, SimMetaData=meta, SimConstants=s.SimConstants, SimKernel=s.SimKernel, SimLogger=None,
                                         SimParticles=p.copy(), SimViscosity=s.SimViscosity, SimDensityDiffusion=s.SimDensityDiffusion,
                                         backend_factory=_MomentStandIn, on_output=lambda m, pp, *extra: got.append((m.Iteration, extra)), **kw)
        return steps, got, _StandIn.instances[0]

    steps, got, eng = run(sample_point_moments=cloud)
    assert len(got) == len(steps) + 1 >= 3 and got[0] == (0, (None,))              # the call before the first step: nothing to sample yet
    for iteration, extra in got[1:]:
        assert len(extra) == 1 and extra[0]["moment2"].shape == (3, 3, 3)
        assert (extra[0]["weight"] == iteration).all() and extra[0]["positions"].tolist() == cloud      # on the state of THIS output
    seq = [e for e in eng.log if isinstance(e, tuple)]
    assert [e[0] for e in seq] == ["advance", "sample_point_moments", "download"] * len(steps)
    # behind the existing optional arguments; the default leaves the callback's arguments as they were
    _, got2, eng2 = run(sample_point_gradients=cloud, sample_point_moments=cloud)
    assert all(len(extra) == 2 for _, extra in got2) and set(got2[1][1][0]) == {"weight"} and "moment2" in got2[1][1][1]
    assert [e[0] for e in eng2.log if isinstance(e, tuple)][:4] == ["advance", "sample_point_gradients", "sample_point_moments", "download"]
    _, got3, eng3 = run()
    assert all(extra == () for _, extra in got3) and not any(e[0] == "sample_point_moments" for e in eng3.log if isinstance(e, tuple))


# ---- the code object --------------------------------------------------------------------------------------------------------------
def test_the_kernels_are_built_for_gfx950_without_scratch(tmp_path):
    """The code object's metadata: every instantiation of k_point_moments — float and double records, 2-D and 3-D, one kernel each
    with all 30 sums — has no scratch, the LDS of its siblings (within kFgLdsBytes) and at most the 256 registers of the two
    workgroups per compute unit it is declared for; with fp32 records it stays within the 128 of its siblings.  And no kernel of
    the library uses scratch."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_report
    from sphexample_amd import build
    if not os.path.exists(build.LIB):
        pytest.skip("the library is not built (python -m sphexample_amd.build)")
    lib = build.LIB
    assert hasattr(C.CDLL(lib), "sphmi_sample_point_moments")
    co = isa_report.code_object(lib, str(tmp_path))
    meta = isa_report.metadata(co)
    names = isa_report.demangle(list(meta))
    mine = {names[k]: v for k, v in meta.items() if "sphmi::k_point_moments<" in names[k]}
    want = [f"k_point_moments<{t}, {d}>" for t in ("float", "double") for d in (2, 3)]
    assert len(mine) == len(want) and all(any(w in n for n in mine) for w in want), sorted(mine)
    header = open(os.path.join(ROOT, "sphexample_amd", "csrc", "sphmi_field_grid.h"), encoding="utf-8").read()
    m = re.search(r"kFgLdsBytes\s*=\s*([^;]+);", header)
    assert m, "kFgLdsBytes is not defined in sphmi_field_grid.h"
    consts = {k: int(re.search(rf"constexpr int {k}\s*=\s*(\d+)\s*;", header).group(1)) for k in ("kFgThreads", "kFgRow")}
    lds_cap = int(eval(m.group(1).replace("(size_t)", ""), {"__builtins__": {}}, consts))      # 2 · 256 · 9 · 8 + 2 · 256 · 4 + 64
    assert lds_cap == 38976
    for d, v in sorted(mine.items()):
        print(f"{d}: {v['vgprs']} VGPRs, {v['agprs']} AGPRs, {v['sgprs']} SGPRs, {v['lds_bytes']} B LDS, {v['scratch_bytes']} B scratch")
        assert v["scratch_bytes"] == 0, (d, v)
        assert 0 < v["lds_bytes"] <= lds_cap and 4 * v["lds_bytes"] <= 160 * 1024, (d, v, lds_cap)
        assert v["vgprs"] + v["agprs"] <= (128 if "<float" in d else 256), (d, v)   # fp32 records: four waves per SIMD; declared for two
        assert v["max_flat_workgroup_size"] == 256, (d, v)
    spilling = [names[k] for k, v in meta.items() if v["scratch_bytes"] != 0]
    assert not spilling, spilling[:4]
