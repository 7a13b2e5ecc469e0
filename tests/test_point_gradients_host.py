"""Host side of the gradient sampler (sphmi_sample_point_gradients, csrc/sphmi_point_gradients.h): the reference enumeration
`brute_force_point_gradients` pinned by closed forms; the helpers of sphexample_amd/fields.py on hand-made sums; the prototype, its
export and its bindings; the RunSimulation plumbing with a stand-in backend; and what the built code object says about the kernel.
No GPU.

The sums, per point x, over the rows j with Type == Fluid and r² = ((dx² + dy²) + dz²) ≤ H²:
    V_j = m0 / ρ_j      g_j = W′(r) · (x − x_j) / r   (0 at r = 0)
    n = rows    S = Σ V_j W    SP = Σ V_j P_j W    Sρ = Σ V_j ρ_j W    Sv[a] = Σ V_j v_j[a] W
    G[b] = Σ V_j g_j[b]    GP[b] = Σ V_j P_j g_j[b]    Gρ[b] = Σ V_j ρ_j g_j[b]    Gv[a][b] = Σ V_j v_j[a] g_j[b]
W: Wendland C2, αD (1 − q/2)⁴ (2q + 1), W′ = −5 αD q (1 − q/2)³ / h; CubicSpline, αD (1 − 3/2 q² + 3/4 q³) for q ≤ 1 and
αD (2 − q)³ / 4 for 1 < q ≤ 2, W′ = αD (−3 q + 9/4 q²) / h and −3/4 αD (2 − q)² / h; q = r / h."""
import copy
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

from sphexample_amd import _abi
from test_field_grid_host import _StandIn, _backend, _prototype

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SUMS = ("S", "SP", "Srho", "Sv", "G", "GP", "Grho", "Gv")
# the keys of Backend.sample_point_gradients → the names of the sums
KEYS = {"weight": "S", "count": "n", "sum_pressure": "SP", "sum_density": "Srho", "sum_velocity": "Sv", "grad_weight": "G",
        "grad_pressure": "GP", "grad_density": "Grho", "grad_velocity": "Gv"}
IRR = np.array([0.318309886, 0.577215665, 0.693147181])            # offsets in units of dp: nothing the particle lattice knows


# ---- the reference --------------------------------------------------------------------------------------------------------------
def kernel_w_dw(cfg, r):
    """W(r) and W′(r) of the handle's kernel (the module docstring); cfg.kernel: 0 Wendland C2, 1 CubicSpline."""
    r = np.asarray(r, dtype=np.float64)
    q = r * cfg.h_inv
    if cfg.kernel == 1:
        inner, outer = q <= 1, (q > 1) & (q <= 2)
        W = cfg.alphaD * ((1 - 1.5 * q ** 2 + 0.75 * q ** 3) * inner + 0.25 * (2 - q) ** 3 * outer)
        dW = cfg.alphaD * cfg.h_inv * ((-3 * q + 2.25 * q ** 2) * inner - 0.75 * (2 - q) ** 2 * outer)
        return W, dW
    return cfg.alphaD * (1 - q / 2) ** 4 * (2 * q + 1), -5 * cfg.alphaD * cfg.h_inv * q * (1 - q / 2) ** 3


def brute_force_point_gradients(cfg, points, pos, vel, rho, press, typ):
    """Every point against every row, O(M·N), in fp64; never calls the library.  Returns n [M] int64, S, SP, Srho [M], Sv, G, GP,
    Grho [M, 3], Gv [M, 3, 3] and near [M]: a Fluid row of the point lies within 1e-6·H of the cut."""
    points, pos, vel = np.asarray(points, np.float64), np.asarray(pos, np.float64), np.asarray(vel, np.float64)
    M, D = points.shape
    fluid = np.asarray(typ) == 1
    x, v, d, p = pos[fluid], vel[fluid], np.asarray(rho, np.float64)[fluid], np.asarray(press, np.float64)[fluid]
    out = {"n": np.zeros(M, np.int64), "S": np.zeros(M), "SP": np.zeros(M), "Srho": np.zeros(M), "Sv": np.zeros((M, 3)), "G": np.zeros((M, 3)),
           "GP": np.zeros((M, 3)), "Grho": np.zeros((M, 3)), "Gv": np.zeros((M, 3, 3)), "near": np.zeros(M, bool)}
    for k in range(M):
        e = points[k][None, :] - x
        r2 = e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]
        if D == 3:
            r2 = r2 + e[:, 2] * e[:, 2]
        dist = np.sqrt(r2)
        out["near"][k] = (np.abs(dist - cfg.H) <= 1e-6 * cfg.H).any()
        sel = r2 <= cfg.H2
        e, dist = e[sel], dist[sel]
        V, P, R, U = cfg.m0 / d[sel], p[sel], d[sel], v[sel]
        W, dW = kernel_w_dw(cfg, dist)
        g = np.where(dist[:, None] > 0, dW[:, None] * e / np.where(dist > 0, dist, 1.0)[:, None], 0.0)      # W′(r) (x − x_j) / r, nothing at r = 0
        out["n"][k] = sel.sum()
        out["S"][k] = (V * W).sum(); out["SP"][k] = (V * P * W).sum(); out["Srho"][k] = (V * R * W).sum()
        out["Sv"][k, :D] = ((V * W)[:, None] * U).sum(0)
        out["G"][k, :D] = (V[:, None] * g).sum(0)
        out["GP"][k, :D] = ((V * P)[:, None] * g).sum(0)
        out["Grho"][k, :D] = ((V * R)[:, None] * g).sum(0)
        out["Gv"][k, :D, :D] = (V[:, None, None] * U[:, :, None] * g[:, None, :]).sum(0)
    return out


def gradient_cloud(F, H, dx, seed=7, count=700):
    """`count` points uniform over the box of the Fluid rows F widened by 0.9·H, offset by the irregular IRR·dx."""
    F = np.asarray(F, np.float64)
    D = F.shape[1]
    rng = np.random.default_rng(seed)
    return rng.uniform(F.min(0) - 0.9 * H, F.max(0) + 0.9 * H, (count, D)) + IRR[:D] * dx


class _Cfg:
    pass


def _cfg(kernel, dims, h=0.13, k=2.0, dp=0.1):
    cfg = _Cfg()
    cfg.h, cfg.h_inv, cfg.H, cfg.kernel, cfg.m0, cfg.dx = h, 1 / h, k * h, kernel, 1000 * dp ** dims, dp
    cfg.H2 = cfg.H * cfg.H
    cfg.alphaD = {(0, 2): 7 / (4 * np.pi * h ** 2), (0, 3): 21 / (16 * np.pi * h ** 3), (1, 2): 10 / (7 * np.pi * h ** 2), (1, 3): 1 / (np.pi * h ** 3)}[(kernel, dims)]
    return cfg


def _closed_form(cfg, r):
    """W and W′ at one distance, in scalar arithmetic with the polynomials written out."""
    q = r / cfg.h
    if cfg.kernel == 1:
        if q <= 1:
            return cfg.alphaD * (1 - 1.5 * q * q + 0.75 * q * q * q), cfg.alphaD * (-3 * q + 2.25 * q * q) / cfg.h
        return cfg.alphaD * 0.25 * (2 - q) * (2 - q) * (2 - q), -0.75 * cfg.alphaD * (2 - q) * (2 - q) / cfg.h
    t = 1 - q / 2
    return cfg.alphaD * t * t * t * t * (2 * q + 1), -5 * cfg.alphaD * q * t * t * t / cfg.h


ROW = {"rho": 1013.0, "P": 2750.0, "v": np.array([0.7, -1.9, 0.4])}


def _one_row(cfg, dims, point, row_at, typ=1):
    return brute_force_point_gradients(cfg, np.array([point[:dims]]), np.array([row_at[:dims]]), ROW["v"][None, :dims], [ROW["rho"]], [ROW["P"]], [typ])


@pytest.mark.parametrize("dims", [2, 3])
@pytest.mark.parametrize("kernel", [0, 1])
def test_one_row_equals_the_closed_form(dims, kernel):
    """One Fluid row at distance r from one point: every sum is one term."""
    cfg = _cfg(kernel, dims)
    x = np.array([0.31, -0.12, 0.055])
    u = np.array([0.6, -0.48, 0.64])[:dims]
    u = np.pad(u / np.sqrt((u * u).sum()), (0, 3 - dims))
    for frac in (0.13, 0.4, 0.5, 0.77, 0.99):                                      # q = 0.26 … 1.98: both branches of the spline
        r = frac * cfg.H
        xj = x - r * u                                                             # x − x_j = r u
        got = _one_row(cfg, dims, x, xj)
        e = (x - xj)[:dims]
        rr = math.sqrt(sum(float(c) * float(c) for c in e))
        W, dW = _closed_form(cfg, rr)
        V = cfg.m0 / ROW["rho"]
        g = np.pad(dW * e / rr, (0, 3 - dims))
        v = np.pad(ROW["v"][:dims], (0, 3 - dims))
        want = {"S": V * W, "SP": V * ROW["P"] * W, "Srho": V * ROW["rho"] * W, "Sv": V * W * v, "G": V * g, "GP": V * ROW["P"] * g,
                "Grho": V * ROW["rho"] * g, "Gv": V * v[:, None] * g[None, :]}
        assert got["n"].tolist() == [1] and not got["near"][0]
        for q in SUMS:
            np.testing.assert_allclose(got[q][0], want[q], rtol=4e-15, atol=0, err_msg=f"{q} at r = {frac} H")
        assert got["G"][0] @ u < 0                                                 # W falls with r: ∇W points from the point to the row's far side
        if dims == 2:
            assert got["Sv"][0, 2] == 0 and (got["G"][0, 2], got["GP"][0, 2], got["Grho"][0, 2]) == (0, 0, 0)
            assert (got["Gv"][0, 2, :] == 0).all() and (got["Gv"][0, :, 2] == 0).all()
    # a row of another Type does not count
    other = _one_row(cfg, dims, x, x - 0.4 * cfg.H * u, typ=2)
    assert other["n"][0] == 0 and all((other[q] == 0).all() for q in SUMS)


@pytest.mark.parametrize("dims", [2, 3])
@pytest.mark.parametrize("kernel", [0, 1])
def test_a_row_at_r_zero_and_rows_at_the_cut(dims, kernel):
    cfg = _cfg(kernel, dims)
    x = np.array([0.31, -0.12, 0.055])
    # r = 0: counts in n and the S sums (W(0) = αD for both kernels), adds nothing to the G sums
    got = _one_row(cfg, dims, x, x)
    V = cfg.m0 / ROW["rho"]
    assert got["n"].tolist() == [1]
    assert got["S"][0] == pytest.approx(V * cfg.alphaD, rel=1e-15) and got["SP"][0] == pytest.approx(V * ROW["P"] * cfg.alphaD, rel=4e-16)
    for q in ("G", "GP", "Grho", "Gv"):
        assert (got[q] == 0).all() and np.isfinite(got[q]).all(), q
    # just inside and just outside H, along one axis so that r² is one product: in by the inclusive cut, out beyond it
    for axis in range(dims):
        step = np.zeros(3); step[axis] = 1.0
        origin = np.zeros(3)
        inside = _one_row(cfg, dims, origin, -cfg.H * step)                        # r² == H² exactly: in
        assert inside["n"].tolist() == [1] and inside["near"][0]
        assert abs(inside["S"][0]) <= 1e-30 and np.abs(inside["G"]).max() <= 1e-12 * cfg.alphaD / cfg.h      # W(H) = W′(H) = 0 for both kernels
        a_bit_in = _one_row(cfg, dims, origin, -cfg.H * (1 - 1e-9) * step)
        assert a_bit_in["n"].tolist() == [1] and a_bit_in["near"][0]
        out = _one_row(cfg, dims, origin, -np.nextafter(cfg.H, 1.0) * step)
        assert out["n"].tolist() == [0] and out["near"][0] and all((out[q] == 0).all() for q in SUMS)
        far = _one_row(cfg, dims, origin, -1.5 * cfg.H * step)
        assert far["n"].tolist() == [0] and not far["near"][0]


@pytest.mark.parametrize("dims", [2, 3])
@pytest.mark.parametrize("kernel", [0, 1])
def test_on_a_lattice_the_corrected_form_returns_a_linear_field(dims, kernel):
    """On a node of a uniform lattice of equal density the neighbourhood is symmetric: G = 0, and the Shepard-corrected difference
    form of the fields helpers returns the gradient of a linear field to the lattice's accuracy (Σ V g ⊗ (x_j − x) ≈ −1)."""
    from sphexample_amd.fields import divergence_at, pressure_gradient, strain_rate, velocity_gradient, vorticity_at
    cfg = _cfg(kernel, dims)
    ax = np.arange(-6, 7) * cfg.dx
    pos = np.stack(np.meshgrid(*[ax] * dims, indexing="ij"), -1).reshape(-1, dims)
    b = np.array([3.0, -2.0, 0.5])[:dims]
    A = np.array([[0.5, -1.5, 0.25], [2.0, 0.125, -0.75], [1.0, 0.5, -0.625]])[:dims, :dims]
    press, vel = 7.0 + pos @ b, 1.0 + pos @ A.T
    r = brute_force_point_gradients(cfg, np.zeros((1, dims)), pos, vel, np.full(len(pos), 1000.0), press, np.ones(len(pos), np.uint8))
    assert r["n"][0] > 8 and np.abs(r["G"]).max() <= 1e-12 * r["S"][0] / cfg.h
    sums = {key: r[name] for key, name in KEYS.items()}
    # the discrete moment −Σ V g_b (x_j − x)_b of the lattice, per axis the same by symmetry: what the lattice makes of "1"
    off = pos[(pos ** 2).sum(1) <= cfg.H2]
    rr = np.sqrt((off ** 2).sum(1))
    dW = kernel_w_dw(cfg, rr)[1]
    moment = (cfg.m0 / 1000.0) * (np.where(rr > 0, dW / np.where(rr > 0, rr, 1.0), 0.0) * off[:, 0] ** 2).sum() / r["S"][0]
    assert -1.1 < moment < -0.9
    L = velocity_gradient(sums)
    np.testing.assert_allclose(L[0, :dims, :dims], -moment * A, rtol=1e-11, atol=1e-11)
    np.testing.assert_allclose(pressure_gradient(sums)[0, :dims], -moment * b, rtol=1e-11, atol=1e-11)
    assert divergence_at(sums)[0] == pytest.approx(-moment * np.trace(A), rel=1e-11)
    np.testing.assert_allclose(strain_rate(sums)[0, :dims, :dims], -moment * 0.5 * (A + A.T), rtol=1e-11, atol=1e-11)
    assert vorticity_at(sums)[0, 2] == pytest.approx(-moment * (A[1, 0] - A[0, 1]), rel=1e-11)


def test_the_cap_on_points_at_the_cut_holds_for_the_chosen_seed():
    """The GPU test excuses a count on fp32 handles only where the enumeration shows a row within 1e-6·H of the cut, at most 2 % of
    the points — and the enumeration alone must stay under that cap.  The cloud of the chosen seed against the fixture at rest."""
    from conftest import load_dam_break_2d
    p, s = load_dam_break_2d()
    F = np.asarray(p.Position, np.float64)[np.asarray(p.Type) == 1]
    cfg = _cfg(0, 2, h=s.SimKernel.h, k=s.SimKernel.k, dp=s.SimConstants.dx)
    pts = gradient_cloud(F, cfg.H, cfg.dx)
    assert pts.shape == (700, 2)
    r = brute_force_point_gradients(cfg, pts, p.Position, p.Velocity, p.Density, p.Pressure, p.Type)
    print(f"700 points, {int(r['near'].sum())} with a row within 1e-6 H of the cut, {int((r['n'] > 0).sum())} see fluid")
    assert r["near"].sum() <= 0.02 * len(pts) and (r["n"] > 0).sum() > 100


# ---- fields.py on hand-made sums --------------------------------------------------------------------------------------------------
def _hand_made(n=4):
    S = np.array([1.0, 0.8, 0.05, 0.0])[:n]
    sums = {"weight": S, "grad_weight": np.zeros((n, 3)), "sum_velocity": np.zeros((n, 3)), "grad_velocity": np.zeros((n, 3, 3)),
            "sum_pressure": np.zeros(n), "grad_pressure": np.zeros((n, 3))}
    return sums


def test_vorticity_from_an_antisymmetric_gradient_and_nan_below_min_weight():
    from sphexample_amd.fields import (MIN_GRADIENT_WEIGHT, divergence_at, pressure_gradient, strain_rate, surface_normal_at, velocity_gradient,
                                       vorticity_at)
    sums = _hand_made()
    Om = np.array([0.3, -1.1, 2.0])
    # v = Ω × x: ∂v_a/∂x_b = −ε_abc Ω_c, antisymmetric; Gv = S · L with G = 0
    L = np.array([[0.0, -Om[2], Om[1]], [Om[2], 0.0, -Om[0]], [-Om[1], Om[0], 0.0]])
    sums["grad_velocity"][:] = sums["weight"][:, None, None] * L
    w = vorticity_at(sums)
    assert w.shape == (4, 3)
    np.testing.assert_allclose(w[:2], np.tile(2 * Om, (2, 1)), rtol=1e-15)          # a rigid rotation: ω = 2Ω
    assert np.isnan(w[2:]).all()                                                   # S = 0.05 and 0 lie below min_weight
    assert 0.05 < MIN_GRADIENT_WEIGHT <= 0.5
    np.testing.assert_allclose(vorticity_at(sums, min_weight=0.01)[2], 2 * Om, rtol=1e-15)
    assert np.isnan(vorticity_at(sums, min_weight=0.01)[3]).all() and np.isnan(vorticity_at(sums, min_weight=0.9)[1]).all()
    assert np.abs(divergence_at(sums)[:2]).max() == 0 and np.abs(strain_rate(sums)[:2]).max() == 0
    assert np.isnan(divergence_at(sums)[2]) and np.isnan(strain_rate(sums)[3]).all() and np.isnan(velocity_gradient(sums)[2]).all()
    # the correction: a constant field has no gradient whatever G is — GA = A · G, SA = A · S
    sums["grad_weight"][:] = [[0.4, -2.0, 0.7]]
    c = np.array([5.0, -3.0, 0.25])
    sums["sum_velocity"][:] = sums["weight"][:, None] * c
    sums["grad_velocity"][:] = c[None, :, None] * sums["grad_weight"][:, None, :]
    sums["sum_pressure"][:] = 9.0 * sums["weight"]
    sums["grad_pressure"][:] = 9.0 * sums["grad_weight"]
    assert np.abs(velocity_gradient(sums)[:2]).max() <= 1e-14 and np.abs(pressure_gradient(sums)[:2]).max() <= 1e-14
    # … and a linear one keeps its own: add S · L on top
    sums["grad_velocity"] += sums["weight"][:, None, None] * L
    np.testing.assert_allclose(velocity_gradient(sums)[:2], np.tile(L, (2, 1, 1)), rtol=0, atol=1e-14)
    sums["grad_pressure"] += sums["weight"][:, None] * np.array([1.0, 2.0, -4.0])
    np.testing.assert_allclose(pressure_gradient(sums)[:2], [[1.0, 2.0, -4.0]] * 2, rtol=0, atol=1e-14)
    assert np.isnan(pressure_gradient(sums)[2:]).all()
    # the outward normal: −G / |G|
    nrm = surface_normal_at(sums)
    np.testing.assert_allclose(nrm[:2], np.tile(-np.array([0.4, -2.0, 0.7]) / np.sqrt(0.16 + 4.0 + 0.49), (2, 1)), rtol=1e-15)
    assert np.isnan(nrm[2:]).all()
    sums["grad_weight"][0] = 0.0
    assert np.isnan(surface_normal_at(sums)[0]).all()                              # no direction where G vanishes
    with pytest.raises(ValueError):
        velocity_gradient({**sums, "grad_velocity": np.zeros((4, 3))})
    with pytest.raises(KeyError):
        pressure_gradient({"weight": sums["weight"], "grad_weight": sums["grad_weight"]})


# ---- the symbol -------------------------------------------------------------------------------------------------------------------
def test_header_library_and_bindings_agree():
    text = open(os.path.join(ROOT, "include", "sphmi.h")).read()
    assert re.search(r"#define\s+SPHMI_ABI_VERSION\s+5\b", text) and _abi.ABI_VERSION == 5      # append-only: the version stays
    proto = _prototype("sphmi_sample_point_gradients")
    assert proto == ["sphmi_handle*", "int64_t", "const double*", "double*", "int64_t*"] + ["double*"] * 7
    assert _prototype("sphmi_sample_points")[:5] == proto[:5]                      # the calling convention of sphmi_sample_points
    from sphexample_amd.engine import load_library
    assert hasattr(load_library(), "sphmi_sample_point_gradients")
    b = _backend(3)
    out = b.sample_point_gradients(np.arange(15.0).reshape(5, 3))
    fn = b._lib.fns["sphmi_sample_point_gradients"]
    assert fn.argtypes == [C.c_void_p, C.c_int64] + [C.c_void_p] * 10 and len(fn.argtypes) == len(proto)
    assert len(fn.calls) == 1 and len(fn.calls[0]) == len(proto) and fn.calls[0][1] == 5
    assert list(out) == list(KEYS) == list(_abi.Backend.GRADIENT_FIELDS)
    assert out["weight"].shape == out["count"].shape == out["sum_pressure"].shape == out["sum_density"].shape == (5,)
    assert out["sum_velocity"].shape == out["grad_weight"].shape == out["grad_pressure"].shape == out["grad_density"].shape == (5, 3)
    assert out["grad_velocity"].shape == (5, 3, 3) and out["count"].dtype == np.int64 and out["grad_velocity"].dtype == np.float64
    assert all(a.flags.c_contiguous for a in out.values())
    b2 = _backend(2)
    out = b2.sample_point_gradients(np.zeros((0, 2)), fields=("grad_velocity", "weight"))      # an empty cloud travels as n = 0
    assert set(out) == {"grad_velocity", "weight"} and out["grad_velocity"].shape == (0, 3, 3)
    call = b2._lib.fns["sphmi_sample_point_gradients"].calls[0]
    assert call[1] == 0 and [a is None for a in call[3:]] == [False, True, True, True, True, True, True, True, False]
    for bad in (lambda: b2.sample_point_gradients(np.zeros((4, 3))), lambda: b2.sample_point_gradients(np.zeros(4)),
                lambda: b2.sample_point_gradients(np.zeros((4, 2)), fields=("vorticity",))):
        with pytest.raises(ValueError):
            bad()


def test_the_julia_shim_binds_the_symbol():
    from test_julia_shim import c_prototypes, shim_ccalls
    calls = [c for c in shim_ccalls() if c[0] == "sphmi_sample_point_gradients"]
    assert len(calls) == 1 and len(calls[0][2]) == len(c_prototypes()["sphmi_sample_point_gradients"][1]) == 12
    shim = open(os.path.join(ROOT, "julia", "SPHExampleMI355X.jl"), encoding="utf-8").read()
    assert shim.index("function sample_points(") < shim.index("function sample_point_gradients(") < shim.index("function particle_fields(")


# ---- RunSimulation ----------------------------------------------------------------------------------------------------------------
class _GradientStandIn(_StandIn):
    def sample_points(self, positions):
        self.log.append(("sample_points", self.iteration))
        return {"weight": np.zeros(len(positions))}

    def sample_point_gradients(self, positions):
        self.log.append(("sample_point_gradients", self.iteration))
        n = len(positions)
        return {"weight": np.full(n, float(self.iteration)), "grad_velocity": np.zeros((n, 3, 3)), "positions": np.array(positions)}


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
                                         backend_factory=_GradientStandIn, on_output=lambda m, pp, *extra: got.append((m.Iteration, extra)), **kw)
        return steps, got, _StandIn.instances[0]

    steps, got, eng = run(sample_point_gradients=cloud)
    assert len(got) == len(steps) + 1 >= 3 and got[0] == (0, (None,))              # the call before the first step: nothing to sample yet
    for iteration, extra in got[1:]:
        assert len(extra) == 1 and extra[0]["grad_velocity"].shape == (3, 3, 3)
        assert (extra[0]["weight"] == iteration).all() and extra[0]["positions"].tolist() == cloud      # on the state of THIS output
    seq = [e for e in eng.log if isinstance(e, tuple)]
    assert [e[0] for e in seq] == ["advance", "sample_point_gradients", "download"] * len(steps)
    # behind sample_points when both are on; the default leaves the callback's arguments as they were
    _, got2, eng2 = run(sample_points=cloud, sample_point_gradients=cloud)
    assert all(len(extra) == 2 for _, extra in got2) and set(got2[1][1][0]) == {"weight"} and "grad_velocity" in got2[1][1][1]
    assert [e[0] for e in eng2.log if isinstance(e, tuple)][:4] == ["advance", "sample_points", "sample_point_gradients", "download"]
    _, got3, eng3 = run()
    assert all(extra == () for _, extra in got3) and not any(e[0] == "sample_point_gradients" for e in eng3.log if isinstance(e, tuple))


# ---- the code object --------------------------------------------------------------------------------------------------------------
def test_the_kernel_is_built_for_gfx950_within_the_budget_of_its_siblings(tmp_path):
    """The code object's metadata — read the way tests/test_bench_contract.py reads it — shows the four instantiations of
    k_point_gradients without scratch, with exactly the LDS of k_point_cloud and at most 128 registers: four workgroups of four
    waves per compute unit, as the sibling kernels.  The bin passes are k_point_cloud's: there is one copy of each."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_report
    from sphexample_amd import build
    lib = build.build()
    assert hasattr(C.CDLL(lib), "sphmi_sample_point_gradients")
    co = isa_report.code_object(lib, str(tmp_path))
    meta = isa_report.metadata(co)
    names = isa_report.demangle(list(meta))
    mine = {names[k]: v for k, v in meta.items() if "sphmi::k_point_gradients<" in names[k]}
    assert len(mine) == 4 and all(any(f"k_point_gradients<{t}, {d}>" in n for n in mine) for t in ("float", "double") for d in (2, 3)), sorted(mine)
    cloud = {names[k]: v for k, v in meta.items() if "sphmi::k_point_cloud<" in names[k]}
    assert len(cloud) == 4
    for d, v in sorted(mine.items()):
        print(f"{d}: {v['vgprs']} VGPRs, {v['agprs']} AGPRs, {v['sgprs']} SGPRs, {v['lds_bytes']} B LDS, {v['scratch_bytes']} B scratch")
        assert v["scratch_bytes"] == 0, (d, v)
        assert v["lds_bytes"] == 38928 and {w["lds_bytes"] for w in cloud.values()} == {38928}, (d, v)
        assert 4 * v["lds_bytes"] <= 160 * 1024, (d, v)
        assert v["vgprs"] + v["agprs"] <= 128, (d, v)                              # four waves per SIMD
        assert v["max_flat_workgroup_size"] == 256, (d, v)
    bins = [names[k] for k in meta if re.search(r"\bk_pc_(count|tiles|scatter|describe)\b", names[k])]
    assert len(bins) == 4, sorted(bins)
    outlined = [d for k, d in isa_report.demangle(list(isa_report.kernels(co))).items() if k not in meta]
    assert not outlined, outlined[:4]
