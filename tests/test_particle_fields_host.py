"""Host side of the per-particle differential fields (sphmi_particle_fields, csrc/sphmi_particle_fields.h): the prototype and
its binding, the reference enumeration `brute_force_particle_fields` pinned against analysis, `free_surface_mask`, the
RunSimulation plumbing with a stand-in backend, and what the built code object says about the kernel.  No GPU.

    for every row i over every row j != i with r^2 = |x_i - x_j|^2 <= H^2, V_j = m0 / rho_j, grad_i W_ij = W'(r) (x_i - x_j) / r:
    n = rows    S = V_i W(0) + sum V_j W_ij    N = sum V_j grad_i W_ij    div r = sum V_j (x_j - x_i) . grad_i W_ij
    div v = sum V_j (v_j - v_i) . grad_i W_ij    w = sum V_j grad_i W_ij x (v_j - v_i)
"""
import copy
import ctypes as C
import os
import re
import sys
import types

import numpy as np
import pytest

from sphexample_amd import _abi
from test_field_grid_host import _backend, _header, _prototype, _StandIn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference ------------------------------------------------------------------------------------------------------
def kernel_w_dw(cfg, r):
    """W(r) and W'(r) of src/SPHKernels.jl:75-105 (Wendland C2, CubicSpline), q = r / h; cfg.kernel: 0 / 1 as in include/sphmi.h."""
    q = np.asarray(r, dtype=np.float64) * cfg.h_inv
    if cfg.kernel == 1:
        inner, outer = (0 <= q) & (q <= 1), (1 < q) & (q <= 2)
        W = cfg.alphaD * ((1 - 1.5 * q ** 2 + 0.75 * q ** 3) * inner + 0.25 * (2 - q) ** 3 * outer)
        dWdq = cfg.alphaD * ((-3 * q + 2.25 * q ** 2) * inner - 0.75 * (2 - q) ** 2 * outer)
    else:
        W = cfg.alphaD * (1 - q / 2) ** 4 * (2 * q + 1)
        dWdq = -5.0 * cfg.alphaD * q * (1 - q / 2) ** 3
    return W, dWdq * cfg.h_inv


def brute_force_particle_fields(cfg, pos, vel, rho, targets=None, chunk=128):
    """Every target row against every row, in fp64, from the definition in the module docstring.  `targets`: row indices (default:
    all rows).  Returns n [M] (int64), S, div_r, div_v [M], N, w [M, 3] and near [M]: a row j != i lies within 1e-6·H of the cut.
    A pair with r = 0 counts in n and S and is left out of the four gradient sums."""
    X, U, rho = np.asarray(pos, np.float64), np.asarray(vel, np.float64), np.asarray(rho, np.float64)
    N, D = X.shape
    idx = np.arange(N) if targets is None else np.asarray(targets, dtype=np.int64)
    M = len(idx)
    V = cfg.m0 / rho
    W0 = float(kernel_w_dw(cfg, 0.0)[0])
    out = {"n": np.zeros(M, np.int64), "S": np.zeros(M), "N": np.zeros((M, 3)), "div_r": np.zeros(M), "div_v": np.zeros(M),
           "w": np.zeros((M, 3)), "near": np.zeros(M, bool)}
    for a0 in range(0, M, chunk):
        rows = idx[a0:a0 + chunk]
        m = len(rows)
        d = [X[rows, c][:, None] - X[None, :, c] for c in range(D)]                 # x_i - x_j per axis, [m, N]
        r2 = d[0] * d[0] + d[1] * d[1]
        if D == 3:
            r2 = r2 + d[2] * d[2]
        notself = np.ones((m, N), bool)
        notself[np.arange(m), rows] = False
        dist = np.sqrt(r2)
        out["near"][a0:a0 + m] = ((np.abs(dist - cfg.H) <= 1e-6 * cfg.H) & notself).any(1)
        sel = (r2 <= cfg.H2) & notself
        a, j = np.nonzero(sel)                                                      # target (within the chunk), neighbour
        r = dist[a, j]
        W, dW = kernel_w_dw(cfg, r)
        add = lambda w: np.bincount(a, weights=w, minlength=m)                      # noqa: E731
        out["n"][a0:a0 + m] = np.bincount(a, minlength=m)
        out["S"][a0:a0 + m] = V[rows] * W0 + add(V[j] * W)
        g = r > 0
        a, j, r, dW = a[g], j[g], r[g], dW[g]
        e = np.zeros((len(a), 3)); u = np.zeros((len(a), 3))
        for c in range(D):
            e[:, c] = d[c][sel][g]
            u[:, c] = U[j, c] - U[rows[a], c]
        grad = (V[j] * dW / r)[:, None] * e                                         # V_j grad_i W_ij
        cross = np.cross(grad, u)
        for c in range(3):
            out["N"][a0:a0 + m, c] = add(grad[:, c])
            out["w"][a0:a0 + m, c] = add(cross[:, c])
        out["div_r"][a0:a0 + m] = add(-(e * grad).sum(1))
        out["div_v"][a0:a0 + m] = add((u * grad).sum(1))
    return out


def lattice_case(D, n, dp=0.02, kernel=0):
    """An n^D lattice at spacing dp with uniform density, h = 1.2·sqrt(D)·dp, H = 2h, and v = Omega x x + diag(a) x."""
    h = 1.2 * np.sqrt(D) * dp
    alphaD = {0: {2: 7 / (4 * np.pi * h ** 2), 3: 21 / (16 * np.pi * h ** 3)}, 1: {2: 10 / (7 * np.pi * h ** 2), 3: 1 / (np.pi * h ** 3)}}[kernel][D]
    rho0 = 1000.0
    cfg = types.SimpleNamespace(kernel=kernel, alphaD=alphaD, h=h, h_inv=1 / h, H=2 * h, H2=(2 * h) ** 2, m0=rho0 * dp ** D, dims=D)
    ax = np.arange(n) * dp
    X = np.stack(np.meshgrid(*[ax] * D, indexing="ij"), -1).reshape(-1, D)
    Om = np.array([0.3, -0.2, 0.7]) if D == 3 else np.array([0.0, 0.0, 0.7])
    a = np.array([0.5, 0.2, -0.1])
    X3 = np.concatenate([X, np.zeros((len(X), 3 - D))], axis=1)
    U = (np.cross(Om[None, :], X3) + a[None, :] * X3)[:, :D]
    centre = int(np.ravel_multi_index((n // 2,) * D, (n,) * D))
    return cfg, X, U, np.full(len(X), rho0), centre, Om, a[:D].sum()


# ---- 1., 2. the prototype and the binding ---------------------------------------------------------------------------------
def test_header_and_binding_agree():
    assert re.search(r"#define\s+SPHMI_ABI_VERSION\s+5\b", _header()) and _abi.ABI_VERSION == 5      # append-only: the version stays
    assert _prototype("sphmi_particle_fields") == ["sphmi_handle*", "int64_t*", "double*", "double*", "double*", "double*", "double*"]
    names = re.findall(r"(\w+_out)\s*[,)]", re.sub(r"/\*.*?\*/", "", re.search(r"int\s+sphmi_particle_fields\s*\((.*?)\)\s*;", _header(), re.S).group(0), flags=re.S))
    assert names == ["count_out", "shepard_out", "normal_out", "div_r_out", "div_v_out", "vorticity_out"]
    b = _backend(3)
    out = b.particle_fields()
    fn = b._lib.fns["sphmi_particle_fields"]
    assert fn.argtypes == [C.c_void_p] * 7 and len(fn.calls) == 1 and len(fn.calls[0]) == 7
    assert tuple(out) == _abi.Backend.PARTICLE_FIELDS == ("count", "shepard", "normal", "div_r", "div_v", "vorticity")
    assert out["count"].shape == out["shepard"].shape == out["div_r"].shape == out["div_v"].shape == (10,)
    assert out["normal"].shape == out["vorticity"].shape == (10, 3)
    assert out["count"].dtype == np.int64 and all(out[k].dtype == np.float64 for k in out if k != "count")
    assert all(a.flags.c_contiguous for a in out.values())
    # a subset of the fields: the others travel as NULL
    b2 = _backend(2)
    out = b2.particle_fields(fields=("vorticity", "div_r"))
    assert set(out) == {"vorticity", "div_r"} and out["vorticity"].shape == (10, 3) and out["div_r"].shape == (10,)
    assert [a is None for a in b2._lib.fns["sphmi_particle_fields"].calls[0][1:]] == [True, True, True, False, True, False]
    assert b2.particle_fields(fields=()) == {} and all(a is None for a in b2._lib.fns["sphmi_particle_fields"].calls[1][1:])
    for bad in (("pressure",), ("count", "curl")):
        with pytest.raises(ValueError):
            b2.particle_fields(fields=bad)
    assert len(b2._lib.fns["sphmi_particle_fields"].calls) == 2                     # refused before the library is asked


# ---- 3. the library ----------------------------------------------------------------------------------------------------------
def test_the_kernel_is_built_for_gfx950_without_scratch(tmp_path):
    """The library exports the entry point; the code object's metadata — read the way tests/test_bench_contract.py reads it — shows
    the four instantiations of k_particle_fields without scratch, with LDS for four workgroups per compute unit (160 KiB) and
    registers for four waves per SIMD (512 / 4)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_report
    from sphexample_amd import build
    lib = build.build()
    assert hasattr(C.CDLL(lib), "sphmi_particle_fields")
    co = isa_report.code_object(lib, str(tmp_path))
    meta = isa_report.metadata(co)
    names = isa_report.demangle(list(meta))
    mine = {names[k]: v for k, v in meta.items() if "k_particle_fields" in names[k]}
    assert len(mine) == 4, sorted(mine)
    assert {("<float, 2>" in d, "<double, 3>" in d) for d in mine} >= {(True, False), (False, True)}
    for d, v in mine.items():
        assert v["scratch_bytes"] == 0, (d, v)
        assert 4 * v["lds_bytes"] <= 160 * 1024, (d, v)
        assert v["vgprs"] + v["agprs"] <= 128, (d, v)
        assert v["max_flat_workgroup_size"] == 256, (d, v)


# ---- 4. the enumeration against analysis ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,n,neighbours", [(2, 21, 36), (3, 13, 304)])
def test_the_enumeration_reproduces_a_linear_velocity_field(D, n, neighbours):
    """v = Omega x x + diag(a) x on a lattice: at the centre row w = 2 Omega, div v = tr(a) and div r = D within 2 % (the
    discretisation error of the kernel sums at h = 1.2·sqrt(D)·dp; a wrong sign or a transposed cross product misses by 200 %)."""
    cfg, X, U, rho, c, Om, tr = lattice_case(D, n)
    ref = brute_force_particle_fields(cfg, X, U, rho, targets=[c])
    w, divv, divr, S = ref["w"][0], ref["div_v"][0], ref["div_r"][0], ref["S"][0]
    print(f"{D}-D: n {ref['n'][0]}, S {S:.6f}, div r {divr:.6f}, div v {divv:.6f} (tr a {tr}), w {w} (2 Omega {2 * Om}), N {ref['N'][0]}")
    assert ref["n"][0] == neighbours
    assert abs(S - 1.0) <= 0.01
    assert abs(divr - D) <= 0.02 * D and abs(divv - tr) <= 0.02 * abs(tr)
    assert np.abs(w - 2 * Om).max() <= 0.02 * np.abs(2 * Om).max()
    if D == 2:
        assert (ref["w"][:, :2] == 0).all() and (ref["N"][:, 2] == 0).all()
    assert np.abs(ref["N"][0]).max() <= 1e-9 / cfg.h                                # a symmetric neighbourhood: the normal cancels
    # a subset of targets is the same rows of the full enumeration
    some = [0, c, len(X) - 1]
    full, part = brute_force_particle_fields(cfg, X, U, rho), brute_force_particle_fields(cfg, X, U, rho, targets=some)
    for k in full:
        np.testing.assert_array_equal(part[k], full[k][some], err_msg=k)
    # a duplicate of the centre row: one more row in n, V·W(0) more in S, nothing in the gradient sums
    dup = brute_force_particle_fields(cfg, np.concatenate([X, X[c:c + 1]]), np.concatenate([U, U[c:c + 1]]), np.append(rho, rho[c]), targets=[c])
    assert dup["n"][0] == neighbours + 1
    assert dup["S"][0] == pytest.approx(S + (cfg.m0 / rho[c]) * cfg.alphaD, rel=1e-14) and dup["S"][0] > S
    for k in ("N", "div_r", "div_v", "w"):
        np.testing.assert_array_equal(dup[k], ref[k], err_msg=k)
    # the cubic spline: the same signs (no bar on its discretisation error is claimed here; a wrong sign gives -1 times the value)
    cfg1 = lattice_case(D, n, kernel=1)[0]
    ref1 = brute_force_particle_fields(cfg1, X, U, rho, targets=[c])
    print(f"{D}-D cubic spline: S {ref1['S'][0]:.6f}, div r {ref1['div_r'][0]:.6f}, w {ref1['w'][0]}")
    assert 0.5 * D <= ref1["div_r"][0] <= 1.5 * D and 0.5 <= ref1["w"][0, 2] / (2 * Om[2]) <= 1.5


# ---- 5. the free-surface mask ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,n", [(2, 21), (3, 13)])
def test_free_surface_mask_flags_the_edge_of_the_lattice(D, n):
    from sphexample_amd.fields import FREE_SURFACE_DIV_R, free_surface_mask
    cfg, X, U, rho, c, _, _ = lattice_case(D, n)
    ref = brute_force_particle_fields(cfg, X, U, rho)
    mask = free_surface_mask(ref["div_r"], D)
    idx = np.stack(np.unravel_index(np.arange(len(X)), (n,) * D), -1)
    edge = ((idx == 0) | (idx == n - 1)).any(1)
    assert mask.dtype == bool and mask.shape == (len(X),)
    assert mask[edge].all() and not mask[c]
    assert FREE_SURFACE_DIV_R == {2: 1.5, 3: 2.4}
    np.testing.assert_array_equal(mask, ref["div_r"] < FREE_SURFACE_DIV_R[D])
    assert free_surface_mask(ref["div_r"], D, threshold=-1.0).sum() == 0 and free_surface_mask(ref["div_r"], D, threshold=10.0).all()
    # N is the gradient of the colour function: at an edge it points into the particle set, -N out of it
    face = int(np.ravel_multi_index((0,) + (n // 2,) * (D - 1), (n,) * D))          # the middle of the face x = 0
    assert ref["N"][face, 0] > 0 and np.abs(ref["N"][face, 1:]).max() <= 1e-9 * abs(ref["N"][face, 0])
    with pytest.raises(ValueError):
        free_surface_mask(ref["div_r"], 4)


# ---- 6. RunSimulation ----------------------------------------------------------------------------------------------------------------
class _FieldsStandIn(_StandIn):
    def particle_fields(self, fields):
        self.log.append(("particle_fields", self.iteration))
        n = 5
        out = {"count": np.zeros(n, np.int64), "shepard": np.full(n, float(self.iteration)), "normal": np.zeros((n, 3)), "div_r": np.zeros(n),
               "div_v": np.zeros(n), "vorticity": np.zeros((n, 3))}
        return {k: out[k] for k in fields}


def test_run_simulation_hands_the_fields_to_the_callback():
    from conftest import load_dam_break_2d
    from sphexample_amd import simulation
    p, s = load_dam_break_2d()

    def run(**kw):
        meta = copy.deepcopy(s.SimMetaData)
        meta.SimulationTime, meta.OutputTimes = 0.002, 0.001
        got = []
        _StandIn.instances.clear()
        steps = simulation.RunSimulation(SimGeometry=None, SimMetaData=meta, SimConstants=s.SimConstants, SimKernel=s.SimKernel, SimLogger=None,
                                         SimParticles=p.copy(), SimViscosity=s.SimViscosity, SimDensityDiffusion=s.SimDensityDiffusion,
                                         backend_factory=_FieldsStandIn, on_output=lambda m, pp, *extra: got.append((m.Iteration, extra)), **kw)
        return steps, got, _StandIn.instances[0]

    steps, got, eng = run(particle_fields=("shepard", "vorticity"))
    assert len(got) == len(steps) + 1 >= 3
    assert got[0] == (0, (None,))                                                  # the call before the first step: nothing to evaluate yet
    for iteration, extra in got[1:]:
        assert len(extra) == 1 and set(extra[0]) == {"shepard", "vorticity"}
        assert (extra[0]["shepard"] == iteration).all()                             # evaluated on the state of THIS output
    seq = [e for e in eng.log if isinstance(e, tuple)]
    assert [e[0] for e in seq] == ["advance", "particle_fields", "download"] * len(steps)
    # behind group forces and the field grid when those are on
    lattice = ([0.05, 0.01], [0.1, 0.05], [12, 9])
    _, got2, eng2 = run(group_forces=[1, 2], field_grid=lattice, particle_fields=("div_r",))
    assert all(len(extra) == 3 for _, extra in got2) and got2[0][1][1:] == (None, None)
    assert got2[1][1][0][3].shape == (3, 2, 3) and got2[1][1][1]["weight"].shape == (9, 12) and set(got2[1][1][2]) == {"div_r"}
    assert [e[0] for e in eng2.log if isinstance(e, tuple)][:4] == ["advance", "sample_grid", "particle_fields", "download"]
    # without the keyword the callback keeps its arguments and nothing is evaluated
    _, got3, eng3 = run()
    assert all(extra == () for _, extra in got3) and not any(e[0] == "particle_fields" for e in eng3.log if isinstance(e, tuple))
