"""Host side of the ray search (sphmi_cast_rays, csrc/sphmi_rays.h): the plain C++ part of the header compiled for the host with the
address and undefined-behaviour sanitizers (tests/host_rays/rays_main.cpp, a program of its own) against `sphexample_amd.rays` to the
bit; `rays.restate` on an analytic half-space and on an O(M·N) enumeration of the 2-D dam-break fixture against a dense scan; the cap
on rays at the level for the seed the GPU test uses; the prototype, its export and its bindings; the RunSimulation plumbing with a
stand-in backend; and what the built code object says about the kernel.  No GPU."""
import copy
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from sphexample_amd import _abi, rays
from test_field_grid_host import _StandIn, _backend, _prototype
from test_point_gradients_host import kernel_w_dw
from test_step_series_host import CSRC, SANITIZE, host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "host_rays", "rays_main.cpp")
KS = (1, 63, 64, 65, 129)
BRUTE_K, BRUTE_SEED = 5, 41
MODE_NAMES = {0: "enter", 1: "leave", 2: "any"}


# ---- shared with tests/test_rays_gpu.py -----------------------------------------------------------------------------------------
def gauge_rays(lo, hi, H, n, K, seed):
    """n rays from 3 H above the fluid box (lo, hi) downwards along the last axis, a third of them oblique and none a unit vector,
    spread over the box widened by H, with exactly K march intervals: (origins, directions, t_end [n], step)."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    D = len(lo)
    rng = np.random.default_rng(seed)
    o = rng.uniform(lo - H, hi + H, (n, D))
    o[:, D - 1] = hi[D - 1] + 3.0 * H
    d = np.zeros((n, D))
    d[:, D - 1] = -rng.uniform(1.0, 1.3, n)
    d[::3, :D - 1] = rng.uniform(-0.3, 0.3, (len(d[::3]), D - 1))
    span = (hi[D - 1] - lo[D - 1]) + 5.0 * H
    step = span / (K - 0.5)
    te = np.full(n, span)
    assert (rays.intervals(0.0, te, step) == K).all()
    return o, d, te, step


def brute_force_weight(cfg, points, pos, rho, typ, chunk=256):
    """S = Σ (m0 / ρ_j) W(|x − x_j|) over the Fluid rows with r² = ((dx² + dy²) + dz²) <= H², every point against every row, in
    fp64; never calls the library.  tests/bruteforce.py enumerates PAIRS OF ROWS for the forces and holds no sum at a free point, so
    the enumeration stands here, in its style and with the kernel of tests/test_point_gradients_host.py (as that file's
    `brute_force_point_gradients` does for the gradients); like bruteforce.py it shares no code with the library."""
    points, pos = np.asarray(points, np.float64), np.asarray(pos, np.float64)
    fluid = np.asarray(typ) == 1
    x, V = pos[fluid], cfg.m0 / np.asarray(rho, np.float64)[fluid]
    S = np.zeros(len(points))
    for a in range(0, len(points), chunk):
        e = points[a:a + chunk, None, :] - x[None, :, :]
        r2 = e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]
        if points.shape[1] == 3:
            r2 = r2 + e[..., 2] * e[..., 2]
        W = kernel_w_dw(cfg, np.sqrt(r2))[0]
        S[a:a + chunk] = np.where(r2 <= cfg.H2, V[None, :] * W, 0.0).sum(axis=1)
    return S


def _fixture_cfg():
    from conftest import load_dam_break_2d
    from sphexample_amd._abi import make_config
    p, s = load_dam_break_2d()
    cfg = make_config(len(p), s.SimConstants, s.SimKernel, s.SimMetaData, s.SimViscosity, s.SimDensityDiffusion, device_float_bytes=8,
                      host_float_bytes=8, device=0)
    return p, s, cfg


# ---- the plain C++ part against rays.py -------------------------------------------------------------------------------------------
def _hex(words):
    return np.array([float.fromhex(w) for w in words])


def test_the_host_program_and_the_restatement_agree_to_the_bit(tmp_path):
    main = [ln.split()[1] for ln in open(MAIN).read().splitlines() if ln.startswith("#include")]
    assert [i for i in main if i.startswith('"')] == ['"sphmi_rays.h"']
    cxx = host_compiler()
    exe = str(tmp_path / "rays_main")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I", CSRC, MAIN, "-o", exe]
    for extra in (SANITIZE + ("-static-libasan", "-static-libubsan"), SANITIZE, ()):
        built = subprocess.run(base + list(extra), capture_output=True, text=True)
        if built.returncode == 0:
            break
    assert built.returncode == 0, built.stderr
    print("sanitizers:", " ".join(extra) or "none")
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip().splitlines()[-1] == "ok" and not run.stderr.strip(), run.stdout[-2000:] + run.stderr
    lines = run.stdout.strip().splitlines()
    cases, cur = [], None
    for ln in lines:
        w = ln.split()
        if w[0] == "case":
            cur = {"name": w[1], "mode": MODE_NAMES[int(w[2])], "K": int(w[3]), "rounds": []}
            cases.append(cur)
        elif w[0] == "args":
            cur["args"] = _hex(w[1:])
        elif w[0] == "march":
            cur["march"] = _hex(w[1:])
        elif w[0] == "found":
            cur["status"], cur["interval"] = int(w[1]), int(w[2])
        elif w[0] == "round":
            cur["rounds"].append((int(w[1]), float.fromhex(w[2]), int(w[3]), _hex(w[4:])))
        elif w[0] == "result":
            cur["result"] = _hex(w[1:])
    names = [c["name"] for c in cases]
    assert len(cases) == 16 and {c["K"] for c in cases} >= set(KS)
    seen_K = {}
    for c in cases:
        ox, oy, dx, dy, tb, te, step, z0 = c["args"]
        K = int(rays.intervals(tb, te, step))
        assert K == c["K"], c["name"]
        t = rays.march_t(tb, te, step, np.arange(K + 1), K)
        assert t.tobytes() == c["march"].tobytes() and t[-1] == te, c["name"]
        half_plane = lambda x: {"weight": (x[:, 1] <= z0).astype(np.float64)}      # noqa: E731
        r = rays.restate(half_plane, [[ox, oy]], [[dx, dy]], tb, te, step, 0.5, c["mode"])
        assert (int(r["status"][0]), int(r["interval"][0])) == (c["status"], c["interval"]), c["name"]
        got = np.concatenate([r["bracket"][0], r["point"][0]])
        assert got.tobytes() == c["result"].tobytes() or (np.isnan(got[:4]).all() and np.isnan(c["result"][:4]).all() and got[4] == c["result"][4] == 0), c["name"]
        # the refinement points of every executed round, from the brackets the choices leave
        if c["interval"] >= 1:
            a, b = t[c["interval"] - 1], t[c["interval"]]
            for _, delta, m, u in c["rounds"]:
                assert (b - a) * 0.015625 == delta != 0
                assert rays.refine_u(a, b, delta, np.arange(1, 64)).tobytes() == u.tobytes(), c["name"]
                a, b = float(rays.refine_u(a, b, delta, m - 1)), float(rays.refine_u(a, b, delta, m))
            assert (a, b) == tuple(c["result"][:2])
        seen_K[c["name"]] = (K, c["interval"], len(c["rounds"]))
    print(seen_K)
    assert seen_K["K63_last"][:2] == (63, 63) and seen_K["K64_last"][:2] == (64, 64) and seen_K["K65_last"][:2] == (65, 65)
    assert seen_K["K129_first"][:2] == (129, 1) and seen_K["K1"][:2] == (1, 1) and seen_K["ragged_end"][1] == seen_K["ragged_end"][0]
    assert seen_K["delta_zero"][1] >= 1 and seen_K["delta_zero"][2] == 0 and seen_K["K64_last"][2] == 4
    assert seen_K["no_crossing"][1] == seen_K["degenerate"][1] == seen_K["leave_as_enter"][1] == -1 and "oblique" in names


# ---- restate on an analytic half-space ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [2, 3])
def test_restate_finds_a_half_space_in_every_mode(dims):
    """S = 1 for z <= z0 and 0 above (z the last axis): the crossing of every ray lies at z0, within step / 2²⁴ along the ray."""
    z0, step = 0.4321, 0.0173
    rng = np.random.default_rng(dims)
    half_space = lambda x: {"weight": (x[:, dims - 1] <= z0).astype(np.float64)}      # noqa: E731
    n = 40
    for mode, start, sign in (("enter", 1.0, -1.0), ("leave", 0.1, 1.0), ("any", 1.0, -1.0), ("any", 0.1, 1.0)):
        o = rng.uniform(-1.0, 1.0, (n, dims)); o[:, dims - 1] = start
        d = np.zeros((n, dims)); d[:, dims - 1] = sign                              # axis-parallel …
        d[n // 2:, :dims - 1] = rng.uniform(-0.7, 0.7, (n - n // 2, dims - 1))     # … and oblique
        d[n // 2:] *= rng.uniform(0.5, 2.0, (n - n // 2, 1))                        # not unit vectors: t is in units of |d|
        te = 0.95 / np.abs(d[:, dims - 1])
        r = rays.restate(half_space, o, d, 0.0, te, step, 0.5, mode)
        assert (r["status"] & 1).all() and ((r["status"] & 2 != 0) == (start < z0)).all()
        t_exact = (z0 - start) / d[:, dims - 1]
        a, b = r["bracket"][:, 0], r["bracket"][:, 1]
        # (every u_m = a + m·δ is rounded once: four rounds leave the width within 8 spacings of t of step / 2²⁴ — the slack
        # profiles/rays.md states; that the exact crossing lies in [a, b] is asserted on its own, next)
        assert (b - a <= step / 2 ** 24 + 8 * np.spacing(te)).all() and (b > a).all()
        assert (a <= t_exact + 1e-15).all() and (t_exact <= b + 1e-15).all(), mode
        assert (r["point"][:, dims - 1] <= z0).all() and (np.abs(r["point"][:, dims - 1] - z0) <= 2 * step / 2 ** 24 * np.abs(d[:, dims - 1]) + 1e-15).all()
        assert (r["weight"] == 1).all()                                             # the record is the inside end's
        K = rays.intervals(0.0, te, step)                                           # (the march interval that holds z0)
        k = r["interval"]
        assert ((1 <= k) & (k <= K)).all()
        assert (rays.march_t(0.0, te, step, k - 1, K) <= t_exact).all() and (t_exact <= rays.march_t(0.0, te, step, k, K)).all(), mode
        if dims == 2:
            assert (r["point"][:, 2] == 0).all()
        assert np.array_equal(rays.hit_parameter(r, mode), np.where(sign > 0, a, b))
    # no crossing: NaN brackets and points, zero sums, interval −1
    r = rays.restate(half_space, np.full((3, dims), 2.0), np.eye(dims)[:1].repeat(3, 0), 0.0, 1.0, step, 0.5, "any")
    assert (r["status"] == 0).all() and (r["interval"] == -1).all() and np.isnan(r["bracket"]).all() and np.isnan(r["point"][:, :dims]).all()
    assert np.allclose(rays.normalize([[3.0, 4.0]]), [[0.6, 0.8]]) and len(rays.hit_points(r, dims)[1]) == 0
    with pytest.raises(ValueError):
        rays.restate(half_space, np.zeros((1, dims)), np.ones((1, dims)), 0.0, 1.0, step, 0.5, "through")


# ---- restate on the enumeration of the fixture --------------------------------------------------------------------------------------
def test_restate_on_the_fixture_against_a_dense_scan_and_the_cap_for_the_gpu_seed():
    """Vertical rays over the 2-D dam-break fixture at rest: the bracket of `restate` over the O(M·N) enumeration holds the first
    crossing a plain dense scan of t finds, within step / 2²⁴.  And the cap the GPU test relies on: for its seed and rays, fewer than
    1 % of the rays evaluate a point with |S − level| < 1e-9 in the enumeration alone."""
    p, s, cfg = _fixture_cfg()
    F = np.asarray(p.Position, np.float64)[np.asarray(p.Type) == 1]
    lo, hi = F.min(0), F.max(0)
    brute = lambda x: {"weight": brute_force_weight(cfg, x, p.Position, p.Density, p.Type)}      # noqa: E731
    # (the rays of test_rays_gpu.py::test_against_brute_force.  Five long intervals: the final bracket is step / 2²⁴ ≈ 3e-8 wide, so its
    # ends lie some 1e-7 from the level in S and a point within 1e-9 of it is an accident — seeds 23 … 43 show 0 … 3 such rays of 120, 41 none; with 65 intervals it is 2e-9 wide and
    # one ray in a hundred has such a point by construction — the search converges on the level)
    o, d, te, step = gauge_rays(lo, hi, cfg.H, 120, BRUTE_K, seed=BRUTE_SEED)
    worst = 0
    for mode in rays.MODES:
        r = rays.restate(brute, o, d, 0.0, te, step, 0.5, mode)
        near = r["margin"] < 1e-9
        worst = max(worst, int(near.sum()))
        print(f"{mode}: {int((r['status'] & 1).sum())} of {len(o)} rays hit, {int(near.sum())} with an evaluated point within 1e-9 of the level, "
              f"{int(r['evaluations'].sum())} evaluations")
        assert near.sum() <= 0.01 * len(o) and (r["status"] & 1).sum() > 40
    # the dense scan: 12 rays, 2¹² points inside the march interval that holds the crossing
    r = rays.restate(brute, o, d, 0.0, te, step, 0.5, "enter")
    sel = np.flatnonzero(r["status"] & 1)[:12]
    for q in sel:
        k = r["interval"][q]
        a, b = rays.march_t(0.0, te[q], step, k - 1, BRUTE_K), rays.march_t(0.0, te[q], step, k, BRUTE_K)
        t = np.linspace(a, b, 16385)
        S = brute_force_weight(cfg, o[q] + t[:, None] * d[q], p.Position, p.Density, p.Type)
        first = np.argmax(S >= 0.5)
        assert S[0] < 0.5 <= S[first] and first >= 1
        # the first crossing of the scan lies in (t[first − 1], t[first]]; the bracket lies inside that stretch or the scan missed a thinner one
        assert t[first - 1] - step / 2 ** 24 <= r["bracket"][q, 0] and r["bracket"][q, 1] <= t[first] + step / 2 ** 24, q
        assert r["bracket"][q, 1] - r["bracket"][q, 0] <= step / 2 ** 24 + 8 * np.spacing(te[q])


# ---- the symbol -------------------------------------------------------------------------------------------------------------------
def test_header_library_and_bindings_agree():
    text = open(os.path.join(ROOT, "include", "sphmi.h")).read()
    assert re.search(r"#define\s+SPHMI_ABI_VERSION\s+5\b", text) and _abi.ABI_VERSION == 5      # append-only: the version stays
    for name, value in (("SPHMI_MAX_RAYS", _abi.MAX_RAYS), ("SPHMI_MAX_RAY_POINTS", _abi.MAX_RAY_POINTS)):
        m = re.search(r"#define\s+%s\s+\(1\s*<<\s*(\d+)\)" % name, text)
        assert m and 1 << int(m.group(1)) == value
    assert re.search(r"#define\s+SPHMI_RAY_REFINE_ROUNDS\s+4\b", text) and _abi.RAY_REFINE_ROUNDS == rays.REFINE_ROUNDS == 4
    assert re.search(r"enum\s*\{\s*SPHMI_RAY_ENTER\s*=\s*0,\s*SPHMI_RAY_LEAVE\s*=\s*1,\s*SPHMI_RAY_ANY\s*=\s*2\s*\}", text)
    assert (_abi.RAY_ENTER, _abi.RAY_LEAVE, _abi.RAY_ANY) == (0, 1, 2) and tuple(_abi.Backend.RAY_MODES) == rays.MODES
    proto = _prototype("sphmi_cast_rays")
    assert proto == ["sphmi_handle*", "int64_t"] + ["const double*"] * 4 + ["double", "double", "int32_t", "int32_t*", "int64_t*", "double*", "double*",
                                                                             "double*", "int64_t*", "double*", "double*", "double*"]
    from sphexample_amd.engine import load_library
    assert hasattr(load_library(), "sphmi_cast_rays")
    b = _backend(3)
    out = b.cast_rays(np.zeros((5, 3)), np.ones((5, 3)), 2.0, t_begin=0.5, step=0.125, level=0.4, mode="leave")
    fn = b._lib.fns["sphmi_cast_rays"]
    assert fn.argtypes == [C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_double, C.c_double, C.c_int32] + [C.c_void_p] * 9
    assert len(fn.argtypes) == len(proto) and len(fn.calls) == 1 and len(fn.calls[0]) == len(proto)
    assert fn.calls[0][1] == 5 and fn.calls[0][6:9] == (0.125, 0.4, 1)
    assert list(out) == list(_abi.Backend.RAY_FIELDS) and out["status"].dtype == np.int32 and out["interval"].dtype == out["count"].dtype == np.int64
    assert out["bracket"].shape == (5, 2) and out["point"].shape == out["sum_velocity"].shape == (5, 3) and out["weight"].shape == (5,)
    assert all(a.flags.c_contiguous for a in out.values())
    b2 = _backend(2)
    out = b2.cast_rays(np.zeros((0, 2)), np.zeros((0, 2)), 1.0, step=0.1, fields=("bracket", "status"))      # no rays travel as n = 0
    assert set(out) == {"bracket", "status"} and out["bracket"].shape == (0, 2)
    call = b2._lib.fns["sphmi_cast_rays"].calls[0]
    assert call[1] == 0 and [a is None for a in call[9:]] == [False, True, False, True, True, True, True, True, True]
    for bad in (lambda: b2.cast_rays(np.zeros((4, 3)), np.zeros((4, 3)), 1.0, step=0.1), lambda: b2.cast_rays(np.zeros((4, 2)), np.zeros((3, 2)), 1.0, step=0.1),
                lambda: b2.cast_rays(np.zeros((4, 2)), np.ones((4, 2)), 1.0, step=0.1, mode="through"),
                lambda: b2.cast_rays(np.zeros((4, 2)), np.ones((4, 2)), 1.0, step=0.1, fields=("normal",))):
        with pytest.raises(ValueError):
            bad()


def test_the_julia_shim_binds_the_symbol():
    from test_julia_shim import c_prototypes, shim_ccalls
    calls = [c for c in shim_ccalls() if c[0] == "sphmi_cast_rays"]
    assert len(calls) == 1 and len(calls[0][2]) == len(c_prototypes()["sphmi_cast_rays"][1]) == 18
    shim = open(os.path.join(ROOT, "julia", "SPHExampleMI355X.jl"), encoding="utf-8").read()
    assert shim.index("function sample_point_gradients(") < shim.index("function cast_rays(") < shim.index("function particle_fields(")


# ---- RunSimulation ----------------------------------------------------------------------------------------------------------------
class _RayStandIn(_StandIn):
    def sample_point_gradients(self, positions):
        self.log.append(("sample_point_gradients", self.iteration))
        return {"weight": np.zeros(len(positions))}

    def cast_rays(self, origins, directions, t_end, **kw):
        self.log.append(("cast_rays", self.iteration))
        n = len(origins)
        return {"status": np.ones(n, np.int32), "bracket": np.full((n, 2), float(self.iteration)), "kw": dict(kw, t_end=t_end)}


def test_run_simulation_hands_the_rays_to_the_callback():
    from conftest import load_dam_break_2d
    from sphexample_amd import simulation
    p, s = load_dam_break_2d()
    call = dict(origins=[[0.1, 1.0], [0.3, 1.0]], directions=[[0.0, -1.0]] * 2, t_end=1.0, step=0.01, mode="any")

    def run(**kw):
        meta = copy.deepcopy(s.SimMetaData)
        meta.SimulationTime, meta.OutputTimes = 0.002, 0.001
        got = []
        _StandIn.instances.clear()
        steps = simulation.RunSimulation(SimGeometry=None, SimMetaData=meta, SimConstants=s.SimConstants, SimKernel=s.SimKernel, SimLogger=None,
                                         SimParticles=p.copy(), SimViscosity=s.SimViscosity, SimDensityDiffusion=s.SimDensityDiffusion,
                                         backend_factory=_RayStandIn, on_output=lambda m, pp, *extra: got.append((m.Iteration, extra)), **kw)
        return steps, got, _StandIn.instances[0]

    steps, got, eng = run(rays=call)
    assert len(got) == len(steps) + 1 >= 3 and got[0] == (0, (None,))              # the call before the first step: nothing to cast through yet
    for iteration, extra in got[1:]:
        assert len(extra) == 1 and extra[0]["bracket"].shape == (2, 2) and (extra[0]["bracket"] == iteration).all()      # on the state of THIS output
        assert extra[0]["kw"] == {"t_end": 1.0, "step": 0.01, "mode": "any"}
    assert [e[0] for e in eng.log if isinstance(e, tuple)] == ["advance", "cast_rays", "download"] * len(steps)
    _, got2, eng2 = run(sample_point_gradients=[[0.1, 0.2]], rays=call)          # behind the gradients when both are on
    assert all(len(extra) == 2 for _, extra in got2) and "bracket" in got2[1][1][1]
    assert [e[0] for e in eng2.log if isinstance(e, tuple)][:4] == ["advance", "sample_point_gradients", "cast_rays", "download"]
    _, got3, eng3 = run()
    assert all(extra == () for _, extra in got3) and not any(e[0] == "cast_rays" for e in eng3.log if isinstance(e, tuple))


# ---- the code object --------------------------------------------------------------------------------------------------------------
def test_the_kernel_is_built_for_gfx950_within_the_budget_of_its_siblings(tmp_path):
    """The code object's metadata — read the way tests/test_point_gradients_host.py reads it — shows the four instantiations of
    k_cast_rays without scratch, without LDS and with at most the 128 registers of k_point_gradients: four waves per SIMD, the
    occupancy of the sibling on-demand kernels."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_report
    from sphexample_amd import build
    lib = build.build()
    assert hasattr(C.CDLL(lib), "sphmi_cast_rays")
    co = isa_report.code_object(lib, str(tmp_path))
    meta = isa_report.metadata(co)
    names = isa_report.demangle(list(meta))
    mine = {names[k]: v for k, v in meta.items() if "sphmi::k_cast_rays<" in names[k]}
    assert len(mine) == 4 and all(any(f"k_cast_rays<{t}, {d}>" in n for n in mine) for t in ("float", "double") for d in (2, 3)), sorted(mine)
    siblings = {names[k]: v for k, v in meta.items() if "sphmi::k_point_gradients<" in names[k] or "sphmi::k_point_cloud<" in names[k]}
    assert len(siblings) == 8
    for d, v in sorted(mine.items()):
        print(f"{d}: {v['vgprs']} VGPRs, {v['agprs']} AGPRs, {v['sgprs']} SGPRs, {v['lds_bytes']} B LDS, {v['scratch_bytes']} B scratch")
        assert v["scratch_bytes"] == 0, (d, v)
        assert v["lds_bytes"] == 0 <= min(w["lds_bytes"] for w in siblings.values()), (d, v)
        assert v["vgprs"] + v["agprs"] <= max(w["vgprs"] + w["agprs"] for w in siblings.values()) <= 128, (d, v)      # four waves per SIMD
        assert v["max_flat_workgroup_size"] == 256, (d, v)
    outlined = [d for k, d in isa_report.demangle(list(isa_report.kernels(co))).items() if k not in meta]
    assert not outlined, outlined[:4]
