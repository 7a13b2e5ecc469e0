#!/usr/bin/env python3
"""What a moment sample costs (sphmi_sample_point_moments) next to sphmi_sample_point_gradients on the same cloud, in the same
process: the bench's 1 M-particle case (C3), a few steps in ("at rest") and, with --time, at that simulated time ("developed
flow").  The cloud is the ~1e6 nodes of the lattice of tools/field_grid_cost.py handed over as points.

    python tools/point_moments_cost.py [--steps 20] [--time 0.4] [--reps 5] [--clouds N] [--still-wedge]

Per call, medians over --reps calls after one untimed call (which allocates): `kernel` ms of a call with every output NULL (upload,
bin, kernels), `all` ms of a call that delivers every output; and, on stderr, the library's own line per call with
SPHMI_POINTS_CLOCK set — the device time of bin / sample / fetch.  The ratio moments : gradients is printed with both; the walk is
the same, with 30 sums against 24 per accepted row and one kernel evaluation fewer.  The case is bench.py's: the dam-break
lattice at dp = 0.00425 generated on the device, fp32 kernels.

--clouds N: instead of the above, N clocked calls of sphmi_sample_point_moments on each of the three clouds of
tools/sample_points_cost.py (lattice, scattered, sphere): the clouds of few points per tile, where a workgroup does little besides
its prologue.

--still-wedge: a demonstration, not a measurement of time.  The StillWedge fixture (2-D, mDBC, fp64) advanced to --settle seconds;
at the boundary rows that touch the water — the bed, the wedge's faces — the Shepard pressure of sphmi_sample_points, the fitted
pressure of fields.linear_fit and ρ₀ g times the depth below the free surface found above the point (rays.water_level)."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
from field_grid_cost import DP, lattice, timed  # noqa: E402
from sphexample_amd.cases import setup_dam_break_3d  # noqa: E402
from sphexample_amd.engine import make_generated_dam_break_engine  # noqa: E402
from sphexample_amd.fields import grid_nodes  # noqa: E402


def measure(eng, label, reps):
    g = eng._fn("sample_point_gradients")
    m = eng._fn("sample_point_moments")
    x = np.ascontiguousarray(grid_nodes(*lattice(1e6)))
    px = x.ctypes.data_as(C.c_void_p)
    os.environ.pop("SPHMI_POINTS_CLOCK", None)
    gk = timed(lambda: eng._check(g(eng._h, len(x), px, *[None] * 9)), reps)
    mk = timed(lambda: eng._check(m(eng._h, len(x), px, *[None] * 10)), reps)
    ga = timed(lambda: eng.sample_point_gradients(x), reps)
    ma = timed(lambda: eng.sample_point_moments(x), reps)
    wet = int((eng.sample_point_moments(x, fields=("count",))["count"] > 0).sum())
    print(f"[{label}] {len(x)} points, {wet} see water", flush=True)
    print(f"[{label}] sphmi_sample_point_gradients: kernel {gk[0]:.2f} ms (min {gk[1]:.2f}, max {gk[2]:.2f}), all fields {ga[0]:.2f} ms (min {ga[1]:.2f}, max {ga[2]:.2f})", flush=True)
    print(f"[{label}] sphmi_sample_point_moments:   kernel {mk[0]:.2f} ms (min {mk[1]:.2f}, max {mk[2]:.2f}), all fields {ma[0]:.2f} ms (min {ma[1]:.2f}, max {ma[2]:.2f})", flush=True)
    print(f"[{label}] ratio moments : gradients: call without outputs {mk[0] / gk[0]:.2f}, call with all outputs {ma[0] / ga[0]:.2f}", flush=True)
    os.environ["SPHMI_POINTS_CLOCK"] = "1"
    for name, call in (("sample_point_gradients", eng.sample_point_gradients), ("sample_point_moments", eng.sample_point_moments)):
        for rep in range(3):                                                      # three lines each: the spread of the device time
            sys.stderr.write(f"[{label}] {name}, all fields: "); sys.stderr.flush()
            call(x)
    os.environ.pop("SPHMI_POINTS_CLOCK", None)


def clouds(eng, label, clocked):
    from field_grid_cost import TANK_HI, TANK_LO
    from sample_points_cost import sphere
    rng = np.random.default_rng(5)
    for name, x in (("lattice", grid_nodes(*lattice(1e6))), ("scattered", rng.uniform(TANK_LO, TANK_HI, (1024, 3))), ("sphere", sphere(100000, rng))):
        x = np.ascontiguousarray(x)
        eng.sample_point_moments(x)                                                   # (untimed: allocates)
        os.environ["SPHMI_POINTS_CLOCK"] = "1"
        for _ in range(clocked):
            sys.stderr.write(f"[{label}] cloud {name}, all fields: "); sys.stderr.flush()
            eng.sample_point_moments(x)
        os.environ.pop("SPHMI_POINTS_CLOCK", None)


def still_wedge_handle(settle):
    """The settled StillWedge handle, its setup, the boundary rows that touch the water and where each lies (bed, wall, wedge);
    tools/probe_moments_cost.py puts its per-step probes at the same rows."""
    from sphexample_amd import AllocateDataStructures, Fixed, Fluid, Geometry, LoadMDBCNormals
    from sphexample_amd.cases import setup_still_wedge_mdbc
    from sphexample_amd.engine import make_engine
    inp = os.path.join(ROOT, "tests", "golden", "input")
    p = AllocateDataStructures([Geometry(CSVFile=os.path.join(inp, "StillWedge_Dp0.02_Bound.csv"), GroupMarker=1, Type=Fixed, Dimensions=2),
                                Geometry(CSVFile=os.path.join(inp, "StillWedge_Dp0.02_Fluid.csv"), GroupMarker=2, Type=Fluid, Dimensions=2)])
    LoadMDBCNormals(p, os.path.join(inp, "StillWedge_Dp0.02_GhostNodes_Correct.csv"))
    s = setup_still_wedge_mdbc()
    eng = make_engine(p, s, device_float_bytes=8)
    t0 = time.perf_counter()
    pr = eng.advance(settle)
    d = eng.download(("Position", "Velocity", "Type"))
    F, B = d["Position"][d["Type"] == 1].astype(np.float64), d["Position"][d["Type"] != 1].astype(np.float64)
    dx, h, H = eng.cfg.dx, eng.cfg.h, eng.cfg.H
    print(f"[StillWedge, fp64] advanced to t = {pr.total_time:.3f} s, iteration {pr.iteration}, in {time.perf_counter() - t0:.1f} s; largest |v| of the fluid "
          f"{np.sqrt((d['Velocity'][d['Type'] == 1].astype(np.float64) ** 2).sum(1)).max():.3g} m/s; dx {dx}, h {h:.4g}, H {H:.4g}", flush=True)
    # the boundary rows that touch the water: a Fluid row within 1.5 dx
    near = np.array([((F - b) ** 2).sum(1).min() <= (1.5 * dx) ** 2 for b in B])
    pts = np.ascontiguousarray(B[near])
    bed = np.abs(pts[:, 1] - pts[:, 1].min()) < 1e-9
    wall = (np.abs(pts[:, 0] - pts[:, 0].min()) < 0.5 * dx) | (np.abs(pts[:, 0] - pts[:, 0].max()) < 0.5 * dx)
    where = np.where(bed, "bed", np.where(wall, "wall", "wedge"))
    return eng, s, pts, where


def still_wedge(settle):
    from sphexample_amd.fields import linear_fit
    from sphexample_amd.rays import water_level
    eng, s, pts, where = still_wedge_handle(settle)
    d = eng.download(("Position", "Type"))
    F = d["Position"][d["Type"] == 1].astype(np.float64)
    h, H = eng.cfg.h, eng.cfg.H
    shep = eng.sample_points(pts)
    fit = linear_fit(eng.sample_point_moments(pts))
    level = water_level(eng, pts[:, 0], F[:, 1].max() + 2 * H, pts[:, 1].min())
    hydro = s.SimConstants.rho0 * s.SimConstants.g * (level - pts[:, 1])
    ok = fit["linear"] & np.isfinite(level) & (level - pts[:, 1] > H)             # below the surface layer: the bias of the WALL, not of the surface
    print(f"[StillWedge] {len(pts)} boundary rows touch the water, {int(ok.sum())} fitted and deeper than H below the free surface "
          f"(level {np.nanmin(level):.4f} … {np.nanmax(level):.4f} m)", flush=True)
    print("[StillWedge] where   points   rho0 g depth (mean, Pa)   Shepard - hydrostatic (mean, Pa)   fitted - hydrostatic (mean, Pa)   in units of rho0 g h: Shepard, fitted", flush=True)
    unit = s.SimConstants.rho0 * s.SimConstants.g * h
    for name in ("bed", "wedge", "wall"):
        k = ok & (where == name)
        if not k.any():
            continue
        es, ef = shep["pressure"][k] - hydro[k], fit["pressure"][k] - hydro[k]
        print(f"[StillWedge] {name:6s} {int(k.sum()):6d}   {hydro[k].mean():10.1f}   {es.mean():+10.1f} (rms {np.sqrt((es ** 2).mean()):.1f})   "
              f"{ef.mean():+10.1f} (rms {np.sqrt((ef ** 2).mean()):.1f})   {es.mean() / unit:+.3f}, {ef.mean() / unit:+.3f}", flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--time", type=float, default=0.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--clouds", type=int, default=0)
    ap.add_argument("--still-wedge", action="store_true")
    ap.add_argument("--settle", type=float, default=1.0)
    args = ap.parse_args()
    if args.still_wedge:
        still_wedge(args.settle)
        return
    eng = make_generated_dam_break_engine(DP, setup_dam_break_3d(DP), device_float_bytes=4)
    eng.advance(1e9, max_steps=args.steps)
    if args.clouds > 0:
        clouds(eng, f"N={eng.N}, fp32, {args.steps} steps in", args.clouds)
        eng.close()
        return
    measure(eng, f"N={eng.N}, fp32, {args.steps} steps in", args.reps)
    if args.time > 0:
        t0 = time.perf_counter()
        pr = eng.advance(args.time)
        print(f"advanced to t = {pr.total_time:.4f} s, iteration {pr.iteration}, in {time.perf_counter() - t0:.1f} s", flush=True)
        measure(eng, f"N={eng.N}, fp32, t = {pr.total_time:.3f} s", args.reps)
    eng.close()


if __name__ == "__main__":
    main()
