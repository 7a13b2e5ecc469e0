#!/usr/bin/env python3
"""What the per-step moment sums cost (sphmi_probe_moments_enable): the bench's 1 M-particle case (BASELINE config 3, 1 057 738 rows,
fp32) disabled, with 256 fixed probes (sphmi_probes_enable) and with 256 moment probes at the same points; with --lib the first two
also on another build of the library (the parent commit's: the probes before pr_walk was factored), with --alt-lib the moment probes
on a third build (another kPmInFlight).  Repetitions interleaved on one GPU, the procedure and the step timing of
tools/tracers_cost.py: every handle is measured AT REST and on DEVELOPED FLOW at t = `--developed` s, the observer enabled again
there on points drawn from the Fluid rows of that state, the same ones for every variant.

    python tools/probe_moments_cost.py [--steps 60] [--warmup 5] [--reps 3] [--lib PATH] [--alt-lib PATH] [--developed 0.4]
                                       [--developed-steps 200] [--out DIR]
    python tools/probe_moments_cost.py --still-wedge [--settle 1.0] [--run-steps 64]

--still-wedge: a demonstration, not a measurement of time.  The StillWedge fixture (2-D, mDBC, fp64) advanced to --settle seconds;
probes and moment probes at the boundary rows that touch the water, --run-steps more steps, then per step the Shepard pressure of
sphmi_probes_read and the fitted pressure of probes.fit_series against rho0 g (level - y): the figures of
tools/point_moments_cost.py --still-wedge, at every step instead of on demand (the last line repeats the on-demand call on the
state after the run)."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

VARIANTS = ("disabled", "256 probes", "256 probe moments")
COUNT = 256


def enable(eng, variant, seed, capacity):
    """Points off the Fluid rows the handle holds now: the same draw for every variant."""
    if variant == "disabled":
        return
    d = eng.download(("Position", "Type"))
    fluid = np.flatnonzero(d["Type"] == 1)
    rng = np.random.default_rng(seed)
    points = d["Position"][rng.choice(fluid, COUNT, replace=False)].astype(np.float64) + rng.uniform(-0.002, 0.002, (COUNT, 3))
    (eng.probes_enable if variant == "256 probes" else eng.probe_moments_enable)(points, capacity=capacity)


def windows(variant, args):
    """(ms per step at rest, ms per step on developed flow, rows, rebuilds in the developed window, probes with S >= 0.5 at the end)"""
    from group_forces_cost import DP, precondition
    from sphexample_amd.cases import setup_dam_break_3d
    from sphexample_amd.engine import make_generated_dam_break_engine
    eng = make_generated_dam_break_engine(DP, setup_dam_break_3d(DP), device_float_bytes=4)
    enable(eng, variant, 1, 4096)
    precondition()
    eng.advance(1e9, max_steps=args.warmup)
    t0 = time.perf_counter()
    pr = eng.advance(1e9, max_steps=args.steps)
    rest = (time.perf_counter() - t0) / args.steps * 1e3
    assert pr.steps_done == args.steps
    developed, rebuilds, wet = float("nan"), 0, -1
    if args.developed > 0:
        r0 = eng.advance(args.developed).n_rebuilds
        enable(eng, variant, 2, args.developed_steps)
        t0 = time.perf_counter()
        pr = eng.advance(1e9, max_steps=args.developed_steps)
        developed = (time.perf_counter() - t0) / args.developed_steps * 1e3
        assert pr.steps_done == args.developed_steps
        rebuilds = int(pr.n_rebuilds - r0)
    if variant != "disabled":
        r = eng.probes_read() if variant == "256 probes" else eng.probe_moments_read()
        assert len(r["iteration"]) == min(pr.iteration, args.developed_steps if args.developed > 0 else 4096)
        wet = int((r["weight"][-1] >= 0.5).sum())
    N = eng.N
    eng.close()
    return rest, developed, N, rebuilds, wet


def other_library(lib, variant, args):
    """the same two windows of `variant` with another build, in a child process (a process loads one libsphmi.so)"""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", variant, "--lib", lib, "--steps", str(args.steps), "--warmup", str(args.warmup),
           "--developed", str(args.developed), "--developed-steps", str(args.developed_steps)]
    out = subprocess.run(cmd, capture_output=True, text=True, check=True).stdout
    rest, developed, N, rebuilds, wet = [ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1].split()[1:]
    return float(rest), float(developed), int(N), int(rebuilds), int(wet)


def still_wedge(settle, run_steps):
    from point_moments_cost import still_wedge_handle
    from sphexample_amd.fields import linear_fit
    from sphexample_amd.probes import fit_series
    from sphexample_amd.rays import water_level
    eng, s, pts, where = still_wedge_handle(settle)
    H, h = eng.cfg.H, eng.cfg.h
    unit = s.SimConstants.rho0 * s.SimConstants.g * h
    eng.probes_enable(pts, capacity=run_steps)
    eng.probe_moments_enable(pts, capacity=run_steps)
    pr = eng.advance(1e9, max_steps=run_steps)
    shep, fit = eng.probes_read(), fit_series(eng.probe_moments_read())
    assert len(shep["iteration"]) == run_steps == len(fit["iteration"]) and (shep["iteration"] == fit["iteration"]).all()
    F = eng.download(("Position", "Type"))
    F = F["Position"][F["Type"] == 1].astype(np.float64)
    level = water_level(eng, pts[:, 0], F[:, 1].max() + 2 * H, pts[:, 1].min())
    hydro = s.SimConstants.rho0 * s.SimConstants.g * (level - pts[:, 1])
    ok = fit["linear"].all(0) & np.isfinite(level) & (level - pts[:, 1] > H)      # below the surface layer: the bias of the WALL, not of the surface
    print(f"[StillWedge] {run_steps} steps to t = {pr.total_time:.4f} s with {len(pts)} probes and {len(pts)} moment probes; {int(ok.sum())} fitted at every step "
          f"and deeper than H below the free surface (level {np.nanmin(level):.4f} … {np.nanmax(level):.4f} m, taken after the run)", flush=True)
    print("[StillWedge] where   points   in units of rho0 g h, mean over the points — per step: Shepard (first, last, min … max over the steps) | "
          "fitted (first, last, min … max) | on demand after the run: Shepard, fitted", flush=True)
    on_demand_s, on_demand_f = eng.sample_points(pts), linear_fit(eng.sample_point_moments(pts))
    for name in ("bed", "wedge", "wall"):
        k = ok & (where == name)
        if not k.any():
            continue
        es = ((shep["pressure"][:, k] - hydro[k]) / unit).mean(1)
        ef = ((fit["pressure"][:, k] - hydro[k]) / unit).mean(1)
        ods, odf = ((on_demand_s["pressure"][k] - hydro[k]) / unit).mean(), ((on_demand_f["pressure"][k] - hydro[k]) / unit).mean()
        print(f"[StillWedge] {name:6s} {int(k.sum()):6d}   {es[0]:+.3f}, {es[-1]:+.3f}, {es.min():+.3f} … {es.max():+.3f} | "
              f"{ef[0]:+.3f}, {ef[-1]:+.3f}, {ef.min():+.3f} … {ef.max():+.3f} | {ods:+.3f}, {odf:+.3f}", flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--developed", type=float, default=0.4)
    ap.add_argument("--developed-steps", type=int, default=200)
    ap.add_argument("--lib")
    ap.add_argument("--alt-lib")
    ap.add_argument("--out")
    ap.add_argument("--still-wedge", action="store_true")
    ap.add_argument("--settle", type=float, default=1.0)
    ap.add_argument("--run-steps", type=int, default=64)
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.still_wedge:
        still_wedge(args.settle, args.run_steps)
        return
    if args.child:
        os.environ["SPHMI_LIB"] = os.path.abspath(args.lib)
        print("RESULT %.6f %.6f %d %d %d" % windows(args.child, args), flush=True)
        return
    runs = ([("parent disabled", args.lib, "disabled"), ("parent 256 probes", args.lib, "256 probes")] if args.lib else []) + [(v, None, v) for v in VARIANTS] \
        + ([("alt 256 probe moments", args.alt_lib, "256 probe moments")] if args.alt_lib else [])
    ms = {n: {"rest": [], "developed": []} for n, _, _ in runs}
    raw = []

    def say(line):
        raw.append(line)
        print(line, flush=True)

    for r in range(args.reps):
        for n, lib, variant in runs:
            rest, developed, N, rebuilds, wet = other_library(lib, variant, args) if lib else windows(variant, args)
            ms[n]["rest"].append(rest); ms[n]["developed"].append(developed)
            say(f"rep {r} {n:22s}: N={N} at rest {rest:.4f} ms/step {N / rest * 1e3:.4g} updates/s | developed (t = {args.developed} s, "
                f"{rebuilds} rebuilds in {args.developed_steps} steps) {developed:.4f} ms/step" + (f" | S >= 0.5 at the last step: {wet} of {COUNT}" if wet >= 0 else ""))
    table = ["| variant | at rest: median ms/step (min – max, spread) | against disabled | developed: median ms/step (min – max, spread) | against disabled |",
             "|---|---|---|---|---|"]
    for n, lib, variant in runs:
        cells = []
        base = "parent disabled" if n.startswith("parent") else "disabled"
        for w in ("rest", "developed"):
            v, off = ms[n][w], np.median(ms[base][w])
            med = np.median(v)
            cells += [f"{med:.4f} ({min(v):.4f} – {max(v):.4f}, {(max(v) - min(v)) / med * 100:.2f} %)",
                      "—" if variant == "disabled" else f"{1e3 * (med - off):+.1f} µs ({(med - off) / off * 100:+.2f} %)"]
        table.append(f"| {n} | " + " | ".join(cells) + " |")
    for line in table:
        say(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        libs = {args.lib: "PARENT_LIB", args.alt_lib: "ALT_LIB", args.out: "OUT_DIR"}
        with open(os.path.join(args.out, "probe_moments_raw.txt"), "w") as f:
            f.write("command: python tools/probe_moments_cost.py " + " ".join(libs.get(a, a) for a in sys.argv[1:]) + "\n" + "\n".join(raw) + "\n")


if __name__ == "__main__":
    main()
