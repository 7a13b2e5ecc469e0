#!/usr/bin/env python3
"""What a point-cloud sample costs (sphmi_sample_points): the bench's 1 M-particle case (C3), a few steps in ("at rest") and, with
--time, at that simulated time, three clouds:

  lattice   the nodes of the ~1e6-node lattice of tools/field_grid_cost.py handed over as a cloud, next to sphmi_sample_grid on the
            same lattice in the same run: what binning and ragged tiles cost
  scattered 1 024 points drawn uniformly over the tank, next to what one step costs more with the same points as probes
  sphere    100 000 points on a sphere round the obstacle: the surface-load use

    python tools/sample_points_cost.py [--steps 20] [--time 0.4] [--reps 5] [--clocked 1]

Per cloud, medians over --reps calls after one untimed call (which allocates): `kernel` ms of a call with every output NULL, `all` ms
of a call that delivers all five fields; and, on stderr, the library's own line per call with SPHMI_POINTS_CLOCK set — the device
time of bin / sample / fetch, the number of tiles and the mean lanes filled; --clocked N makes N such calls per cloud, for a median
of the device time.  The case is bench.py's: the dam-break lattice at
dp = 0.00425 generated on the device, fp32 kernels."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
from field_grid_cost import DP, TANK_HI, TANK_LO, lattice, timed  # noqa: E402
from sphexample_amd.cases import setup_dam_break_3d  # noqa: E402
from sphexample_amd.engine import make_generated_dam_break_engine  # noqa: E402
from sphexample_amd.fields import grid_nodes  # noqa: E402

OBSTACLE, RADIUS = np.array([0.96, 0.335, 0.10]), 0.15             # a sphere that encloses the obstacle's box, floor included


def sphere(n, rng):
    v = rng.normal(size=(n, 3))
    return OBSTACLE + RADIUS * v / np.linalg.norm(v, axis=1)[:, None]


def measure(eng, label, reps, clocked=1):
    f = eng._fn("sample_points")
    g = eng._fn("sample_grid")
    rng = np.random.default_rng(5)
    o, s, c = lattice(1e6)
    nodes = grid_nodes(o, s, c)
    clouds = {"lattice": nodes, "scattered": rng.uniform(TANK_LO, TANK_HI, (1024, 3)), "sphere": sphere(100000, rng)}
    for name, x in clouds.items():
        x = np.ascontiguousarray(x)
        px = x.ctypes.data_as(C.c_void_p)
        os.environ.pop("SPHMI_POINTS_CLOCK", None)
        k = timed(lambda: eng._check(f(eng._h, len(x), px, *[None] * 5)), reps)
        a = timed(lambda: eng.sample_points(x), reps)
        wet = int((eng.sample_points(x, fields=("count",))["count"] > 0).sum())
        print(f"[{label}] cloud {name}: {len(x)} points, {wet} see water: kernel {k[0]:.2f} ms (min {k[1]:.2f}, max {k[2]:.2f}), "
              f"all fields {a[0]:.2f} ms (min {a[1]:.2f}, max {a[2]:.2f})", flush=True)
        os.environ["SPHMI_POINTS_CLOCK"] = "1"
        for _ in range(clocked):
            sys.stderr.write(f"[{label}] cloud {name}, all fields: "); sys.stderr.flush()
            eng.sample_points(x)
        os.environ.pop("SPHMI_POINTS_CLOCK", None)
        if name == "lattice":
            po, ps, pc = [v.ctypes.data_as(C.c_void_p) for v in (o, s, c)]
            gk = timed(lambda: eng._check(g(eng._h, po, ps, pc, *[None] * 5)), reps)
            ga = timed(lambda: eng.sample_grid(o, s, c), reps)
            same = all(np.array_equal(v.reshape(-1), eng.sample_points(x)[q].reshape(-1)) for q, v in eng.sample_grid(o, s, c).items())
            print(f"[{label}] sphmi_sample_grid on the same lattice {tuple(int(v) for v in c)}: kernel {gk[0]:.2f} ms (min {gk[1]:.2f}, max {gk[2]:.2f}), "
                  f"all fields {ga[0]:.2f} ms (min {ga[1]:.2f}, max {ga[2]:.2f}); the cloud's results bit-identical: {same}", flush=True)
    return clouds["scattered"]


def probe_step(eng, points, label, steps=20):
    """What `steps` steps cost with and without the 1 024 points as probes: the difference per step."""
    def run():
        t0 = time.perf_counter()
        eng.advance(1e9, max_steps=steps)
        return (time.perf_counter() - t0) * 1e3 / steps
    run()
    plain = [run() for _ in range(3)]
    eng.probes_enable(points, capacity=4 * steps)
    run()
    probed = [run() for _ in range(3)]
    eng.probes_read()
    eng.probes_enable(np.zeros((0, 3)), capacity=1)
    print(f"[{label}] a step with the 1 024 points as probes: {np.median(probed):.3f} ms against {np.median(plain):.3f} ms without "
          f"({np.median(probed) - np.median(plain):+.3f} ms per step; {steps} steps per sample, 3 samples each)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--time", type=float, default=0.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--clocked", type=int, default=1)
    args = ap.parse_args()
    eng = make_generated_dam_break_engine(DP, setup_dam_break_3d(DP), device_float_bytes=4)
    eng.advance(1e9, max_steps=args.steps)
    label = f"N={eng.N}, fp32, {args.steps} steps in"
    scattered = measure(eng, label, args.reps, args.clocked)
    probe_step(eng, scattered, label)
    if args.time > 0:
        t0 = time.perf_counter()
        pr = eng.advance(args.time)
        print(f"advanced to t = {pr.total_time:.4f} s, iteration {pr.iteration}, in {time.perf_counter() - t0:.1f} s", flush=True)
        label = f"N={eng.N}, fp32, t = {pr.total_time:.3f} s"
        measure(eng, label, args.reps, args.clocked)
        probe_step(eng, scattered, label)
    eng.close()


if __name__ == "__main__":
    main()
