#!/usr/bin/env python3
"""What a gradient sample costs (sphmi_sample_point_gradients) next to sphmi_sample_points on the same cloud and box: the bench's
1 M-particle case (C3), a few steps in ("at rest") and, with --time, at that simulated time ("developed flow").  The cloud is the
~1e6 nodes of the lattice of tools/field_grid_cost.py handed over as points.

    python tools/point_gradients_cost.py [--steps 20] [--time 0.4] [--reps 5]

Per call, medians over --reps calls after one untimed call (which allocates): `kernel` ms of a call with every output NULL (upload,
bin, kernel), `all` ms of a call that delivers every output; and, on stderr, the library's own line per call with SPHMI_POINTS_CLOCK
set — the device time of bin / sample / fetch.  The ratio gradients : sample_points is printed with both.  The case is bench.py's:
the dam-break lattice at dp = 0.00425 generated on the device, fp32 kernels."""
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
    f = eng._fn("sample_points")
    g = eng._fn("sample_point_gradients")
    x = np.ascontiguousarray(grid_nodes(*lattice(1e6)))
    px = x.ctypes.data_as(C.c_void_p)
    os.environ.pop("SPHMI_POINTS_CLOCK", None)
    sk = timed(lambda: eng._check(f(eng._h, len(x), px, *[None] * 5)), reps)
    sa = timed(lambda: eng.sample_points(x), reps)
    gk = timed(lambda: eng._check(g(eng._h, len(x), px, *[None] * 9)), reps)
    ga = timed(lambda: eng.sample_point_gradients(x), reps)
    wet = int((eng.sample_points(x, fields=("count",))["count"] > 0).sum())
    print(f"[{label}] {len(x)} points, {wet} see water", flush=True)
    print(f"[{label}] sphmi_sample_points:          kernel {sk[0]:.2f} ms (min {sk[1]:.2f}, max {sk[2]:.2f}), all fields {sa[0]:.2f} ms (min {sa[1]:.2f}, max {sa[2]:.2f})", flush=True)
    print(f"[{label}] sphmi_sample_point_gradients: kernel {gk[0]:.2f} ms (min {gk[1]:.2f}, max {gk[2]:.2f}), all fields {ga[0]:.2f} ms (min {ga[1]:.2f}, max {ga[2]:.2f})", flush=True)
    print(f"[{label}] ratio gradients : sample_points: call without outputs {gk[0] / sk[0]:.2f}, call with all outputs {ga[0] / sa[0]:.2f}", flush=True)
    os.environ["SPHMI_POINTS_CLOCK"] = "1"
    for name, call in (("sample_points", eng.sample_points), ("sample_point_gradients", eng.sample_point_gradients)):
        sys.stderr.write(f"[{label}] {name}, all fields: "); sys.stderr.flush()
        call(x)
    os.environ.pop("SPHMI_POINTS_CLOCK", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--time", type=float, default=0.0)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    eng = make_generated_dam_break_engine(DP, setup_dam_break_3d(DP), device_float_bytes=4)
    eng.advance(1e9, max_steps=args.steps)
    measure(eng, f"N={eng.N}, fp32, {args.steps} steps in", args.reps)
    if args.time > 0:
        t0 = time.perf_counter()
        pr = eng.advance(args.time)
        print(f"advanced to t = {pr.total_time:.4f} s, iteration {pr.iteration}, in {time.perf_counter() - t0:.1f} s", flush=True)
        measure(eng, f"N={eng.N}, fp32, t = {pr.total_time:.3f} s", args.reps)
    eng.close()


if __name__ == "__main__":
    main()
