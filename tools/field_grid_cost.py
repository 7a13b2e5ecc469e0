#!/usr/bin/env python3
"""What a lattice sample costs (sphmi_sample_grid): the bench's 1 M-particle case (C3) a few steps in, lattices of about 1e4, 1e5,
1e6 and 1e7 nodes over the whole tank, next to a full sphmi_download of the same handle as a yardstick.

    python tools/field_grid_cost.py [--steps 20] [--reps 5] [--nodes 1e4,1e5,1e6,1e7]

Per lattice size, medians over --reps calls after one untimed call (which allocates the arena):
  kernel   ms of a call with every output NULL: the sums are formed in the device arena, nothing is delivered
  weight   ms of a call that delivers S alone (one copy, no host pass)
  all      ms of a call that delivers all five fields (seven copies and the host's normalisation)
The case is bench.py's: the dam-break lattice at dp = 0.00425 generated on the device, fp32 kernels."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from sphexample_amd.cases import setup_dam_break_3d  # noqa: E402
from sphexample_amd.engine import make_generated_dam_break_engine  # noqa: E402

DP = 0.00425
TANK_LO, TANK_HI = np.array([-0.01, -0.01, -0.01]), np.array([1.62, 0.68, 0.46])


def lattice(n_nodes):
    """About n_nodes nodes, the same spacing on every axis, over the tank; the origin knows nothing of the particle lattice."""
    ext = TANK_HI - TANK_LO
    s = (ext.prod() / n_nodes) ** (1.0 / 3.0)
    counts = np.maximum(np.round(ext / s).astype(np.int64), 1)
    return TANK_LO + np.array([0.318309886, 0.577215665, 0.693147181]) * DP, np.full(3, s), counts


def timed(f, reps):
    f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nodes", default="1e4,1e5,1e6,1e7")
    args = ap.parse_args()
    eng = make_generated_dam_break_engine(DP, setup_dam_break_3d(DP), device_float_bytes=4)
    eng.advance(1e9, max_steps=args.steps)
    d = eng.download()
    med, lo, hi = timed(lambda: eng.download(), args.reps)
    print(f"[dam break 3-D, N={eng.N}, fp32, {args.steps} steps in] full sphmi_download into fresh arrays: {med:.2f} ms (min {lo:.2f}, max {hi:.2f})", flush=True)
    into = {k: np.empty_like(v) for k, v in d.items()}
    f = eng._fn("download")
    order = ("Position", "Velocity", "Acceleration", "Density", "Pressure", "ID", "Type", "GroupMarker", "GhostPoints", "Cells")
    ptrs = [into[k].ctypes.data_as(C.c_void_p) for k in order]
    med, lo, hi = timed(lambda: eng._check(f(eng._h, *ptrs)), args.reps)
    print(f"[dam break 3-D, N={eng.N}] full sphmi_download into the same arrays: {med:.2f} ms (min {lo:.2f}, max {hi:.2f})", flush=True)
    g = eng._fn("sample_grid")
    for n in [float(x) for x in args.nodes.split(",")]:
        o, s, c = lattice(n)
        nodes = int(c.prod())
        po, ps, pc = [a.ctypes.data_as(C.c_void_p) for a in (o, s, c)]
        k = timed(lambda: eng._check(g(eng._h, po, ps, pc, *[None] * 5)), args.reps)
        w = np.empty(tuple(int(v) for v in c[::-1]))
        pw = w.ctypes.data_as(C.c_void_p)
        ww = timed(lambda: eng._check(g(eng._h, po, ps, pc, pw, None, None, None, None)), args.reps)
        a = timed(lambda: eng.sample_grid(o, s, c), args.reps)
        print(f"lattice {tuple(int(v) for v in c)} = {nodes} nodes, spacing {s[0] / eng.cfg.H:.3f} H, {int((w > 0).sum())} nodes see water: "
              f"kernel {k[0]:.2f} ms (min {k[1]:.2f}, max {k[2]:.2f}), weight {ww[0]:.2f} ms, all fields {a[0]:.2f} ms (min {a[1]:.2f}, max {a[2]:.2f})", flush=True)
    eng.close()


if __name__ == "__main__":
    main()
