#!/usr/bin/env python3
"""What the per-particle differential fields cost (sphmi_particle_fields): the bench's 1 M-particle case (C3) a few steps in, next
to the two things a user does without the call — a full sphmi_download alone, and that download plus a neighbour search on the host.

    python tools/particle_fields_cost.py [--steps 20] [--reps 5] [--host-rows 2048]

Medians over --reps calls after one untimed call (which allocates the arena):
  kernel     ms of a call with every output NULL: the sums are formed in the device arena, nothing is delivered
  vorticity  ms of a call that delivers the vorticity alone (one copy of N x 3 doubles)
  all        ms of a call that delivers all six fields
  download   ms of a full sphmi_download into the same arrays
  host       s of the neighbour search alone on the downloaded positions — the pairs within H, before any sum is formed:
             scipy.spatial.cKDTree.query_ball_point over all rows where scipy is importable (the line says so), else the chunked numpy
             enumeration of --host-rows target rows against all N, scaled by N / rows (the line says that instead)
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


def timed(f, reps):
    f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def host_search(X, H, rows):
    """Seconds of the neighbour search alone, and how it was done."""
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None
    workers = int(os.environ.get("OMP_NUM_THREADS", "16"))
    if cKDTree is not None:
        t0 = time.perf_counter()
        n = cKDTree(X).query_ball_point(X, H, workers=workers, return_length=True)
        return time.perf_counter() - t0, f"scipy.spatial.cKDTree, all {len(X)} rows, {workers} workers, mean {n.mean() - 1:.1f} neighbours"
    pick = np.random.default_rng(5).choice(len(X), rows, replace=False)
    t0 = time.perf_counter()
    total = 0
    for a in range(0, rows, 64):
        d = X[pick[a:a + 64], None, :] - X[None, :, :]
        total += int(((d * d).sum(-1) <= H * H).sum())
    return (time.perf_counter() - t0) * len(X) / rows, f"numpy enumeration of {rows} rows against all, scaled by {len(X) / rows:.0f}, mean {total / rows - 1:.1f} neighbours"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-rows", type=int, default=2048)
    args = ap.parse_args()
    eng = make_generated_dam_break_engine(DP, setup_dam_break_3d(DP), device_float_bytes=4)
    eng.advance(1e9, max_steps=args.steps)
    d = eng.download()
    order = ("Position", "Velocity", "Acceleration", "Density", "Pressure", "ID", "Type", "GroupMarker", "GhostPoints", "Cells")
    f = eng._fn("download")
    ptrs = [d[k].ctypes.data_as(C.c_void_p) for k in order]
    dl = timed(lambda: eng._check(f(eng._h, *ptrs)), args.reps)
    print(f"[dam break 3-D, N={eng.N}, fp32, {args.steps} steps in] full sphmi_download into the same arrays: {dl[0]:.2f} ms (min {dl[1]:.2f}, max {dl[2]:.2f})", flush=True)
    g = eng._fn("particle_fields")
    k = timed(lambda: eng._check(g(eng._h, *[None] * 6)), args.reps)
    w = np.empty((eng.N, 3))
    v = timed(lambda: eng._check(g(eng._h, None, None, None, None, None, w.ctypes.data_as(C.c_void_p))), args.reps)
    a = timed(lambda: eng.particle_fields(), args.reps)
    out = eng.particle_fields()
    print(f"sphmi_particle_fields: kernel {k[0]:.2f} ms (min {k[1]:.2f}, max {k[2]:.2f}), vorticity alone {v[0]:.2f} ms (min {v[1]:.2f}, max {v[2]:.2f}), "
          f"all six fields {a[0]:.2f} ms (min {a[1]:.2f}, max {a[2]:.2f}); mean n {out['count'].mean():.1f}, max |w| {np.abs(out['vorticity']).max():.3g}", flush=True)
    secs, how = host_search(np.ascontiguousarray(d["Position"], dtype=np.float64), eng.cfg.H, args.host_rows)
    print(f"host neighbour search alone ({how}): {secs:.2f} s; with the download {secs + dl[0] / 1e3:.2f} s", flush=True)
    eng.close()


if __name__ == "__main__":
    main()
