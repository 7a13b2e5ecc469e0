#!/usr/bin/env python3
"""What the free-surface mesh costs (sphmi_isosurface_build / sphmi_isosurface_read): the bench's 1 M-particle case (C3) a few steps
in, on the million-node lattice of tools/field_grid_cost.py.

    python tools/isosurface_cost.py [--steps 20] [--reps 5] [--nodes 1e6]

Prints the vertex and element counts, then medians over --reps calls after one untimed call (which allocates the arenas):
  sampler    ms of sphmi_sample_grid with every output NULL — k_field_grid alone, the yardstick the new passes stand next to
  build      ms of sphmi_isosurface_build (the sampler, classify, two scans, vertices, elements; synchronous) by the host's clock
  read       ms of sphmi_isosurface_read of vertices, elements, pressure and velocity into pageable numpy arrays
  host way   the same product as the parent commit would have to get it: sphmi_sample_grid delivering S alone, and
             sphexample_amd.isosurface.extract on it (numpy), timed apart — and whether it gives the same bytes
With $SPHMI_ISOSURFACE_TIMING=1 (set here) the library itself writes the device time of the sampler and of every pass of every build
to stderr, from events on its stream.  The sampler and the build are timed in turns, three rounds, to show their spread.
The case is bench.py's: the dam-break lattice at dp = 0.00425 generated on the device, fp32 kernels."""
import argparse
import ctypes as C
import os
import sys
import time

os.environ.setdefault("SPHMI_ISOSURFACE_TIMING", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
from field_grid_cost import DP, lattice, timed  # noqa: E402
from sphexample_amd import isosurface  # noqa: E402
from sphexample_amd.cases import setup_dam_break_3d  # noqa: E402
from sphexample_amd.engine import make_generated_dam_break_engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nodes", type=float, default=1e6)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy extraction (minutes at 1e7 nodes)")
    args = ap.parse_args()
    eng = make_generated_dam_break_engine(DP, setup_dam_break_3d(DP), device_float_bytes=4)
    eng.advance(1e9, max_steps=args.steps)
    o, s, c = lattice(args.nodes)
    nodes = int(c.prod())
    g = eng._fn("sample_grid")
    po, ps, pc = [a.ctypes.data_as(C.c_void_p) for a in (o, s, c)]
    print(f"[dam break 3-D, N={eng.N}, fp32, {args.steps} steps in] lattice {tuple(int(v) for v in c)} = {nodes} nodes, spacing {s[0] / eng.cfg.H:.3f} H", flush=True)
    for rep in range(3):
        k = timed(lambda: eng._check(g(eng._h, po, ps, pc, *[None] * 5)), args.reps)
        b = timed(lambda: eng.isosurface_build(o, s, c), args.reps)
        print(f"round {rep + 1}/3: sampler alone {k[0]:.3f} ms (min {k[1]:.3f}, max {k[2]:.3f}); sphmi_isosurface_build {b[0]:.3f} ms (min {b[1]:.3f}, max {b[2]:.3f})", flush=True)
    nv, ne = eng.isosurface_build(o, s, c)
    arena = 25 * nodes + 56 * nv + 12 * ne
    print(f"mesh: {nv} vertices, {ne} triangles; arena {arena} bytes ({25 * nodes} per-node, {56 * nv + 12 * ne} mesh)", flush=True)
    mesh = eng.isosurface_read(pressure=True, velocity=True)
    f = eng._fn("isosurface_read")
    r = timed(lambda: eng._check(f(eng._h, *[a.ctypes.data_as(C.c_void_p) for a in mesh])), args.reps)
    print(f"sphmi_isosurface_read: {r[0]:.3f} ms (min {r[1]:.3f}, max {r[2]:.3f}) for {sum(a.nbytes for a in mesh) / 1e6:.2f} MB", flush=True)
    w = np.empty(tuple(int(v) for v in c[::-1]))
    pw = w.ctypes.data_as(C.c_void_p)
    ww = timed(lambda: eng._check(g(eng._h, po, ps, pc, pw, None, None, None, None)), args.reps)
    print(f"host way: sphmi_sample_grid delivering S ({w.nbytes / 1e6:.1f} MB): {ww[0]:.3f} ms (min {ww[1]:.3f}, max {ww[2]:.3f})", flush=True)
    if not args.no_host:
        t0 = time.perf_counter()
        v, e = isosurface.extract(w, o, s, 0.5)
        dt = time.perf_counter() - t0
        print(f"host way: isosurface.extract (numpy) {dt * 1e3:.0f} ms; same vertices {v.tobytes() == mesh[0].tobytes()}, same elements {bool(np.array_equal(e, mesh[1]))}; "
              f"closed {isosurface.is_closed(v, e)}, area {isosurface.surface_area(v, e):.4f} m^2, volume {isosurface.enclosed_volume(v, e):.5f} m^3", flush=True)
    eng.isosurface_release()
    eng.close()


if __name__ == "__main__":
    main()
