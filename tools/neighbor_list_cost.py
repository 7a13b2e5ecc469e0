#!/usr/bin/env python3
"""What the neighbour list costs (sphmi_neighbors_build / sphmi_neighbors_read): the bench's 1 M-particle case (C3) a few steps in.

    python tools/neighbor_list_cost.py [--steps 20] [--reps 5] [--half]

Prints n_pairs and the arena bytes, then medians over --reps calls after one untimed call (which allocates the arena):
  build      ms of sphmi_neighbors_build (count + scan + fill, synchronous) by the host's clock
  read       ms of sphmi_neighbors_read of offsets and entries into pageable numpy arrays
  yardstick  ms of sphmi_particle_fields with every output NULL — the same candidate walk with 64-byte staged rows and the fp64
             kernel sums on top — three repetitions of the same median, to show their spread
With $SPHMI_NEIGHBORS_TIMING=1 (set here) the library itself writes the device time of the count, scan and fill passes of every
build to stderr, from events on its stream; the fill pass's write bandwidth is 4 · n_pairs bytes over its time.
The case is bench.py's: the dam-break lattice at dp = 0.00425 generated on the device, fp32 kernels."""
import argparse
import ctypes as C
import os
import sys
import time

os.environ.setdefault("SPHMI_NEIGHBORS_TIMING", "1")
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--half", action="store_true")
    args = ap.parse_args()
    eng = make_generated_dam_break_engine(DP, setup_dam_break_3d(DP), device_float_bytes=4)
    eng.advance(1e9, max_steps=args.steps)
    g = eng._fn("particle_fields")
    for rep in range(3):
        k = timed(lambda: eng._check(g(eng._h, *[None] * 6)), args.reps)
        print(f"[dam break 3-D, N={eng.N}, fp32, {args.steps} steps in] yardstick {rep + 1}/3: sphmi_particle_fields kernel {k[0]:.2f} ms (min {k[1]:.2f}, max {k[2]:.2f})", flush=True)
    b = timed(lambda: eng.neighbors_build(args.half), args.reps)
    rows, pairs = eng.neighbors_build(args.half)
    arena = 4 * pairs + 8 * (rows + 1) + 4 * rows + 8 * ((rows + 2047) // 2048)
    print(f"sphmi_neighbors_build ({'half' if args.half else 'full'}): {rows} rows, n_pairs {pairs} ({pairs / rows:.1f} per row), arena {arena} bytes "
          f"({4 * pairs / 1e9:.3f} GB of entries); build {b[0]:.2f} ms (min {b[1]:.2f}, max {b[2]:.2f}); "
          f"at the fill pass's time t ms its write bandwidth is {4 * pairs / 1e6:.1f} / t GB/s", flush=True)
    off, nbr = eng.neighbors_read()
    f = eng._fn("neighbors_read")
    r = timed(lambda: eng._check(f(eng._h, off.ctypes.data_as(C.c_void_p), nbr.ctypes.data_as(C.c_void_p))), args.reps)
    step = np.diff(nbr)                                                             # within a row: > 0; across a row boundary: anything
    cut = off[1:-1] - 1
    step[cut[(cut >= 0) & (cut < len(step))]] = 1
    print(f"sphmi_neighbors_read: {r[0]:.2f} ms (min {r[1]:.2f}, max {r[2]:.2f}) for {(off.nbytes + nbr.nbytes) / 1e9:.3f} GB; "
          f"rows ascending: {bool((step > 0).all())}, offsets[-1] == n_pairs: {bool(off[-1] == pairs)}, longest row {int(np.diff(off).max())}", flush=True)
    if not args.half:
        cnt = eng.particle_fields(("count",))["count"]
        print(f"row lengths equal sphmi_particle_fields' count: {bool((np.diff(off) == cnt).all())}", flush=True)
    eng.neighbors_release()
    eng.close()


if __name__ == "__main__":
    main()
