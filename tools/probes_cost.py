#!/usr/bin/env python3
"""What the per-step probes cost (sphmi_probes_enable): the bench's 1 M-particle window (C3) with 0, 8, 512 and 1024 probes,
repetitions interleaved on one GPU.  Prints one line per run and a summary per probe count: µs per step, the difference to
the runs without probes, the spread of those.

    python tools/probes_cost.py [--steps 60] [--warmup 5] [--reps 3] [--counts 0,8,512,1024]

The case is bench.py's: the dam-break lattice at dp = 0.00425 generated on the device, fp32 kernels, 60 ms of untimed
pre-conditioning on a scratch handle before every window, W warm-up steps, K timed steps.  The probes: a regular lattice of points
through the water column and the obstacle's front face (every probe has neighbours: the expensive kind)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from sphexample_amd.cases import setup_dam_break_3d  # noqa: E402
from sphexample_amd.engine import make_generated_dam_break_engine  # noqa: E402

DP = 0.00425


def precondition(ms=60.0):
    scratch = make_generated_dam_break_engine(DP, setup_dam_break_3d(DP), device_float_bytes=4)
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < ms:
        scratch.advance(1e9, max_steps=16)
    scratch.close()


def probe_points(n):
    """n points inside the reservoir of the lattice (0 … 0.38 × 0 … 0.62 × 0 … 0.28 m of water)."""
    rng = np.random.default_rng(1)
    return rng.uniform([0.01, 0.01, 0.01], [0.37, 0.61, 0.27], (n, 3))


def window(n_probes, warmup, steps):
    eng = make_generated_dam_break_engine(DP, setup_dam_break_3d(DP), device_float_bytes=4)
    if n_probes:
        eng.probes_enable(probe_points(n_probes), capacity=warmup + steps)
    precondition()
    eng.advance(1e9, max_steps=warmup)
    t0 = time.perf_counter()
    pr = eng.advance(1e9, max_steps=steps)
    dt = time.perf_counter() - t0
    if n_probes:
        r = eng.probes_read()
        assert len(r["iteration"]) == warmup + steps and (r["count"][-1] > 0).all()
    assert pr.steps_done == steps
    N = eng.N
    eng.close()
    return dt / steps * 1e6, N


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--counts", default="0,8,512,1024")
    args = ap.parse_args()
    counts = [int(c) for c in args.counts.split(",")]
    us = {c: [] for c in counts}
    for r in range(args.reps):
        for c in counts:
            t, N = window(c, args.warmup, args.steps)
            us[c].append(t)
            print(f"rep {r} probes {c:5d}: N={N} {t:.2f} us/step {N / t * 1e6:.4g} updates/s", flush=True)
    off = np.array(us[counts[0]])
    for c in counts:
        a = np.array(us[c])
        print(f"[dam break 3-D, 1.06 M particles, fp32] probes {c:5d}: {np.median(a):.2f} us/step (min {a.min():.2f}, max {a.max():.2f})  "
              f"against {counts[0]} probes {np.median(a) - np.median(off):+.2f} us/step ({100 * (np.median(a) / np.median(off) - 1):+.2f} %; "
              f"spread of those runs {100 * (off.max() - off.min()) / np.median(off):.2f} %)", flush=True)


if __name__ == "__main__":
    main()
