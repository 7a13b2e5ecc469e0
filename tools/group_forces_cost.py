#!/usr/bin/env python3
"""What the per-step group forces cost (sphmi_group_forces_enable): the bench's 1 M-particle window and the 2-D dam break, each with
sampling off and on, three repetitions interleaved on one GPU.  Prints one line per run and a summary per case:
µs per step off / on, the difference per step, the spread of the off runs.

    python tools/group_forces_cost.py [--steps 60] [--warmup 5] [--steps-2d 2000] [--reps 3]

The large case is bench.py's: the dam-break lattice at dp = 0.00425 generated on the device, fp32 kernels, 60 ms of untimed
pre-conditioning on a scratch handle before every window, W warm-up steps, K timed steps; sampled: the boundary group (marker 1).
The small case is tools/latency_2d.py's: DamBreak2d Dp 0.02, fp32, both groups sampled."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from sphexample_amd import Fixed, Fluid, Geometry  # noqa: E402
from sphexample_amd.cases import setup_dam_break_2d, setup_dam_break_3d  # noqa: E402
from sphexample_amd.engine import make_engine, make_generated_dam_break_engine  # noqa: E402
from sphexample_amd.preprocess import AllocateDataStructures  # noqa: E402

DP = 0.00425


def precondition(ms=60.0):
    scratch = make_generated_dam_break_engine(DP, setup_dam_break_3d(DP), device_float_bytes=4)
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < ms:
        scratch.advance(1e9, max_steps=16)
    scratch.close()


def window_1m(sampled, warmup, steps):
    eng = make_generated_dam_break_engine(DP, setup_dam_break_3d(DP), device_float_bytes=4)
    if sampled:
        eng.group_forces_enable([1], capacity=warmup + steps)
    precondition()
    eng.advance(1e9, max_steps=warmup)
    t0 = time.perf_counter()
    pr = eng.advance(1e9, max_steps=steps)
    dt = time.perf_counter() - t0
    n = len(eng.group_forces_read()[0]) if sampled else 0
    assert pr.steps_done == steps and n == (warmup + steps if sampled else 0)
    N = eng.N
    eng.close()
    return dt / steps * 1e6, N


def window_2d(p, s, sampled, steps):
    eng = make_engine(p, s, device_float_bytes=4)
    if sampled:
        eng.group_forces_enable([1, 2], capacity=steps + 50)
    eng.advance(1e9, max_steps=50)
    t0 = time.perf_counter()
    pr = eng.advance(1e9, max_steps=steps)
    dt = time.perf_counter() - t0
    assert pr.steps_done == steps
    eng.close()
    return dt / steps * 1e6, len(p)


def summary(name, off, on):
    off, on = np.array(off), np.array(on)
    print(f"[{name}] off {np.median(off):.2f} us/step (min {off.min():.2f}, max {off.max():.2f}, spread {100 * (off.max() - off.min()) / np.median(off):.2f} %)  "
          f"on {np.median(on):.2f} us/step (min {on.min():.2f}, max {on.max():.2f})  cost {np.median(on) - np.median(off):+.2f} us/step "
          f"({100 * (np.median(on) / np.median(off) - 1):+.2f} %)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps-2d", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    off, on = [], []
    for r in range(args.reps):
        for sampled in (False, True):
            us, N = window_1m(sampled, args.warmup, args.steps)
            (on if sampled else off).append(us)
            print(f"1M rep {r} sampling {'on ' if sampled else 'off'}: N={N} {us:.2f} us/step {N / us * 1e6:.4g} updates/s", flush=True)
    summary("dam break 3-D, 1.06 M particles, fp32, boundary group", off, on)
    inp = os.path.join(ROOT, "tests", "golden", "input")
    p = AllocateDataStructures([Geometry(os.path.join(inp, "DamBreak2d_Dp0.02_Bound.csv"), 1, Fixed, None, 2, "Float64"),
                                Geometry(os.path.join(inp, "DamBreak2d_Dp0.02_Fluid.csv"), 2, Fluid, None, 2, "Float64")])
    s = setup_dam_break_2d()
    off, on = [], []
    for r in range(args.reps):
        for sampled in (False, True):
            us, N = window_2d(p, s, sampled, args.steps_2d)
            (on if sampled else off).append(us)
            print(f"2-D rep {r} sampling {'on ' if sampled else 'off'}: N={N} {us:.2f} us/step", flush=True)
    summary("dam break 2-D, 6 881 particles, fp32, both groups", off, on)


if __name__ == "__main__":
    main()
