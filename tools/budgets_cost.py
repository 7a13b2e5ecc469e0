#!/usr/bin/env python3
"""What the per-step budgets of the fluid cost (sphmi_budgets_enable): the bench's 1 M-particle window and the 2-D dam break, each
with sampling off and on, three repetitions interleaved on one GPU — the procedure of tools/group_forces_cost.py.  The 2-D case runs
the sampled window with the library's threshold between the one-launch and the two-stage path, with two stages forced and with one
launch forced (SPHMI_BUDGETS_SMALL_ROWS), so that the threshold rests on a measurement.  Prints one line per run and a summary per
case: µs per step off / on, the difference per step, the spread of the off runs.

    python tools/budgets_cost.py [--steps 60] [--warmup 5] [--steps-2d 2000] [--reps 3]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import time  # noqa: E402

import numpy as np  # noqa: E402
from group_forces_cost import DP, precondition, summary  # noqa: E402
from sphexample_amd import Fixed, Fluid, Geometry  # noqa: E402
from sphexample_amd.cases import setup_dam_break_2d, setup_dam_break_3d  # noqa: E402
from sphexample_amd.engine import make_engine, make_generated_dam_break_engine  # noqa: E402
from sphexample_amd.preprocess import AllocateDataStructures  # noqa: E402


def enable(eng, capacity, small_rows=None):
    """$SPHMI_BUDGETS_SMALL_ROWS is read at enable."""
    os.environ.pop("SPHMI_BUDGETS_SMALL_ROWS", None)
    if small_rows is not None:
        os.environ["SPHMI_BUDGETS_SMALL_ROWS"] = str(small_rows)
    eng.budgets_enable(capacity=capacity)
    os.environ.pop("SPHMI_BUDGETS_SMALL_ROWS", None)


def window_1m(sampled, warmup, steps):
    eng = make_generated_dam_break_engine(DP, setup_dam_break_3d(DP), device_float_bytes=4)
    if sampled:
        enable(eng, warmup + steps)
    precondition()
    eng.advance(1e9, max_steps=warmup)
    t0 = time.perf_counter()
    pr = eng.advance(1e9, max_steps=steps)
    dt = time.perf_counter() - t0
    n = len(eng.budgets_read()["iteration"]) if sampled else 0
    assert pr.steps_done == steps and n == (warmup + steps if sampled else 0)
    N = eng.N
    eng.close()
    return dt / steps * 1e6, N


def window_2d(p, s, mode, steps):
    """mode: None = off, "default" = the library's threshold, an integer = that SPHMI_BUDGETS_SMALL_ROWS."""
    eng = make_engine(p, s, device_float_bytes=4)
    if mode is not None:
        enable(eng, steps + 50, None if mode == "default" else mode)
    eng.advance(1e9, max_steps=50)
    t0 = time.perf_counter()
    pr = eng.advance(1e9, max_steps=steps)
    dt = time.perf_counter() - t0
    assert pr.steps_done == steps and (mode is None or len(eng.budgets_read()["iteration"]) == steps + 50)
    eng.close()
    return dt / steps * 1e6, len(p)


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
            print(f"1M rep {r} budgets {'on ' if sampled else 'off'}: N={N} {us:.2f} us/step {N / us * 1e6:.4g} updates/s", flush=True)
    summary("dam break 3-D, 1.06 M particles, fp32, two stages", off, on)
    inp = os.path.join(ROOT, "tests", "golden", "input")
    p = AllocateDataStructures([Geometry(os.path.join(inp, "DamBreak2d_Dp0.02_Bound.csv"), 1, Fixed, None, 2, "Float64"),
                                Geometry(os.path.join(inp, "DamBreak2d_Dp0.02_Fluid.csv"), 2, Fluid, None, 2, "Float64")])
    s = setup_dam_break_2d()
    modes = {None: "off", "default": "default threshold", 0: "two stages", 8192: "one launch"}
    us = {m: [] for m in modes}
    for r in range(args.reps):
        for m, label in modes.items():
            t, N = window_2d(p, s, m, args.steps_2d)
            us[m].append(t)
            print(f"2-D rep {r} budgets {label}: N={N} {t:.2f} us/step", flush=True)
    for m, label in modes.items():
        if m is not None:
            summary(f"dam break 2-D, 6 881 particles, fp32, {label}", us[None], us[m])


if __name__ == "__main__":
    main()
