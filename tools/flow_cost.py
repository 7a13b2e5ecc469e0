#!/usr/bin/env python3
"""What the per-step flow through control boxes costs (sphmi_flow_enable): the bench's 1 M-particle window (BASELINE config 3,
1 057 738 rows, fp32) with the flow disabled, with one box and with sixteen boxes, three repetitions interleaved on one GPU — the
procedure of tools/budgets_cost.py.  Prints one line per run and a summary per configuration: ms per step, the difference to the
disabled runs, the spread of the disabled runs.

    python tools/flow_cost.py [--steps 60] [--warmup 5] [--reps 3] [--lib PATH]
    rocprofv3 --kernel-trace --stats -d OUT -o flow -f csv -- python tools/flow_cost.py --trace 1m|2d

--trace runs one short window for a kernel trace instead of the timing: `1m` = the large case with 16 boxes AND the budgets (the
yardstick's kernels in the same trace), 20 steps; `2d` = the 2-D dam break (6 881 rows, fp32, the perturbed state of the tests)
with 16 strips, 20 steps with two stages forced (SPHMI_FLOW_SMALL_ROWS=0) and 20 steps with one launch forced (=8192).

--lib (or $SPHMI_LIB before the start) runs another build of the library, e.g. the parent commit's for the disabled figure; such a
library is only asked for the disabled configuration when it does not export sphmi_flow_enable."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import time  # noqa: E402

import numpy as np  # noqa: E402


def boxes(n, extent=1.6):
    """n boxes: one gate [extent / 2, +inf) along x, or a tiling of sixteen strips along x over the tank"""
    from sphexample_amd import flow
    if n == 1:
        lo, hi = np.full((1, 3), -np.inf), np.full((1, 3), np.inf)
        lo[0, 0] = 0.5 * extent
        return lo, hi
    return flow.strips(0, np.linspace(0.0, extent, n + 1)[1:-1], 3)


def window(n_boxes, warmup, steps):
    from group_forces_cost import DP, precondition
    from sphexample_amd.cases import setup_dam_break_3d
    from sphexample_amd.engine import make_generated_dam_break_engine
    eng = make_generated_dam_break_engine(DP, setup_dam_break_3d(DP), device_float_bytes=4)
    if n_boxes:
        eng.flow_enable(*boxes(n_boxes), capacity=warmup + steps)
    precondition()
    eng.advance(1e9, max_steps=warmup)
    t0 = time.perf_counter()
    pr = eng.advance(1e9, max_steps=steps)
    dt = time.perf_counter() - t0
    if n_boxes:
        f = eng.flow_read()
        assert len(f["iteration"]) == warmup + steps and f["count"].shape[1] == n_boxes
        if n_boxes > 1:
            assert (f["count"].sum(1) == f["count"][0].sum()).all() and f["count"][0].sum() > 0      # a tiling holds every Fluid row once
    assert pr.steps_done == steps
    N = eng.N
    eng.close()
    return dt / steps * 1e3, N


def trace(which, steps=20):
    from sphexample_amd import flow
    if which == "1m":
        from group_forces_cost import DP
        from sphexample_amd.cases import setup_dam_break_3d
        from sphexample_amd.engine import make_generated_dam_break_engine
        eng = make_generated_dam_break_engine(DP, setup_dam_break_3d(DP), device_float_bytes=4)
        eng.flow_enable(*boxes(16), capacity=steps)
        eng.budgets_enable(capacity=steps)
        eng.advance(1e9, max_steps=steps)
        f = eng.flow_read()
        print(f"1m: N={eng.N} {len(f['iteration'])} samples, count {f['count'][-1].tolist()}, entered {f['entered'].sum(0).tolist()}")
        eng.close()
        return
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import load_dam_break_2d, perturbed
    from sphexample_amd.engine import make_engine
    p0, s = load_dam_break_2d()
    for rows in ("0", "8192"):
        os.environ["SPHMI_FLOW_SMALL_ROWS"] = rows          # read at enable
        eng = make_engine(perturbed(p0, seed=3, vel_scale=3.0), s, device_float_bytes=4)
        eng.flow_enable(*flow.strips(0, [0.1 * k for k in range(1, 16)], 2), capacity=steps)
        eng.advance(1e9, max_steps=steps)
        print(f"2d, SPHMI_FLOW_SMALL_ROWS={rows}: N={eng.N} count {eng.flow_read()['count'][-1].tolist()}")
        eng.close()
    os.environ.pop("SPHMI_FLOW_SMALL_ROWS", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lib")
    ap.add_argument("--trace", choices=("1m", "2d"))
    args = ap.parse_args()
    if args.lib:
        os.environ["SPHMI_LIB"] = os.path.abspath(args.lib)
    if args.trace:
        return trace(args.trace)
    from sphexample_amd.engine import load_library
    configs = [0, 1, 16] if hasattr(load_library(), "sphmi_flow_enable") else [0]
    ms = {n: [] for n in configs}
    for r in range(args.reps):
        for n in configs:
            t, N = window(n, args.warmup, args.steps)
            ms[n].append(t)
            print(f"rep {r} flow {'disabled' if n == 0 else f'{n:2d} boxes'}: N={N} {t:.4f} ms/step {N / t * 1e3:.4g} updates/s", flush=True)
    off = np.median(ms[0])
    print(f"disabled: median {off:.4f} ms/step (min {min(ms[0]):.4f}, max {max(ms[0]):.4f}, spread {(max(ms[0]) - min(ms[0])) / off * 100:.2f} %)")
    for n in configs[1:]:
        on = np.median(ms[n])
        print(f"{n:2d} boxes: median {on:.4f} ms/step (min {min(ms[n]):.4f}, max {max(ms[n]):.4f}); "
              f"cost {1e3 * (on - off):+.1f} us/step ({(on - off) / off * 100:+.2f} %)")


if __name__ == "__main__":
    main()
