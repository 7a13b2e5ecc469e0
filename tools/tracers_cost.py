#!/usr/bin/env python3
"""What the tracers cost (sphmi_tracers_enable): the bench's 1 M-particle case (BASELINE config 3, 1 057 738 rows, fp32) with another
build of the library (--lib: the parent commit's), with this tree disabled, with 256 tracked particles, with 256 drifters, with both,
and — the yardstick of the drifter pass, which runs the probes' walk — with 256 fixed probes (sphmi_probes_enable) at the points the
drifters are released at.  Repetitions interleaved on one GPU, the procedure of tools/envelopes_cost.py.  Every handle is measured twice:
AT REST (`--steps` steps behind `--warmup` from the lattice; rows and points drawn from the Fluid rows of the lattice) and on DEVELOPED
FLOW (the handle advanced to t = `--developed` s with its observer running, then the observer enabled AGAIN on rows and points drawn
from the Fluid rows of the state there, the same ones for every variant — the runs are bit-identical — and `--developed-steps` steps
timed; the rows' map still dates from the upload, so by then its order is random with respect to the row order).

    python tools/tracers_cost.py [--steps 60] [--warmup 5] [--reps 3] [--lib PATH] [--developed 0.4] [--developed-steps 200] [--out DIR]

Prints one line per window and a summary per variant — median ms per step, min, max, the difference to the disabled runs — and, with
--out, writes the raw lines to DIR/tracers_raw.txt and the summary table to DIR/tracers_table.md.  The other library runs in a child
process of its own per repetition (a process loads one libsphmi.so)."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

VARIANTS = ("disabled", "256 particles", "256 drifters", "both", "256 probes")
COUNT = 256


def enable(eng, variant, seed, capacity):
    """Rows and points of the Fluid rows the handle holds now: the same draw for every variant."""
    if variant == "disabled":
        return
    d = eng.download(("Position", "Type"))
    fluid = np.flatnonzero(d["Type"] == 1)
    rng = np.random.default_rng(seed)
    rows = np.sort(rng.choice(fluid, COUNT, replace=False))
    points = d["Position"][rng.choice(fluid, COUNT, replace=False)].astype(np.float64) + rng.uniform(-0.002, 0.002, (COUNT, 3))
    if variant == "256 probes":
        eng.probes_enable(points, capacity=capacity)
    else:
        eng.tracers_enable(particles=rows if variant != "256 drifters" else None, drifters=points if variant != "256 particles" else None, capacity=capacity)


def windows(variant, args):
    """(ms per step at rest, ms per step on developed flow, rows, rebuilds in the developed window, wet drifters / probes at the end)"""
    from group_forces_cost import DP, precondition
    from sphexample_amd.cases import setup_dam_break_3d
    from sphexample_amd.engine import make_generated_dam_break_engine
    eng = make_generated_dam_break_engine(DP, setup_dam_break_3d(DP), device_float_bytes=4)
    enable(eng, variant, 1, 4096)
    precondition()
    eng.advance(1e9, max_steps=args.warmup)
    t0 = time.perf_counter()
    pr = eng.advance(1e9, max_steps=args.steps)
    rest = (time.perf_counter() - t0) / args.steps * 1e3
    assert pr.steps_done == args.steps
    developed, rebuilds, wet = float("nan"), 0, -1
    if args.developed > 0:
        r0 = eng.advance(args.developed).n_rebuilds
        enable(eng, variant, 2, args.developed_steps)
        t0 = time.perf_counter()
        pr = eng.advance(1e9, max_steps=args.developed_steps)
        developed = (time.perf_counter() - t0) / args.developed_steps * 1e3
        assert pr.steps_done == args.developed_steps
        rebuilds = int(pr.n_rebuilds - r0)
    if variant == "256 probes":
        r = eng.probes_read()
        assert len(r["iteration"]) == min(pr.iteration, args.developed_steps if args.developed > 0 else 4096)
        wet = int((r["weight"][-1] >= 0.5).sum())
    elif variant != "disabled":
        r = eng.tracers_read()
        assert int(r["iteration"][-1]) == pr.iteration and r["particles"]["values"].shape[1] + r["drifters"]["position"].shape[1] in (COUNT, 2 * COUNT)
        if variant != "256 particles":
            wet = int((r["drifters"]["weight"][-1] >= 0.5).sum())
            assert np.isfinite(r["drifter_position"]).all()
    N = eng.N
    eng.close()
    return rest, developed, N, rebuilds, wet


def other_library(args):
    """the same two windows with --lib, disabled, in a child process"""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--lib", args.lib, "--steps", str(args.steps), "--warmup", str(args.warmup),
           "--developed", str(args.developed), "--developed-steps", str(args.developed_steps)]
    out = subprocess.run(cmd, capture_output=True, text=True, check=True).stdout
    rest, developed, N, rebuilds, wet = [ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1].split()[1:]
    return float(rest), float(developed), int(N), int(rebuilds), int(wet)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--developed", type=float, default=0.4)
    ap.add_argument("--developed-steps", type=int, default=200)
    ap.add_argument("--lib")
    ap.add_argument("--out")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        os.environ["SPHMI_LIB"] = os.path.abspath(args.lib)
        print("RESULT %.6f %.6f %d %d %d" % windows("disabled", args), flush=True)
        return
    names = (["parent"] if args.lib else []) + list(VARIANTS)
    ms = {n: {"rest": [], "developed": []} for n in names}
    raw = []

    def say(line):
        raw.append(line)
        print(line, flush=True)

    for r in range(args.reps):
        for n in names:
            rest, developed, N, rebuilds, wet = other_library(args) if n == "parent" else windows(n, args)
            ms[n]["rest"].append(rest); ms[n]["developed"].append(developed)
            say(f"rep {r} {n:13s}: N={N} at rest {rest:.4f} ms/step {N / rest * 1e3:.4g} updates/s | developed (t = {args.developed} s, "
                f"{rebuilds} rebuilds in {args.developed_steps} steps) {developed:.4f} ms/step" + (f" | S >= 0.5 at the last step: {wet} of {COUNT}" if wet >= 0 else ""))
    table = ["| variant | at rest: median ms/step (min – max, spread) | against disabled | developed: median ms/step (min – max, spread) | against disabled |",
             "|---|---|---|---|---|"]
    for n in names:
        cells = []
        for w in ("rest", "developed"):
            v, off = ms[n][w], np.median(ms["disabled"][w])
            med = np.median(v)
            cells += [f"{med:.4f} ({min(v):.4f} – {max(v):.4f}, {(max(v) - min(v)) / med * 100:.2f} %)",
                      "—" if n == "disabled" else f"{1e3 * (med - off):+.1f} µs ({(med - off) / off * 100:+.2f} %)"]
        table.append(f"| {n} | " + " | ".join(cells) + " |")
    for line in table:
        say(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "tracers_raw.txt"), "w") as f:
            f.write("command: python tools/tracers_cost.py " + " ".join(a if a != args.lib else "PARENT_LIB" for a in sys.argv[1:]) + "\n" + "\n".join(raw) + "\n")
        with open(os.path.join(args.out, "tracers_table.md"), "w") as f:
            f.write("\n".join(table) + "\n")


if __name__ == "__main__":
    main()
