#!/usr/bin/env python3
"""What the per-bin maps cost (sphmi_maps_enable): the bench's 1 M-particle case (BASELINE config 3, 1 057 738 rows, fp32) with another
build of the library (--lib: the parent commit's), with this tree disabled, with a floor map of spacing 2·dp over the tank and with a
full 3-D lattice just below SPHMI_MAX_MAP_BINS — repetitions interleaved on one GPU, the procedure of tools/envelopes_cost.py.  Every
handle is measured twice: AT REST (`--steps` steps behind `--warmup` from the lattice) and on DEVELOPED FLOW (the handle advanced to
t = `--developed` s: `--developed-steps` steps there, the fluid spread over the floor).

    python tools/maps_cost.py [--steps 60] [--warmup 5] [--reps 3] [--lib PATH] [--developed 0.4] [--developed-steps 200] [--out DIR]

Prints one line per window and a summary per variant — median ms per step, min, max, the difference to the disabled runs — and, with
--out, writes the raw lines to DIR/maps_raw.txt and the summary table to DIR/maps_table.md.  The other library runs in a child process
of its own per repetition (a process loads one libsphmi.so)."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

MAX_BINS = 1 << 20


def floor_map(lo, hi, dp):
    """columns of 2·dp × 2·dp over the whole tank, the vertical collapsed"""
    s = 2.0 * dp
    return (lo[0], lo[1], 0.0), (s, s, np.inf), (int(np.ceil((hi[0] - lo[0]) / s)), int(np.ceil((hi[1] - lo[1]) / s)), 1), 2


def full_lattice(lo, hi, dp):
    """cubic bins over the whole tank, as fine as SPHMI_MAX_MAP_BINS allows"""
    s = (np.prod(hi - lo) / MAX_BINS) ** (1.0 / 3.0)
    while True:
        counts = tuple(int(np.ceil((hi[d] - lo[d]) / s)) for d in range(3))
        if counts[0] * counts[1] * counts[2] <= MAX_BINS:
            return tuple(lo), (s, s, s), counts, 2
        s *= 1.002


VARIANTS = {"disabled": None, "floor map": floor_map, "full lattice": full_lattice}


def windows(make, args):
    """(ms per step at rest, ms per step on developed flow, rows, bins, wet bins and fluid rows outside the lattice at the end) of one fresh handle"""
    from group_forces_cost import DP, precondition
    from sphexample_amd.cases import setup_dam_break_3d
    from sphexample_amd.engine import make_generated_dam_break_engine
    eng = make_generated_dam_break_engine(DP, setup_dam_break_3d(DP), device_float_bytes=4)
    bins = 0
    if make:
        x = eng.download(("Position",))["Position"]
        lattice = make(x.min(axis=0) - 0.5 * DP, x.max(axis=0) + 0.5 * DP, DP)
        eng.maps_enable(*lattice)
        bins = int(np.prod(lattice[2]))
    precondition()
    eng.advance(1e9, max_steps=args.warmup)
    t0 = time.perf_counter()
    pr = eng.advance(1e9, max_steps=args.steps)
    rest = (time.perf_counter() - t0) / args.steps * 1e3
    assert pr.steps_done == args.steps
    developed = float("nan")
    if args.developed > 0:
        eng.advance(args.developed)
        t0 = time.perf_counter()
        pr = eng.advance(1e9, max_steps=args.developed_steps)
        developed = (time.perf_counter() - t0) / args.developed_steps * 1e3
        assert pr.steps_done == args.developed_steps
    wet = outside = 0
    if make:
        r = eng.maps_read()
        fluid = int((eng.download(("Type",))["Type"] == 1).sum())
        assert r["steps"] == pr.iteration and 0 < int(r["last_n"].sum()) <= fluid and (r["n_max"] >= r["last_n"]).all()
        outside = fluid - int(r["last_n"].sum())           # (rows that left the tank)
        wet = int((r["t_arrival"] < np.inf).sum())
    N = eng.N
    eng.close()
    return rest, developed, N, bins, wet, outside


def other_library(args):
    """the same two windows with --lib, disabled, in a child process"""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--lib", args.lib, "--steps", str(args.steps), "--warmup", str(args.warmup),
           "--developed", str(args.developed), "--developed-steps", str(args.developed_steps)]
    out = subprocess.run(cmd, capture_output=True, text=True, check=True).stdout
    rest, developed, N, bins, wet, outside = [ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1].split()[1:]
    return float(rest), float(developed), int(N), int(bins), int(wet), int(outside)


def main(variants=VARIANTS):
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
        print("RESULT %.6f %.6f %d %d %d %d" % windows(None, args), flush=True)
        return
    names = (["parent"] if args.lib else []) + list(variants)
    ms = {n: {"rest": [], "developed": []} for n in names}
    raw = []

    def say(line):
        raw.append(line)
        print(line, flush=True)

    for r in range(args.reps):
        for n in names:
            rest, developed, N, bins, wet, outside = other_library(args) if n == "parent" else windows(variants[n], args)
            ms[n]["rest"].append(rest); ms[n]["developed"].append(developed)
            say(f"rep {r} {n:12s}: N={N} bins={bins} (wet at the end: {wet}, fluid rows outside: {outside}) at rest {rest:.4f} ms/step {N / rest * 1e3:.4g} updates/s | "
                f"developed (t = {args.developed} s, {args.developed_steps} steps) {developed:.4f} ms/step")
    table = ["| variant | at rest: median ms/step (min – max, spread) | against disabled | developed: median ms/step (min – max, spread) | against disabled |",
             "|---|---|---|---|---|"]
    cells = {}
    for n in names:
        for w in ("rest", "developed"):
            v, off = ms[n][w], np.median(ms["disabled"][w])
            med = np.median(v)
            cells[n, w] = (f"{med:.4f} ({min(v):.4f} – {max(v):.4f}, {(max(v) - min(v)) / med * 100:.2f} %)",
                           "—" if n == "disabled" else f"{1e3 * (med - off):+.1f} µs ({(med - off) / off * 100:+.2f} %)")
        table.append(f"| {n} | {cells[n, 'rest'][0]} | {cells[n, 'rest'][1]} | {cells[n, 'developed'][0]} | {cells[n, 'developed'][1]} |")
    for line in table:
        say(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "maps_raw.txt"), "w") as f:
            f.write("command: python tools/maps_cost.py " + " ".join(a if a != args.lib else "PARENT_LIB" for a in sys.argv[1:]) + "\n" + "\n".join(raw) + "\n")
        with open(os.path.join(args.out, "maps_table.md"), "w") as f:
            f.write("\n".join(table) + "\n")


if __name__ == "__main__":
    main()
