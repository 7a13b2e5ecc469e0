#!/usr/bin/env python3
"""What a selected download costs against a full one (sphmi_select_* against sphmi_download + a numpy mask): the bench's
1 M-particle case (C3), at rest and in developed flow.

    python tools/bench_select.py [--reps 7] [--rest-steps 20] [--developed 0.4]

For each state and each selection — the Fluid rows, a slab one cell (H) thick through the pillar, every 8th particle by ID, the
free-surface mask of sphmi_particle_fields, and everything with all clauses off (the overhead case) — medians over --reps
alternating repetitions after one untimed repetition of each:
  A  ms of Backend.select(spec): build (flag, scan, fill), read of the rows, download of all ten fields, release — by the host's
     clock; every call ends in a synchronisation of the stream
  B  ms of Backend.download() of the same ten fields into pageable numpy arrays plus the numpy mask and the ten gathers on the host
     (the mask's share is printed on its own)
Then one more call of A with $SPHMI_SELECT_TIMES set: the library writes the device time of the flag, scan and fill passes and of
the pack and copy of the download to stderr, from events on its stream.
The case is bench.py's: the dam-break lattice at dp = 0.00425 generated on the device, fp32 kernels, Float64 host arrays."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from sphexample_amd import selection  # noqa: E402
from sphexample_amd.cases import setup_dam_break_3d  # noqa: E402
from sphexample_amd.engine import make_generated_dam_break_engine  # noqa: E402
from sphexample_amd.fields import free_surface_mask  # noqa: E402

DP = 0.00425


def stats(t):
    return f"{np.median(t):.2f} ms (min {np.min(t):.2f}, max {np.max(t):.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rest-steps", type=int, default=20)
    ap.add_argument("--developed", type=float, default=0.4)
    args = ap.parse_args()
    os.environ.pop("SPHMI_SELECT_TIMES", None)
    eng = make_generated_dam_break_engine(DP, setup_dam_break_3d(DP), device_float_bytes=4)
    H = eng.cfg.H
    for state in ("at rest", "developed"):
        if state == "at rest":
            pr = eng.advance(1e9, max_steps=args.rest_steps)
        else:
            pr = eng.advance(args.developed)
        where = f"[dam break 3-D, N={eng.N}, fp32, {state}: t = {pr.total_time:.4f} s, iteration {pr.iteration}]"
        surface = free_surface_mask(eng.particle_fields(("div_r",))["div_r"], 3)
        specs = {
            "fluid": selection.Selection(types=("Fluid",)),
            "slab H through the pillar": selection.slab(0, 0.96, H, dims=3),
            "every(8)": selection.every(8),
            "free-surface mask": selection.where(surface),
            "everything": selection.Selection(),
        }
        for name, spec in specs.items():
            def a():
                t0 = time.perf_counter()
                rows, got = eng.select(spec)
                return (time.perf_counter() - t0) * 1e3, rows, got

            def b():
                t0 = time.perf_counter()
                d = eng.download()
                t1 = time.perf_counter()
                rows = np.flatnonzero(selection.keep_mask(spec, d))
                got = {k: v[rows] for k, v in d.items()}
                t2 = time.perf_counter()
                return (t2 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3, rows, got
            _, rows_a, got_a = a()
            _, _, _, rows_b, got_b = b()
            same = bool(np.array_equal(rows_a, rows_b) and all(got_a[k].tobytes() == got_b[k].tobytes() for k in got_a))
            ta, tb, tdl, tmask = [], [], [], []
            for _ in range(args.reps):                                              # alternating: the host is shared
                ta.append(a()[0])
                r = b()
                tb.append(r[0]); tdl.append(r[1]); tmask.append(r[2])
            kept = len(rows_a)
            bytes_a = sum(v.nbytes for v in got_a.values()) + rows_a.nbytes
            bytes_b = sum(v.nbytes for v in eng.download().values())
            print(f"{where} {name}: kept {kept} of {eng.N} ({100.0 * kept / eng.N:.1f} %), same bytes as the host mask: {same} | "
                  f"A select {stats(ta)}, {bytes_a / 1e6:.1f} MB over the bus | B download + mask {stats(tb)} = download {stats(tdl)} + mask and gathers "
                  f"{stats(tmask)}, {bytes_b / 1e6:.1f} MB over the bus | A / B = {np.median(ta) / np.median(tb):.3f}", flush=True)
            os.environ["SPHMI_SELECT_TIMES"] = "1"                                  # the device time of every pass of one more call → stderr
            sys.stderr.write(f"{where} {name}: passes of one call\n"); sys.stderr.flush()
            a()
            os.environ.pop("SPHMI_SELECT_TIMES", None)
    eng.close()


if __name__ == "__main__":
    main()
