#!/usr/bin/env python3
"""What labelling the connected bodies costs (sphmi_components_build / sphmi_components_read): the bench's 1 M-particle dam break
(C3) at rest — a few steps in — and in developed flow, in one process on one device.

    python tools/components_cost.py [--steps 20] [--developed 0.4] [--reps 5] [--link-dx 0]

Per state it prints C, the size of the main body and the medians over --reps builds (after one untimed build, which allocates the
arena) of the device time of the five passes — init, hook, flatten, number, table — which the library itself reports from events on
its stream ($SPHMI_COMPONENTS_TIMING, set here), the host's clock around build and read, and the yardstick: k_neighbor_count, the
same walk without the hooking, timed the same way in the same run ($SPHMI_NEIGHBORS_TIMING, a HALF list like the hook's walk, and
the FULL list profiles/neighbor_list.md timed).  The last line of a state is the ratio hook / count.
--link-dx F links within F * dx instead of H.  The case is bench.py's: the lattice at dp = 0.00425 generated on the device, fp32."""
import argparse
import os
import re
import sys
import tempfile
import time

os.environ.setdefault("SPHMI_COMPONENTS_TIMING", "1")
os.environ.setdefault("SPHMI_NEIGHBORS_TIMING", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from sphexample_amd.cases import setup_dam_break_3d  # noqa: E402
from sphexample_amd.engine import make_generated_dam_break_engine  # noqa: E402

DP = 0.00425


class Stderr:
    """What the library writes to file descriptor 2 while the block runs."""
    def __enter__(self):
        sys.stderr.flush()
        self.keep, self.tmp = os.dup(2), tempfile.TemporaryFile()
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.keep, 2); os.close(self.keep)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


def passes(text, names):
    rows = [[float(re.search(rf"{n} ([0-9.]+) ms", ln).group(1)) for n in names] for ln in text.splitlines() if all(f"{n} " in ln for n in names)]
    return np.array(rows)


def measure(eng, what, reps, link):
    host = []
    with Stderr() as err:
        eng.components_build(link)                                                  # allocates the arena
        for _ in range(reps):
            t0 = time.perf_counter(); rows, comps = eng.components_build(link); host.append((time.perf_counter() - t0) * 1e3)
    names = ("init", "hook", "flatten", "number", "table")
    ms = np.median(passes(err.text, names)[1:], axis=0)
    t0 = time.perf_counter(); lab, first, cnt, box = eng.components_read(); read = (time.perf_counter() - t0) * 1e3
    print(f"[{what}] sphmi_components_build: {rows} rows, link {link:.6g}, C = {comps}, main body {int(cnt.max())} rows "
          f"({100.0 * cnt.max() / max(int((lab >= 0).sum()), 1):.2f} % of the selected), singletons {int((cnt == 1).sum())}", flush=True)
    print(f"[{what}] passes (median of {reps}): " + ", ".join(f"{n} {v:.3f} ms" for n, v in zip(names, ms)) +
          f"; build by the host's clock {np.median(host):.2f} ms; read {read:.2f} ms for {(lab.nbytes + first.nbytes + cnt.nbytes + box.nbytes) / 1e6:.2f} MB", flush=True)
    eng.components_release()
    count = {}
    for half in (True, False):
        with Stderr() as err:
            for _ in range(reps + 1):
                eng.neighbors_build(half)
        count[half] = float(np.median(passes(err.text, ("count", "scan", "fill"))[1:, 0]))
        eng.neighbors_release()
    print(f"[{what}] yardstick k_neighbor_count (median of {reps}): half list {count[True]:.3f} ms, full list {count[False]:.3f} ms", flush=True)
    print(f"[{what}] hook / count = {ms[1] / count[True]:.3f} (half), {ms[1] / count[False]:.3f} (full)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--developed", type=float, default=0.4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--link-dx", type=float, default=0.0)
    args = ap.parse_args()
    eng = make_generated_dam_break_engine(DP, setup_dam_break_3d(DP), device_float_bytes=4)
    link = args.link_dx * DP if args.link_dx > 0 else eng.cfg.H
    pr = eng.advance(1e9, max_steps=args.steps)
    measure(eng, f"at rest, N={eng.N}, fp32, step {pr.iteration}", args.reps, link)
    if args.developed > 0:
        t0 = time.perf_counter()
        pr = eng.advance(args.developed)
        print(f"advanced to t = {pr.total_time:.4f} s (step {pr.iteration}) in {time.perf_counter() - t0:.1f} s", flush=True)
        measure(eng, f"developed, t={pr.total_time:.3f} s, step {pr.iteration}", args.reps, link)
    eng.close()


if __name__ == "__main__":
    main()
