#!/usr/bin/env python3
"""What a ray search costs (sphmi_cast_rays) next to what the library offered for the same answer before it: sphmi_sample_points
over EVERY march point of every ray plus the search on the host.  The bench's 1 M-particle case (C3), a few steps in ("at rest")
and, with --time, at that simulated time ("developed flow").

    python tools/rays_cost.py [--steps 20] [--time 0.4] [--reps 5]

Two sets of rays, both vertical, from above the tank to its floor, step h / 2:
  gauges   64 rays along the tank's centre line
  image    256 × 256 rays over the tank's footprint
Per set, medians over --reps calls after one untimed call (which allocates): `call` ms of Backend.cast_rays with every output; on
stderr the library's own line with SPHMI_RAYS_CLOCK set — the device time of upload / cast / fetch; evaluations per ray (march
lanes up to and including the round of the crossing and 63 per refinement round; the one re-evaluation of a march end that stays
the record is not counted) and
evaluations per second over the `cast` time of that line; and the baseline: one sphmi_sample_points call over all K + 1 march
points of every ray (weight only; the points are built once, OUTSIDE the timed calls) — its call time and, with SPHMI_POINTS_CLOCK,
the library's own line for it — the numpy search for the first crossing on its own, and the two together.  The baseline delivers the
march interval only, 2²⁴ times coarser than the bracket."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
from field_grid_cost import DP, TANK_HI, TANK_LO, timed  # noqa: E402
from sphexample_amd import rays  # noqa: E402
from sphexample_amd.cases import setup_dam_break_3d  # noqa: E402
from sphexample_amd.engine import make_generated_dam_break_engine  # noqa: E402


def ray_sets():
    top = TANK_HI[2]
    gx = np.linspace(TANK_LO[0] + 0.02, TANK_HI[0] - 0.02, 64)
    gauges = np.stack([gx, np.full(64, 0.5 * (TANK_LO[1] + TANK_HI[1])), np.full(64, top)], axis=1)
    u = np.array([(TANK_HI[0] - TANK_LO[0]) / 255, 0.0, 0.0])
    v = np.array([0.0, (TANK_HI[1] - TANK_LO[1]) / 255, 0.0])
    image = rays.pixel_origins([TANK_LO[0], TANK_LO[1], top], u, v, (256, 256))
    return {"gauges": gauges, "image": image}


def evaluations(result, K):
    """Lane evaluations per ray, from the result: the march rounds run, the refinement rounds, the extra record."""
    k = result["interval"]
    found = k >= 1
    last = np.where(found, k, K)
    march = np.minimum(64 * (last // 64 + 1), K + 1)
    return march + np.where(found, 63 * rays.REFINE_ROUNDS, 0)


def measure(eng, label, reps):
    step = 0.5 * float(eng.cfg.h)
    t_end = float(TANK_HI[2] - TANK_LO[2])
    K = int(rays.intervals(0.0, t_end, step))
    down = np.array([0.0, 0.0, -1.0])
    for name, o in ray_sets().items():
        d = np.tile(down, (len(o), 1))
        os.environ.pop("SPHMI_RAYS_CLOCK", None)
        call = timed(lambda: eng.cast_rays(o, d, t_end, step=step), reps)
        r = eng.cast_rays(o, d, t_end, step=step)
        ev = evaluations(r, K)

        # the baseline's points are built ONCE, outside every timed call: a caller who casts the same rays again keeps them
        t = rays.march_t(0.0, t_end, step, np.arange(K + 1), K)
        x = np.ascontiguousarray(rays.ray_points(o[:, None, :], d[:, None, :], np.broadcast_to(t, (len(o), K + 1))).reshape(-1, 3))

        def sample():
            return eng.sample_points(x, fields=("weight",))["weight"]

        def search(S):
            inside = S.reshape(len(o), K + 1) >= 0.5
            cross = ~inside[:, :-1] & inside[:, 1:]
            return np.where(cross.any(1), cross.argmax(1) + 1, -1)

        S = sample()
        samp, srch = timed(sample, reps), timed(lambda: search(S), reps)
        base = timed(lambda: search(sample()), reps)
        same = int((search(S) == r["interval"]).sum())
        print(f"[{label}] {name}: {len(o)} rays, K = {K}, {int((r['status'] & 1).sum())} hit; cast_rays call {call[0]:.2f} ms (min {call[1]:.2f}, max {call[2]:.2f}); "
              f"{ev.mean():.1f} evaluations per ray, {int(ev.sum())} in all; baseline over {len(x)} points built beforehand: sample_points call {samp[0]:.2f} ms "
              f"(min {samp[1]:.2f}, max {samp[2]:.2f}) + host search {srch[0]:.2f} ms = {base[0]:.2f} ms together (min {base[1]:.2f}, max {base[2]:.2f}); "
              f"the same march interval for {same} rays", flush=True)
        os.environ["SPHMI_POINTS_CLOCK"] = "1"
        sys.stderr.write(f"[{label}] {name}: baseline: "); sys.stderr.flush()
        sample()
        os.environ.pop("SPHMI_POINTS_CLOCK", None)
        os.environ["SPHMI_RAYS_CLOCK"] = "1"
        sys.stderr.write(f"[{label}] {name}: "); sys.stderr.flush()
        eng.cast_rays(o, d, t_end, step=step)
        os.environ.pop("SPHMI_RAYS_CLOCK", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--time", type=float, default=0.0)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    eng = make_generated_dam_break_engine(DP, setup_dam_break_3d(DP), device_float_bytes=4)
    eng.advance(1e9, max_steps=args.steps)
    measure(eng, f"N={eng.N}, fp32, {args.steps} steps in", args.reps)
    if args.time > 0:
        t0 = time.perf_counter()
        pr = eng.advance(args.time)
        print(f"advanced to t = {pr.total_time:.4f} s, iteration {pr.iteration}, in {time.perf_counter() - t0:.1f} s", flush=True)
        measure(eng, f"N={eng.N}, fp32, t = {pr.total_time:.3f} s", args.reps)
    eng.close()


if __name__ == "__main__":
    main()
