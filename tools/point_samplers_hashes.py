#!/usr/bin/env python3
"""SHA-256 of every output array of the three point samplers (sphmi_sample_points, sphmi_sample_point_gradients,
sphmi_sample_point_moments) on the fixtures dam_break_2d (8 steps in) and dam_break_3d_shipped (5 steps in), fp64 and fp32 handles:
one line per array.  Run it once per library ($SPHMI_LIB names another build) and compare the two outputs: a change that is to
leave the samplers' bits alone leaves every line alone.

    python tools/point_samplers_hashes.py > tree.txt;  SPHMI_LIB=/path/to/other/libsphmi.so python tools/point_samplers_hashes.py > other.txt

The cloud is seeded: 4 000 points drawn over the box of the rows widened by 2 H (points in the fluid, at the surface, in air and
outside the grid), 600 points inside one cell (three tiles of one block), 12 points ON particles (r = 0) and a point far outside."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import conftest  # noqa: E402
from sphexample_amd.engine import make_engine  # noqa: E402

CASES = {"dam_break_2d": (conftest.load_dam_break_2d, 8), "dam_break_3d_shipped": (conftest.load_dam_break_3d_shipped, 5)}


def cloud(eng):
    d = eng.download(("Position", "Type"))
    X = d["Position"].astype(np.float64)
    F = X[d["Type"] == 1]
    H = eng.cfg.H
    rng = np.random.default_rng(11)
    c = np.round(F[len(F) // 2] / H)
    return np.ascontiguousarray(np.concatenate([
        rng.uniform(X.min(0) - 2 * H, X.max(0) + 2 * H, (4000, X.shape[1])),
        (c + rng.uniform(-0.45, 0.45, (600, X.shape[1]))) * H,
        F[rng.choice(len(F), 12, replace=False)],
        X.max(0)[None] + 100.0]))


def main():
    for case, (load, steps) in CASES.items():
        p, s = load()
        for fb in (8, 4):
            eng = make_engine(p, s, device_float_bytes=fb)
            eng.advance(1e9, max_steps=steps)
            x = cloud(eng)
            for call in ("sample_points", "sample_point_gradients", "sample_point_moments"):
                out = getattr(eng, call)(x)
                for key in sorted(out):
                    a = np.ascontiguousarray(out[key])
                    print(f"{case} fp{8 * fb} {steps} steps in, {len(x)} points: {call}.{key} {a.dtype} {a.shape} "
                          f"{hashlib.sha256(a.tobytes()).hexdigest()}", flush=True)
            eng.close()


if __name__ == "__main__":
    main()
