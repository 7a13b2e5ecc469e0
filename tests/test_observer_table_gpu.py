"""The seven per-step observers behind one corrector (group forces, probes, budgets, flow, envelopes, maps, tracers:
csrc/sphmi_step_record.h, Engine::observe_step) — needs a real MI355X.

The observers share the step loop, the batch clock and the place of a step's record; none of them may see whether another one is
on.  So a handle with ALL of them enabled delivers, byte for byte, what seven handles with ONE observer each deliver, and ends in
the state of a handle with none.  40 steps of the perturbed 2-D dam break cross a batch boundary (32 steps) and Δx-triggered
rebuilds; no comparison has a tolerance."""
import numpy as np
import pytest

from conftest import perturbed
from sphexample_amd import flow

pytestmark = pytest.mark.gpu

STEPS = 40
EVERY = ("Position", "Velocity", "Acceleration", "Density", "Pressure", "Type", "ID", "GroupMarker")
SERIES = ("group_forces", "probes", "budgets", "flow")          # the observers a multi-device handle serves
ALL = SERIES + ("envelopes", "maps", "tracers")


def _flat(v, prefix=""):
    """a read, whatever its shape (tuple, dict, nested dict), as {name: bytes}"""
    if isinstance(v, dict):
        return {k2: b for k, x in v.items() for k2, b in _flat(x, f"{prefix}{k}.").items()}
    if isinstance(v, (tuple, list)):
        return {k2: b for k, x in enumerate(v) for k2, b in _flat(x, f"{prefix}{k}.").items()}
    return {prefix.rstrip("."): np.ascontiguousarray(v).tobytes()}


def _run(p, s, fb, on, **kw):
    """one handle, the observers `on` enabled, STEPS steps: (rebuilds inside the window, {observer: read}, download)"""
    from sphexample_amd.engine import make_engine
    eng = make_engine(p, s, device_float_bytes=fb, **kw)
    fluid = p.Position[p.Type == 1]
    lo, hi = fluid.min(axis=0), fluid.max(axis=0)
    mid = 0.5 * (lo + hi)
    if "group_forces" in on:
        eng.group_forces_enable([1, 2], capacity=256)
    if "probes" in on:
        eng.probes_enable(np.array([mid, lo + 0.25 * (hi - lo), [hi[0] + 10.0, mid[1]]]), capacity=256)      # the third: outside the grid
    if "budgets" in on:
        eng.budgets_enable(capacity=256)
    if "flow" in on:
        eng.flow_enable(*flow.strips(0, [mid[0]], 2), capacity=256)
    if "envelopes" in on:
        eng.envelopes_enable(("Fluid", "Fixed"))
    if "maps" in on:
        eng.maps_enable(origin=lo - 0.01, spacing=[(hi[0] - lo[0] + 0.5) / 8, np.inf], counts=[8, 1], up_axis=1)
    if "tracers" in on:
        rows = np.flatnonzero(p.Type == 1)
        eng.tracers_enable(particles=[int(rows[0]), int(rows[-1])], drifters=np.array([mid, lo + 0.75 * (hi - lo)]), capacity=256)
    pr0 = eng.advance(0.0, max_steps=0)
    pr = eng.advance(1e9, max_steps=STEPS)
    assert pr.steps_done == STEPS
    reads = {name: _flat(getattr(eng, name + "_read")()) for name in on}
    for name, r in reads.items():
        assert r, name
    d = {k: v.tobytes() for k, v in eng.download(EVERY).items()}
    eng.close()
    return pr.n_rebuilds - pr0.n_rebuilds, reads, d


def _compare(p, s, fb, names, **kw):
    rebuilds, together, d = _run(p, s, fb, names, **kw)
    print(f"fp{8 * fb}: rebuilds inside the window: {rebuilds}")
    assert rebuilds >= 2                                         # the one every first step runs, and at least one asked for by Δx
    for name in names:
        r, alone, _ = _run(p, s, fb, (name,), **kw)
        assert r == rebuilds, name
        assert sorted(alone[name]) == sorted(together[name]), name
        # every executed step was observed: a series holds STEPS samples (group_forces_read is a tuple, `time` its second array) …
        if name in ("envelopes", "maps"):
            assert alone[name]["steps"] == np.ascontiguousarray(STEPS).tobytes(), name
        else:
            assert len(alone[name]["1" if name == "group_forces" else "time"]) == 8 * STEPS, name
        # … and what the handle with every observer delivers is what this one delivers
        for key, b in alone[name].items():
            assert together[name][key] == b, (name, key)
    _, _, d0 = _run(p, s, fb, (), **kw)
    for key in EVERY:
        assert d[key] == d0[key], key


@pytest.mark.parametrize("fb", [8, 4])
def test_all_observers_together_equal_each_alone(dam_break_2d, fb):
    p0, s = dam_break_2d
    _compare(perturbed(p0, seed=3, vel_scale=6.0), s, fb, ALL)


def test_slabs_in_one_handle(dam_break_2d):
    """two slabs on one device: the four observers a multi-device handle serves, together against each alone"""
    p0, s = dam_break_2d
    _compare(perturbed(p0, seed=3, vel_scale=6.0), s, 4, SERIES, devices=[0, 0])
