"""Every output of the three samplers at arbitrary points asked for ON ITS OWN (sphmi_sample_points, sphmi_sample_point_gradients,
sphmi_sample_point_moments) — needs a real MI355X.

The host fetches only the slots the requested outputs need, by the tables of csrc/sphmi_series.h (kPgOutputs, kPmOutputs); the other
outputs travel as NULL.  tests/host_series/series_main.cpp drives those tables for every subset on the host; here each output is
fetched alone through the whole call, on a one-device handle and on a handle of two slabs:

  - a call for one output delivers the bits the call for all outputs delivers for it (np.array_equal);
  - S, n, SP, Sρ and Sv of the gradients and of the moments are the same bits, and they are the cloud's (that call delivers SP / S,
    so the quotient of the raw sums is compared, a correctly rounded division on both sides — as
    tests/test_point_gradients_gpu.py::test_agrees_with_sample_points does);
  - the two-slab handle delivers the one-device handle's sums within 1e-9 (fp64 handles) / 1e-5 (fp32) of each sum's largest
    magnitude over the points, the bars of tests/test_sample_points_gpu.py::test_slabs_in_one_handle for sums added over slabs.

Five points: four next to Fluid rows, one outside the cell grid (all zeros).
"""
import numpy as np
import pytest

from test_point_gradients_gpu import _fluid
from test_point_gradients_host import IRR
from test_probes_gpu import _engine, _state

pytestmark = pytest.mark.gpu

STEPS = 5
SHARED = ("weight", "count", "sum_pressure", "sum_density", "sum_velocity")
SAMPLERS = {"sample_points": "GRID_FIELDS", "sample_point_gradients": "GRADIENT_FIELDS", "sample_point_moments": "MOMENT_FIELDS"}


def _all_and_each(eng, pts):
    """{sampler: the call with all outputs}, after asserting that every output asked for alone holds the same bits."""
    full = {}
    for call, table in SAMPLERS.items():
        names = tuple(getattr(eng, table))
        full[call] = getattr(eng, call)(pts)
        assert set(names) <= set(full[call]), (call, names)
        for name in names:
            one = getattr(eng, call)(pts, fields=(name,))
            assert set(one) - {"h", "dims"} == {name}, (call, name, set(one))
            assert one[name].dtype == full[call][name].dtype and one[name].shape == full[call][name].shape, (call, name)
            assert np.array_equal(one[name], full[call][name]), (call, name, int((one[name] != full[call][name]).sum()))
    return full


def _shared_sums_agree(full):
    c, g, m = full["sample_points"], full["sample_point_gradients"], full["sample_point_moments"]
    for k in SHARED:
        assert np.array_equal(g[k], m[k]), ("gradients against moments", k)
    S, n = g["weight"], g["count"]
    some = (n > 0) & (S > 0)
    safe = np.where(some, S, 1.0)
    assert np.array_equal(c["weight"], S) and np.array_equal(c["count"], n)
    assert np.array_equal(c["pressure"], np.where(some, g["sum_pressure"] / safe, 0.0))
    assert np.array_equal(c["density"], np.where(some, g["sum_density"] / safe, 0.0))
    assert np.array_equal(c["velocity"], np.where(some[:, None], g["sum_velocity"] / safe[:, None], 0.0))


@pytest.mark.parametrize("fb", [8, 4])
@pytest.mark.parametrize("case", ["dam_break_2d", "dam_break_3d_shipped"])
def test_every_output_alone(case, fb, request):
    p, s = _state(case, request)
    one, two = _engine(p, s, fb), _engine(p, s, fb, devices=[0, 0], slab_axis=0)
    pa, pb = one.advance(1e9, max_steps=STEPS), two.advance(1e9, max_steps=STEPS)
    assert (pb.iteration, pb.steps_done) == (pa.iteration, pa.steps_done) == (STEPS, STEPS)
    assert two.multi_info().world == 2
    F = _fluid(one)
    H, D = one.cfg.H, one.D
    inside = F[np.linspace(0, len(F) - 1, 4).astype(int)] + IRR[:D] * one.cfg.dx
    pts = np.concatenate([inside[:2], F.max(0)[None, :] + 50.0 * H, inside[2:]])      # the point outside the grid in the middle of the call
    a, b = _all_and_each(one, pts), _all_and_each(two, pts)
    _shared_sums_agree(a)
    _shared_sums_agree(b)
    g = a["sample_point_gradients"]
    assert (g["count"][[0, 1, 3, 4]] > 0).all() and np.abs(g["grad_velocity"]).max() > 0 and np.abs(a["sample_point_moments"]["moment_velocity"]).max() > 0
    for out in a.values():
        for k, v in out.items():
            if k not in ("h", "dims"):
                assert (v[2] == 0).all(), k                                        # outside the grid: exact zeros
    tol = 1e-9 if fb == 8 else 1e-5
    for call in SAMPLERS:
        for k, v in a[call].items():
            if k in ("h", "dims"):
                continue
            w = b[call][k]
            if call == "sample_points" and k in ("pressure", "density", "velocity"):      # the bar is for the SUMS: S · mean, as that test forms them
                Sa, Sb = a[call]["weight"], b[call]["weight"]
                v, w = (Sa * v, Sb * w) if v.ndim == 1 else (Sa[:, None] * v, Sb[:, None] * w)
            scale = np.abs(v).max()
            worst = np.abs(w - v).max() / scale if scale > 0 else np.abs(w).max()
            print(f"{case} fp{8 * fb} {call} {k}: two slabs against one device {worst:.3g} (bar {tol:g})")
            assert worst <= tol, (call, k, worst, tol)
    one.close(); two.close()
