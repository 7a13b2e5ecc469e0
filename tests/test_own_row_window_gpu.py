"""The own-row window of the neighbour kernel (sphmi_kernels.h, `kWindow`) against the fp64 oracle.

The launches of 3 000 tiles and more (fp32, half tiles of one wave per half, two tiles per workgroup, the compiled-in default model)
stage the records of 256 consecutive indices around a workgroup's targets in LDS and read the neighbours inside that range from
there.  Every case below runs at ≥ 3 000 tiles per launch, so that this instantiation is the one launched, and covers the window's
edge cases:
  * workgroups whose targets straddle two cell rows, and windows clipped at index 0 and at N: every lattice has them (the first and
    the last tile of the sorted order; rows end every few tiles);
  * N not a multiple of 64 (the last tile is partial);
  * a cell row longer than the window (a larger smoothing length: ≈ 140 records per cell, the three cells of a row ≈ 420 > 256);
  * a slab handle: its record arrays hold ghost rows, which the window stages like any other record;
  * a rebuild between calls (every advance() call opens with one), so that the window follows a new sort;
  * workgroups whose two tiles are not neighbours in the sorted order (cost-class boundaries of the tile schedule): the second tile has no
    window and gathers every neighbour.
Tolerances: those of tests/test_full_resolution_gpu.py (state < 1e-5 of the field maximum after K steps).
"""
import dataclasses
import os

import numpy as np
import pytest

from conftest import perturbed
from sphexample_amd import cases

pytestmark = pytest.mark.gpu

TOL_STATE = 1e-5
MIN_TILES = 3000                 # the engine's default waves-per-tile choice: two waves per tile, two tiles per workgroup from here on


@pytest.fixture(autouse=True)
def _default_launch_shape(monkeypatch):
    """The launch-shape overrides of experiment runs would move these launches off the window kernel: the defaults hold here."""
    for k in ("SPHMI_WPT", "SPHMI_WPT2_BELOW", "SPHMI_TPB", "SPHMI_TPB2"):
        monkeypatch.delenv(k, raising=False)


def _threads():
    from oracle.oracle import Oracle
    return max(1, min(16, os.cpu_count() or 1, Oracle.max_threads()))


def _by_id(st):
    order = np.argsort(st["ID"], kind="stable")
    return {k: v[order] for k, v in st.items()}


def _relmax(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _compare(p, s, calls, steps, **engine_kw):
    from oracle.oracle import make_oracle
    from sphexample_amd.engine import make_engine
    eng = make_engine(p, s, device_float_bytes=4, **engine_kw)
    orc = make_oracle(p, s, threads=_threads())
    try:
        for _ in range(calls):
            pe = eng.advance(1e9, max_steps=steps)
            po = orc.advance(1e9, max_steps=steps)
            assert (pe.iteration, pe.n_rebuilds) == (po.iteration, po.n_rebuilds)
            assert abs(pe.last_dt - po.last_dt) / po.last_dt < TOL_STATE
            e = _by_id(eng.download(("ID", "Density", "Position", "Velocity")))
            o = _by_id(orc.download(("ID", "Density", "Position", "Velocity")))
            np.testing.assert_array_equal(e["ID"], o["ID"])
            assert _relmax(e["Density"], o["Density"]) < TOL_STATE
            assert float(np.abs(e["Position"] - o["Position"]).max() / np.abs(o["Position"]).max()) < TOL_STATE
            assert float(np.abs(e["Velocity"] - o["Velocity"]).max() / max(np.abs(o["Velocity"]).max(), 1e-12)) < 1e-3
        assert pe.n_rebuilds >= calls
    finally:
        eng.close(); orc.close()


def test_window_on_a_partial_last_tile_matches_the_oracle():
    """287 622 particles = 4 494 tiles and 6 particles: the windows of the first and the last workgroups are clipped to [0, N)."""
    dp = 0.0068
    p = cases.dam_break_3d(dp)
    assert len(p) // 64 >= MIN_TILES and len(p) % 64 != 0
    _compare(perturbed(p, seed=11), cases.setup_dam_break_3d(dp), calls=2, steps=2)


def test_window_shorter_than_a_cell_row_matches_the_oracle():
    """Smoothing length ×1.5: a target's own row (three cells, ≈ 420 records) is longer than the 256-record window."""
    dp = 0.0068
    p = cases.dam_break_3d(dp)
    s = cases.setup_dam_break_3d(dp)
    s = dataclasses.replace(s, SimKernel=cases.SPHKernelInstance(3, cases.WendlandC2(), h=1.5 * np.sqrt(3 * dp ** 2)))
    assert len(p) // 64 >= MIN_TILES
    _compare(perturbed(p, seed=12), s, calls=2, steps=1)


def test_window_over_ghost_rows_of_slabs_matches_the_oracle():
    """Two slabs of 517 818 particles on one GPU (≥ 4 000 tiles each): windows of the slab-edge tiles hold ghost records."""
    dp = 0.0055
    p = cases.dam_break_3d(dp)
    assert len(p) // 128 >= MIN_TILES
    _compare(perturbed(p, seed=13), cases.setup_dam_break_3d(dp), calls=2, steps=2, devices=[0, 0], slab_axis=0)
