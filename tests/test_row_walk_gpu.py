"""The second batch of ranges of the workgroup candidate walk (the walk k_field_grid, k_particle_fields and the neighbour list's
nl_walk each carry: csrc/sphmi_field_grid.h, sphmi_particle_fields.h, sphmi_neighbor_list.h) — needs a real MI355X.

A workgroup takes its (cy, cz) ranges 256 per batch.  The dense cases of the per-feature tests span a few cells per run or brick and
stay inside the first batch; here a SPARSE 3-D cloud makes one run of 256 rows, and one brick of a coarse lattice, span more than
256 ranges, so that the range tables are refilled behind a barrier while the staging buffers are reused.  `nrange` is restated on
the host from the span formula of those headers and asserted, so that the cases cannot silently stop reaching that path.  Every result
is held to the enumeration and the bars of the neighbouring test of its feature.
(k_point_cloud cannot get there: a tile spans at most B cells plus the reach per axis, at most 8 x 8 ranges.  It has no case.)
"""
import numpy as np
import pytest

import test_components_gpu as cc
import test_field_grid_gpu as fg
import test_neighbor_list_gpu as nl
import test_particle_fields_gpu as pf
from test_probes_gpu import _engine

pytestmark = pytest.mark.gpu

SITES = (2, 7, 8)                                                                   # per axis, 3 H apart; x fastest in the sorted order


def _sparse_cloud(H):
    """Sites 3 H apart at cell centres (cells are H wide, centred on the multiples of H), at each a cluster of two or three rows
    within 0.2 H of it per axis: every row is within H of the rows of its cluster and more than 2 H from every other."""
    rng = np.random.default_rng(41)
    pos = []
    for n, site in enumerate(np.ndindex(*SITES[::-1])):
        centre = (10.0 + 3.0 * np.array(site[::-1])) * H
        for _ in range(2 + n % 2):
            pos.append(centre + rng.uniform(-0.2, 0.2, 3) * H)
    return np.array(pos)


def _cells(cfg, X):
    """The hash of the rows: trunc(|x| / H + 1/2) with the sign of x; the padded grid around them (gmin, np)."""
    c = (np.sign(X) * np.trunc(np.abs(X) * cfg.H_inv + 0.5)).astype(np.int64)
    return c.min(0), c.max(0) - c.min(0) + 3


def _nrange(cfg, first, last, gmin, npad):
    """The span of the kernels restated: the (cy, cz) ranges of the span from `first` to `last`, 0 where it misses the grid."""
    reach = cfg.H + cfg.h
    a, b = (first - reach) * cfg.H_inv, (last + reach) * cfg.H_inv
    a = a - 1e-6 * (1.0 + np.abs(a)); b = b + 1e-6 * (1.0 + np.abs(b))
    lo = np.maximum(np.ceil(a - 0.5) + (1.0 - gmin), 0.0)
    hi = np.minimum(np.floor(b + 0.5) + (1.0 - gmin), npad - 1.0)
    if not (lo <= hi).all():
        return 0
    n = (hi - lo + 1).astype(np.int64)
    return int(n[1] * n[2])


def _sparse_engine(fb, request):
    """The cloud as Fluid rows with random velocities, one step in; its download.  The first run of 256 rows spans > 256 ranges."""
    p0, s = request.getfixturevalue("dam_break_3d_shipped")
    pos = _sparse_cloud(s.SimKernel.H)
    assert 256 < len(pos) < 512
    p = nl._cloud(p0, len(pos), pos)
    p.Type[...] = 1
    p.Velocity[...] = np.random.default_rng(23).uniform(-0.1, 0.1, p.Velocity.shape)
    eng = _engine(p, s, fb)
    assert eng.advance(1e9, max_steps=1).iteration == 1
    X = np.asarray(eng.download(("Position",))["Position"], np.float64)
    gmin, npad = _cells(eng.cfg, X)
    runs = [_nrange(eng.cfg, X[a:a + 256].min(0), X[a:a + 256].max(0), gmin, npad) for a in range(0, len(X), 256)]
    print(f"sparse cloud fp{8 * fb}: {len(X)} rows, grid {npad.tolist()}, (cy, cz) ranges per run of 256 rows {runs}")
    assert npad[1] >= 17 and npad[2] >= 17 and runs[0] > 256
    return eng, X, gmin, npad


@pytest.mark.parametrize("fb", [8, 4])
def test_particle_fields_past_the_first_batch(fb, request):
    eng, X, _, _ = _sparse_engine(fb, request)
    got, ref, _ = pf._check(eng, fb, "sparse cloud")
    assert sorted(set(got["count"].tolist())) == [1, 2]                             # the other rows of the cluster, no row of another
    eng.close()


@pytest.mark.parametrize("fb", [8, 4])
def test_neighbor_list_past_the_first_batch(fb, request):
    """Count, fill and HALF (nl._check builds both lists)."""
    eng, X, _, _ = _sparse_engine(fb, request)
    off, nbr, _ = nl._check(eng, f"sparse cloud fp{8 * fb}")
    assert sorted(set(np.diff(off).tolist())) == [1, 2]
    eng.close()


@pytest.mark.parametrize("fb", [8, 4])
def test_components_past_the_first_batch(fb, request):
    eng, X, _, _ = _sparse_engine(fb, request)
    got, _, _ = cc._check(eng, f"sparse cloud fp{8 * fb}", None, cc.FLUID)
    assert len(got["count"]) == int(np.prod(SITES)) and sorted(set(got["count"].tolist())) == [2, 3]      # one body per site
    eng.close()


@pytest.mark.parametrize("fb", [8, 4])
def test_lattice_past_the_first_batch(fb, request):
    """A coarse lattice of ONE brick (its nodes fit a workgroup) over the cloud: the brick's span holds more than 256 ranges."""
    eng, X, gmin, npad = _sparse_engine(fb, request)
    H = eng.cfg.H
    origin, spacing, counts = X.min(0) - 0.15 * H, np.full(3, 2.0 * H), np.array([4, 8, 8], np.int64)
    assert int(np.prod(counts)) <= 256                                              # fg_plan_brick: the whole lattice is one brick
    nrange = _nrange(eng.cfg, origin, origin + (counts - 1) * spacing, gmin, npad)
    print(f"lattice {counts.tolist()} at 2 H: (cy, cz) ranges of its brick {nrange}")
    assert nrange > 256
    out, ref, _ = fg._check_lattice(eng, (origin, spacing, counts), fb, "sparse cloud, coarse lattice")
    assert (ref["n"] > 0).sum() >= 3
    eng.close()
