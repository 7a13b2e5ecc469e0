"""The host side the on-demand results share (csrc/sphmi_results.h: DeviceBuf, scan64, PassClock, HeldResult) on the paths no other
file walks — needs a real MI355X.

1. Buffers that grow, are reused for a smaller result and grow again give the bytes of a fresh handle that makes only the last call.
2. A release in the middle: the next build gives the bytes of the first, and releasing one result leaves another one as it was.
3. Lattices of 2 047, 2 048 and 2 049 nodes — the scan tile is kNlScanTile = 2 048 — give the mesh of the numpy restatement.
4. The three $SPHMI_*_TIMING lines keep the words tools/*_cost.py parse; without the variables nothing is written.

Everything on the 2-D dam-break fixture, a dozen steps in; runs of one upload are equal to the bit (the *_repeats_and_does_not_disturb
tests of the neighbouring files rest on the same).
"""
import re

import numpy as np
import pytest

from sphexample_amd import isosurface
from sphexample_amd._abi import ERR_STATE, SphmiError
from test_probes_gpu import _engine, _state

pytestmark = pytest.mark.gpu

STEPS = 12
IRR = np.array([0.318309886, 0.577215665])                          # offsets in units of dp: nothing the particle lattice knows


def _stepped(request, fb, handles=1):
    p, s = _state("dam_break_2d", request)
    engines = [_engine(p, s, fb) for _ in range(handles)]
    for e in engines:
        assert e.advance(1e9, max_steps=STEPS).iteration == STEPS
    return engines, s


def _same(a, b, what):
    a, b = (list(a.values()), list(b.values())) if isinstance(a, dict) else (list(a), list(b))
    assert len(a) == len(b), what
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, k, x.shape, y.shape)


def _fluid_box(eng):
    d = eng.download(("Position", "Type"))
    F = d["Position"].astype(np.float64)[d["Type"] == 1]
    return F.min(0), F.max(0), int((d["Type"] == 1).sum())


def _over_the_fluid(eng, nx, ny):
    """A lattice of nx × ny nodes that overhangs the fluid by 0.4 H on every side: the free surface crosses it."""
    flo, fhi, _ = _fluid_box(eng)
    c = np.array([nx, ny], dtype=np.int64)
    return flo - 0.4 * eng.cfg.H + IRR * eng.cfg.dx, (fhi + 0.8 * eng.cfg.H - flo) / (c - 1), c


# ---- 1. grow, shrink, grow ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fb", [8, 4])
def test_grow_shrink_grow_equals_a_fresh_handle(fb, request):
    (used, fresh), s = _stepped(request, fb, handles=2)
    # neighbours: HALF → FULL (the entries double) → HALF
    half = used.neighbors_build(half=True)
    full = used.neighbors_build(half=False)
    assert full == (half[0], 2 * half[1]) and half[1] > 0
    assert used.neighbors_build(half=True) == half
    assert fresh.neighbors_build(half=True) == half
    _same(used.neighbors_read(), fresh.neighbors_read(), "neighbours")
    # components: every fluid row its own component (the per-component buffers at their largest) → a handful → every row again
    _, _, n_fluid = _fluid_box(used)
    small, H = 0.25 * s.SimConstants.dx, used.cfg.H
    first = used.components_build(small)
    few = used.components_build(H)
    print(f"fp{8 * fb}: {n_fluid} fluid rows, {first[1]} components with link dp / 4, {few[1]} with link H")
    assert first[1] == n_fluid and 0 < few[1] < n_fluid // 10
    assert used.components_build(small) == first
    assert fresh.components_build(small) == first
    _same(used.components_read(), fresh.components_read(), "components")
    # the mesh and the lattice sums: 5 × 4 nodes → 40 × 30 → 5 × 4
    coarse, fine = _over_the_fluid(used, 5, 4), _over_the_fluid(used, 40, 30)
    a = used.isosurface_build(*coarse)
    b = used.isosurface_build(*fine)
    assert b[0] > a[0] > 0 and b[1] > a[1] > 0
    assert used.isosurface_build(*coarse) == a
    assert fresh.isosurface_build(*coarse) == a
    _same(used.isosurface_read(pressure=True, velocity=True), fresh.isosurface_read(pressure=True, velocity=True), "mesh")
    used.sample_grid(*coarse)
    used.sample_grid(*fine)
    _same(used.sample_grid(*coarse), fresh.sample_grid(*coarse), "lattice sums")
    # … and none of it disturbed what the handle holds: the earlier results still read back the same
    _same(used.neighbors_read(), fresh.neighbors_read(), "neighbours, after the others")
    _same(used.components_read(), fresh.components_read(), "components, after the others")
    used.close()
    fresh.close()


# ---- 2. a release in the middle ------------------------------------------------------------------------------------------------
def test_release_in_the_middle(request):
    (eng,), s = _stepped(request, 8)
    lattice = _over_the_fluid(eng, 40, 30)
    kinds = {   # name → (build, read, release, what a read without a result says)
        "neighbours": (lambda: eng.neighbors_build(half=True), eng.neighbors_read, eng.neighbors_release, "no neighbour list"),
        "components": (lambda: eng.components_build(1.2 * s.SimConstants.dx), eng.components_read, eng.components_release, "no components"),
        "mesh": (lambda: eng.isosurface_build(*lattice), lambda: eng.isosurface_read(pressure=True, velocity=True), eng.isosurface_release, "no mesh"),
    }

    def refused(read, words):
        with pytest.raises(SphmiError) as ei:
            read()
        assert ei.value.status == ERR_STATE and words in str(ei.value), str(ei.value)

    first = {}
    for name, (build, read, release, words) in kinds.items():
        shape = build()
        first[name] = read()
        release()
        refused(read, words)
        assert build() == shape
        _same(read(), first[name], f"{name}, built again after a release")
        release()
    names = list(kinds)
    for a, b in zip(names, names[1:] + names[:1]):                                   # two held at once: releasing `a` leaves `b` alone
        (build_a, read_a, release_a, words_a), (build_b, read_b, release_b, _) = kinds[a], kinds[b]
        build_a(); build_b()
        _same(read_a(), first[a], a)
        release_a()
        refused(read_a, words_a)
        _same(read_b(), first[b], f"{b}, after the release of {a}")
        build_a()
        _same(read_a(), first[a], f"{a}, built again beside {b}")
        _same(read_b(), first[b], f"{b}, after {a} was built again")
        release_a(); release_b()
    assert eng.advance(1e9, max_steps=1).steps_done == 1
    eng.close()


# ---- 3. the scan's tile edge for a lattice ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("fb", [8, 4])
def test_lattices_around_one_scan_tile(fb, request):
    (eng,), _ = _stepped(request, fb)
    flo, fhi, _ = _fluid_box(eng)
    H, dp = eng.cfg.H, eng.cfg.dx
    lattices = {2047: _over_the_fluid(eng, 23, 89), 2048: _over_the_fluid(eng, 64, 32)}
    # 3 × 683: three columns through the middle of the fluid, from under its floor to over its surface
    o = np.array([0.5 * (flo[0] + fhi[0]) - 1.1 * dp, flo[1] - 0.4 * H]) + IRR * dp
    lattices[2049] = (o, np.array([1.1 * dp, (fhi[1] + 0.8 * H - flo[1]) / 682]), np.array([3, 683], dtype=np.int64))
    for nodes, lattice in lattices.items():
        assert int(np.prod(lattice[2])) == nodes
        got = eng.isosurface(*lattice, attributes=True)
        out = eng.sample_grid(*lattice)
        ref = isosurface.extract(out["weight"], lattice[0], lattice[1], 0.5, pressure=out["pressure"], velocity=out["velocity"], count=out["count"])
        print(f"fp{8 * fb}: {nodes} nodes {tuple(int(c) for c in lattice[2])}: {len(ref[0])} vertices, {len(ref[1])} elements")
        assert len(ref[1]) > 0, nodes                                               # the surface crosses the lattice
        np.testing.assert_array_equal(got[1], ref[1], err_msg=f"{nodes} nodes: elements")
        _same(got, ref, f"{nodes} nodes")
    eng.close()


# ---- 4. the timing lines -----------------------------------------------------------------------------------------------------
TIMING = {   # variable → (prefix of the line, its passes in order)
    "SPHMI_NEIGHBORS_TIMING": ("sphmi_neighbors_build:", ("count", "scan", "fill")),
    "SPHMI_COMPONENTS_TIMING": ("sphmi_components_build:", ("init", "hook", "flatten", "number", "table")),
    "SPHMI_ISOSURFACE_TIMING": ("sphmi_isosurface_build:", ("sample", "classify", "scans", "vertices", "elements")),
}


def test_the_timing_lines(request, monkeypatch, capfd):
    (eng,), _ = _stepped(request, 4)
    lattice = _over_the_fluid(eng, 40, 30)

    def build_each():
        eng.neighbors_build()
        eng.components_build()
        eng.isosurface_build(*lattice)

    for var in TIMING:
        monkeypatch.delenv(var, raising=False)
    capfd.readouterr()
    build_each()
    assert "sphmi_" not in capfd.readouterr().err                                   # unset: nothing is written
    for var in TIMING:
        monkeypatch.setenv(var, "1")
    build_each()
    lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("sphmi_")]
    print("\n".join(lines))
    assert len(lines) == len(TIMING)
    number = r"\d+\.\d+"
    for line, (prefix, passes) in zip(lines, TIMING.values()):
        assert line.startswith(prefix), line
        assert re.search(r": " + ", ".join(rf"{name} {number} ms" for name in passes) + "$", line), line
    eng.close()
