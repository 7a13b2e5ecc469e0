"""The connected bodies of selected rows, labelled on the device (sphmi_components_build / _read / _release,
csrc/sphmi_components.h) — needs a real MI355X.

The reference is computed HERE from the download taken right after the build: an enumeration of every pair with
r^2 = ((dx^2 + dy^2) + dz^2) <= link^2 (rows sorted along x so that only a window of candidates is tested; the cut itself is the
exact one), then scipy's connected_components — or the plain union–find of tests/test_components_host.py where scipy does not
import — canonicalised to ascending first row.  It never goes through the code under test nor through sphexample_amd.components,
which is separately held to the same reference.  label, first_row, count and box must be EQUAL to it, on fp64 and on fp32 handles.

Not tested here: the loop bounds of the union–find (reviewed, not exercised: no state reaches them) and SPHMI_ERR_DEVICE.
"""
import ctypes as C

import numpy as np
import pytest

from sphexample_amd import components, neighbors
from sphexample_amd._abi import ERR_ARGUMENT, ERR_STATE, SphmiError
from test_components_host import _union_find
from test_neighbor_list_gpu import _cloud, _refused
from test_probes_gpu import _engine, _state, _variant

pytestmark = pytest.mark.gpu

FLUID, FIXED, ALL = ("Fluid",), ("Fixed",), ("Fluid", "Fixed", "Moving")
TYPE_NO = {"Fluid": 1, "Fixed": 2, "Moving": 3}


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def enumerate_pairs(position, link):
    """(i, j, r2), i < j, of every pair of rows with r2 <= link^2, r2 = ((dx^2 + dy^2) + dz^2) term by term."""
    X = np.asarray(position, np.float64)
    n, D = X.shape
    cut = float(link) * float(link)
    order = np.argsort(X[:, 0], kind="stable")
    Y = X[order]
    I, J, R = [], [], []
    reach = float(link) * (1.0 + 1e-6)                                              # |dx| beyond it: dx^2 alone exceeds the cut
    for a in range(0, n, 512):
        A = Y[a:a + 512]
        e = int(np.searchsorted(Y[:, 0], A[-1, 0] + reach, side="right"))
        B = Y[a:e]                                                                  # sorted position > own only: every pair once
        dx = A[:, None, 0] - B[None, :, 0]
        dy = A[:, None, 1] - B[None, :, 1]
        r2 = dx * dx + dy * dy
        if D == 3:
            dz = A[:, None, 2] - B[None, :, 2]
            r2 = r2 + dz * dz
        ii, jj = np.nonzero(r2 <= cut)
        keep = jj > ii
        ii, jj = ii[keep], jj[keep]
        R.append(r2[ii, jj])
        I.append(order[ii + a]); J.append(order[jj + a])
    I, J, R = np.concatenate(I), np.concatenate(J), np.concatenate(R)
    return np.minimum(I, J), np.maximum(I, J), R


def reference(position, sel, pairs, link):
    """(label, first_row, count, box) from the pairs of `enumerate_pairs` at a link >= this one."""
    X = np.asarray(position, np.float64)
    n, D = X.shape
    i, j, r2 = pairs
    keep = (r2 <= float(link) * float(link)) & sel[i] & sel[j]
    i, j = i[keep], j[keep]
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        _, comp = connected_components(coo_matrix((np.ones(len(i), np.int8), (i, j)), shape=(n, n)), directed=False)
        first_of = np.full(n, n, np.int64)
        np.minimum.at(first_of, comp[sel], np.flatnonzero(sel))
        root = first_of[comp]
    except ImportError:
        root = _union_find(n, i, j, sel)
    firsts = np.unique(root[sel])
    label = np.where(sel, np.searchsorted(firsts, root), -1).astype(np.int32)
    Cn = len(firsts)
    count = np.bincount(label[sel], minlength=Cn).astype(np.int32)
    box = np.zeros((Cn, 6))
    box[:, :D], box[:, 3:3 + D] = np.inf, -np.inf
    for d in range(D):
        np.minimum.at(box[:, d], label[sel], X[sel, d])
        np.maximum.at(box[:, 3 + d], label[sel], X[sel, d])
    return label, firsts.astype(np.int32), count, box


def _selected(typ, types):
    return np.isin(np.asarray(typ), [TYPE_NO[t] for t in types])


def _equal(got, want, what):
    for k, w in zip(("label", "first_row", "count", "box"), want):
        assert got[k].dtype == w.dtype and got[k].shape == w.shape, (what, k, got[k].shape, w.shape)
        np.testing.assert_array_equal(got[k], w, err_msg=f"{what}: {k}")


def _check(eng, what, link, types, d=None, pairs=None, module=True):
    """One build against the reference on the download taken right after it; prints its figures before it asserts.  Returns
    (the device's dict, the download, the pairs at this link — for a shorter link on the same state)."""
    n_rows, n_comp = eng.components_build(link, types)
    got = dict(zip(("label", "first_row", "count", "box"), eng.components_read()))
    d = d or eng.download(("Position", "Type"))
    X = np.asarray(d["Position"], np.float64)
    sel = _selected(d["Type"], types)
    link = eng.cfg.H if link is None else link
    pairs = pairs if pairs is not None else enumerate_pairs(X, link)
    want = reference(X, sel, pairs, link)
    print(f"{what}: {len(X)} rows, {int(sel.sum())} selected, link {link:.6g}: C = {n_comp} (reference {len(want[1])}), "
          f"main body {int(got['count'].max(initial=0))} rows (reference {int(want[2].max(initial=0))})")
    assert n_rows == len(X) and n_comp == len(got["first_row"])
    _equal(got, want, what)
    if eng.D == 2:
        assert (got["box"][:, [2, 5]] == 0).all() and not np.signbit(got["box"][:, [2, 5]]).any()
    if module:                                                                      # the numpy restatement, held to the same reference
        i, j, r2 = pairs
        short = r2 <= link * link
        _equal(components.from_pairs(len(X), i[short], j[short], sel, position=X), want, what + " (components.from_pairs)")
    return got, d, pairs


# ---- 1. the fixtures ---------------------------------------------------------------------------------------------------------------------
CASES = {  # name → (fixture, steps, kernel variant, rows)
    "dam_break_2d": ("dam_break_2d", 30, None, 6881),
    "moving_square": ("moving_square", 25, None, None),
    "cubic_spline": ("dam_break_2d", 20, "cubic", 6881),
    "dam_break_3d_shipped": ("dam_break_3d_shipped", 12, None, 17446),
}


@pytest.mark.parametrize("fb", [8, 4])
@pytest.mark.parametrize("case", list(CASES))
def test_equals_the_reference(case, fb, request):
    fixture, K, kernel, rows = CASES[case]
    p, s = _state(fixture, request)
    if kernel:
        s = _variant(s, kernel, None)
    eng = _engine(p, s, fb)
    assert eng.advance(1e9, max_steps=K).iteration == K
    assert rows is None or len(p) == rows
    if fixture == "moving_square":
        assert eng.cfg.H < 2 * eng.cfg.h                                            # k < 2: five candidate cells per axis
    short = 1.2 * s.SimConstants.dx                                                 # below the diagonal lattice distance: only axis neighbours of an intact lattice link
    assert short < eng.cfg.H
    d = pairs = None
    for types in (FLUID, ALL):
        got, d, pairs = _check(eng, f"{case} fp{8 * fb} {'+'.join(types)} link H", None, types, d, pairs)
        got2, _, _ = _check(eng, f"{case} fp{8 * fb} {'+'.join(types)} link 1.2 dx", short, types, d, pairs)
        assert len(got2["count"]) >= len(got["count"])                              # fewer links never merge more
    # components(): build, read and release in one call — the same arrays, and nothing is held afterwards
    again = eng.components(short, ALL)
    assert all(again[k].tobytes() == got2[k].tobytes() for k in again)
    with pytest.raises(SphmiError):
        eng.components_read()
    if case == "dam_break_2d":                                                      # … and the restatement from the positions alone
        _equal(components.label(d["Position"], _selected(d["Type"], ALL), short), [got2[k] for k in ("label", "first_row", "count", "box")], "components.label")
    eng.close()


# ---- 2. percolating clouds ---------------------------------------------------------------------------------------------------------------
CLOUD_ROWS = 4096
CLOUD_SEED = {2: 5, 3: 3}                                                           # chosen on the host so that the spread below holds


def _percolating(D, H, seed):
    """CLOUD_ROWS uniform points and the link at the percolation threshold of discs (4.5 links per row) / spheres (2.7), at most H."""
    rng = np.random.default_rng(seed)
    link = 0.95 * H
    if D == 2:
        side = link * np.sqrt(CLOUD_ROWS * np.pi / 4.5)
    else:
        side = link * (CLOUD_ROWS * 4.0 / 3.0 * np.pi / 2.7) ** (1.0 / 3.0)
    return 0.1 + side * rng.random((CLOUD_ROWS, D)), link


@pytest.mark.parametrize("fb", [8, 4])
@pytest.mark.parametrize("D", [2, 3])
def test_percolating_cloud(D, fb, request):
    """The case that can break a racing union–find: component sizes spread over three decades, trees of every depth, many lanes
    hooking into the same large trees at once."""
    p0, s = request.getfixturevalue("dam_break_2d" if D == 2 else "dam_break_3d_shipped")
    pos, link = _percolating(D, s.SimKernel.H, CLOUD_SEED[D])
    eng = _engine(_cloud(p0, CLOUD_ROWS, pos, walls=True), s, fb)
    assert eng.advance(1e9, max_steps=1).iteration == 1
    d = eng.download(("Position", "Type"))
    X = np.asarray(d["Position"], np.float64)
    pairs = enumerate_pairs(X, link)
    want = reference(X, np.ones(len(X), bool), pairs, link)
    big = int(want[2].max())
    print(f"{D}-D cloud: {2 * len(pairs[0]) / len(X):.2f} links per row, {len(want[1])} components, largest {big} rows, singletons {int((want[2] == 1).sum())}")
    assert len(want[1]) >= 100 and 0.05 * len(X) <= big <= 0.80 * len(X)            # on the reference alone
    got, _, _ = _check(eng, f"{D}-D cloud fp{8 * fb}", link, FIXED, d, pairs)
    _equal(components.label(X, np.ones(len(X), bool), link), want, "components.label")
    assert eng.components(link, FLUID)["label"].tolist() == [-1] * len(X)           # nothing selected: no component
    eng.close()


# ---- 3. chains ---------------------------------------------------------------------------------------------------------------------------
def _serpentine(step, per_row=40, rows=8):
    pts = []
    for r in range(rows):
        xs = np.arange(per_row) * step
        pts += [(x, 3 * step * r) for x in (xs if r % 2 == 0 else xs[::-1])]
        if r + 1 < rows:
            x_end = xs[-1] if r % 2 == 0 else 0.0
            pts += [(x_end, 3 * step * r + step), (x_end, 3 * step * r + 2 * step)]
    return np.array(pts)


@pytest.mark.parametrize("fb", [8, 4])
@pytest.mark.parametrize("shape", ["line", "gaps", "serpentine"])
def test_chains(shape, fb, request):
    p0, s = request.getfixturevalue("dam_break_2d")
    link = s.SimKernel.H
    if shape == "serpentine":                                                       # the minimum travels the whole walk: 334 rows, one body
        pos = 0.1 + _serpentine(0.9 * link)
        sizes = [len(pos)]
    else:
        gap = np.full(599, 0.9 * link)
        if shape == "gaps":
            gap[49::50] = 1.1 * link                                                # after every 50th row
        pos = np.stack([0.1 + np.concatenate([[0.0], np.cumsum(gap)]), np.full(600, 0.1)], 1)
        sizes = [600] if shape == "line" else [50] * 12
    eng = _engine(_cloud(p0, len(pos), pos, walls=True), s, fb)
    assert eng.advance(1e9, max_steps=1).iteration == 1
    got, d, _ = _check(eng, f"{shape} fp{8 * fb}", link, FIXED)
    assert got["count"].tolist() == sizes
    if shape != "serpentine":
        assert (np.diff(d["Position"][:, 0]) > 0).all()                             # rows ascend along the line: a body spans runs of 256
        assert got["first_row"].tolist() == list(range(0, 600, 600 // len(sizes)))
    eng.close()


# ---- 4. types ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fb", [8, 4])
def test_types(fb, request):
    p0, s = request.getfixturevalue("dam_break_2d")
    H = s.SimKernel.H
    blob = np.stack(np.meshgrid(np.arange(3) * 0.4 * H, np.arange(3) * 0.4 * H, indexing="ij"), -1).reshape(-1, 2)
    bridge = np.stack([0.8 * H + 0.5 * H * np.arange(1, 12), np.full(11, 0.4 * H)], 1)      # from 0.5 H right of one blob to 0.5 H left of the other
    pos = 0.5 + np.concatenate([blob, bridge, blob + [0.8 * H + 6.0 * H, 0.0]])
    p = _cloud(p0, len(pos), pos)
    p.Type[...] = [1] * 9 + [2] * 11 + [1] * 9
    p.Velocity[...] = 0
    eng = _engine(p, s, fb)
    assert eng.advance(1e9, max_steps=1).iteration == 1
    got, d, pairs = _check(eng, f"types fp{8 * fb} Fluid", None, FLUID)
    assert len(got["count"]) == 2 and got["count"].tolist() == [9, 9]
    assert (got["label"][np.asarray(d["Type"]) == 2] == -1).all() and (got["label"] == -1).sum() == 11
    both, _, _ = _check(eng, f"types fp{8 * fb} Fluid + Fixed", None, ("Fluid", "Fixed"), d, pairs)
    assert both["count"].tolist() == [29] and (both["label"] == 0).all()
    only, _, _ = _check(eng, f"types fp{8 * fb} Fixed", None, FIXED, d, pairs)
    assert only["count"].tolist() == [11]
    eng.close()


# ---- 5. the cut ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fb", [8, 4])
def test_the_cut_is_inclusive_and_exact(fb, request):
    """A lattice on multiples of 2^-5: every difference and every square is exact, r^2 of lattice neighbours is link^2 itself."""
    p0, s = request.getfixturevalue("dam_break_2d")
    a = 2.0 ** -5
    assert a <= s.SimKernel.H
    pos = 0.5 + a * np.stack(np.meshgrid(np.arange(20), np.arange(20), indexing="ij"), -1).reshape(-1, 2).astype(np.float64)
    eng = _engine(_cloud(p0, len(pos), pos, walls=True), s, fb)
    assert eng.advance(1e9, max_steps=1).iteration == 1
    got, d, _ = _check(eng, f"lattice fp{8 * fb} link 2^-5", a, FIXED)
    assert (np.asarray(d["Position"], np.float64) * 32.0 % 1.0 == 0).all()                  # the lattice came back on its multiples of 2^-5
    assert got["count"].tolist() == [400]
    below, _, _ = _check(eng, f"lattice fp{8 * fb} link just below", float(np.nextafter(a, 0.0)), FIXED, d)
    assert below["count"].tolist() == [1] * 400 and below["first_row"].tolist() == list(range(400)) and below["label"].tolist() == list(range(400))
    eng.close()


# ---- 6. run edges --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fb", [8, 4])
@pytest.mark.parametrize("rows", [1, 255, 256, 257, 513])
def test_run_edges(rows, fb, request):
    p0, s = request.getfixturevalue("dam_break_2d")
    assert len(p0) > rows
    eng = _engine(_cloud(p0, rows), s, fb)
    assert eng.advance(1e9, max_steps=1).iteration == 1
    got, d, _ = _check(eng, f"{rows} rows fp{8 * fb}", None, ALL)
    assert got["count"].sum() == rows
    if rows == 1:
        x = np.asarray(d["Position"], np.float64)[0]
        assert got["label"].tolist() == [0] and got["first_row"].tolist() == [0] and got["count"].tolist() == [1]
        assert got["box"].tolist() == [[x[0], x[1], 0.0, x[0], x[1], 0.0]]
        assert eng.components_build() in ((1, 0), (1, 1))                           # (the fluid alone: the row may be a wall)
        lab, first, cnt, box = eng.components_read(first_row=False, count=False, box=False)      # NULL pointers
        assert first is None and cnt is None and box is None and len(lab) == 1
        assert eng.components_read(label=False)[0] is None
    eng.close()


# ---- 7. the same bytes, no side effects ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fb", [8, 4])
def test_repeats_and_does_not_disturb(fb, request):
    p, s = _state("dam_break_2d", request)
    markers = sorted(int(m) for m in np.unique(p.GroupMarker))
    Fl = p.Position[p.Type == 1]
    probes = np.array([Fl.mean(0), Fl.min(0) + 0.05, Fl.max(0) - 0.05])
    short = 1.2 * s.SimConstants.dx
    same = lambda a, b: all(x.tobytes() == y.tobytes() for x, y in zip(a, b))      # noqa: E731
    runs = []
    for called in (False, True):
        eng = _engine(p, s, fb)
        eng.group_forces_enable(markers, capacity=64)
        eng.probes_enable(probes, capacity=64)
        prog = []
        for _ in range(8):
            q = eng.advance(1e9, max_steps=5)
            prog.append((q.iteration, q.steps_done, q.n_rebuilds, q.index_counter, q.total_time, q.last_dt, q.delta_x))
            if called:
                eng.components_build(short, ALL)
                a = eng.components_read()
                eng.components_build(short, ALL)                                   # no step in between: the same bytes
                b = eng.components_read()
                assert same(a, b) and same(eng.components_read(), a)               # … and a second read of one build
        runs.append((prog, eng.download(), eng.group_forces_read(), eng.probes_read()))
        if called:
            # a download begun before a build completes with the snapshot taken at its begin
            want = eng.download()
            spec = {k: np.zeros_like(want[k]) for k in ("Position", "Velocity", "Acceleration", "Density", "Pressure", "ID", "Type", "GroupMarker", "GhostPoints", "Cells")}
            fbeg = eng._fn("download_begin"); fbeg.argtypes = [C.c_void_p] * 11
            eng._check(fbeg(eng._h, *[spec[k].ctypes.data_as(C.c_void_p) for k in spec]))
            eng.components_build(short, ALL)
            mid = eng.components_read()
            eng.download_end()
            for k in spec:
                np.testing.assert_array_equal(spec[k], want[k], err_msg=k)
            assert same(mid, a)
            # a neighbour list built before a components build still reads back unchanged: the arenas are separate
            eng.neighbors_build()
            nl = eng.neighbors_read()
            eng.components_build(None, FLUID)
            assert same(eng.neighbors_read(), nl)
            assert not same(eng.components_read()[:1], a[:1])                      # (another selection, another result)
            eng.neighbors_build(half=True)                                         # … and the other way round
            assert same(eng.components_read(), eng.components_read())
            eng.neighbors_release()
            eng.components_release()
        eng.close()
    assert runs[0][0][-1][0] == 40 and runs[0][0] == runs[1][0]                    # the progress blocks, n_rebuilds among them
    for k, v in runs[0][1].items():
        assert runs[1][1][k].tobytes() == v.tobytes(), k                            # the final download, byte for byte
    for a, b in zip(runs[0][2], runs[1][2]):
        np.testing.assert_array_equal(a, b)                                         # the group-force series
    assert len(runs[0][3]["iteration"]) == 40
    for k in runs[0][3]:
        np.testing.assert_array_equal(runs[1][3][k], runs[0][3][k], err_msg=k)      # the probe series


# ---- 8. lifetime and errors --------------------------------------------------------------------------------------------------------------------
def test_lifetime(request):
    p, s = _state("dam_break_2d", request)
    eng = _engine(p, s, 8)
    _refused(eng.components_read, ERR_STATE, "no components")                      # before any build (and before any step)
    assert eng.advance(1e9, max_steps=3).iteration == 3
    _refused(eng.components_read, ERR_STATE, "no components")
    n_rows, n_comp = eng.components_build()
    lab, first, cnt, box = eng.components_read()
    assert len(lab) == n_rows and len(first) == len(cnt) == len(box) == n_comp > 0
    assert eng.advance(1e9, max_steps=1).steps_done == 1
    _refused(eng.components_read, ERR_STATE, "stale")                              # rows may have moved
    assert eng.components_build()[0] == n_rows                                     # a new build after a stale result serves again
    _check(eng, "after a stale result", None, FLUID)
    eng.forces_once()
    _refused(eng.components_read, ERR_STATE, "stale")
    assert eng.advance(1e9, max_steps=1).steps_done == 1
    eng.components_build()
    eng.upload_particles(p)                                                        # a new particle set
    _refused(eng.components_read, ERR_STATE, "stale")
    _refused(eng.components_build, ERR_STATE, "has not executed a step")
    _refused(eng.components_read, ERR_STATE, "")                                   # (a refused build leaves nothing to read)
    assert eng.advance(1e9, max_steps=2).steps_done == 2
    eng.components_build()
    eng.components_release()
    _refused(eng.components_read, ERR_STATE, "no components")                      # after release
    eng.components_release()                                                       # releasing nothing is legal
    assert eng.components_build()[1] == len(eng.components_read()[1])
    assert eng.advance(1e9, max_steps=1).steps_done == 1
    eng.close()


def test_errors(request):
    from sphexample_amd._abi import make_config
    from sphexample_amd.engine import Engine
    p, s = _state("dam_break_2d", request)
    cfg = make_config(len(p), s.SimConstants, s.SimKernel, s.SimMetaData, s.SimViscosity, s.SimDensityDiffusion, device_float_bytes=8, host_float_bytes=8)
    bare = Engine(cfg)
    _refused(bare.components_build, ERR_STATE, "before sphmi_upload")
    bare.upload_particles(p)
    _refused(bare.components_build, ERR_STATE, "has not executed a step")          # uploaded, no step yet: no cell list
    assert bare.advance(1e9, max_steps=3).iteration == 3                            # the handle still advances …
    f = bare._fn("components_build")
    f.argtypes = [C.c_void_p, C.c_double, C.c_uint32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    rows, comps = C.c_int64(), C.c_int64()
    H = cfg.H
    for link in (0.0, -H, float("nan"), float("inf"), float(np.nextafter(H, 1.0)), 2 * H):
        _refused(lambda: bare._check(f(bare._h, link, 2, C.byref(rows), C.byref(comps))), ERR_ARGUMENT, "link")
        assert bare.advance(1e9, max_steps=1).steps_done == 1
    for mask in (0, 1, 1 << 4, 0b1111, 0b10010, 1 << 31):
        _refused(lambda: bare._check(f(bare._h, H, mask, C.byref(rows), C.byref(comps))), ERR_ARGUMENT, "type mask")
    assert bare.advance(1e9, max_steps=1).steps_done == 1
    _refused(lambda: bare._check(f(bare._h, H, 2, C.byref(rows), None)), ERR_ARGUMENT, "null n_components_out")
    bare._check(f(bare._h, H, 2, None, C.byref(comps)))                            # n_rows_out may be NULL
    with pytest.raises(RuntimeError, match="did not build"):                       # the wrapper sizes its arrays from its OWN build: it
        bare.components_read()                                                     # refuses a result built behind its back, and writes nothing
    assert comps.value > 0 and bare.components_build() == (len(p), comps.value)     # … and serves
    assert bare.advance(1e9, max_steps=1).steps_done == 1
    bare.close()
    slabs = _engine(p, s, 8, devices=[0, 0])                                       # two slabs on one GPU
    _refused(slabs.components_build, ERR_STATE, "single-device")
    slabs.advance(1e9, max_steps=3)
    _refused(slabs.components_build, ERR_STATE, "single-device")                   # … with a cell list too
    _refused(slabs.components_read, ERR_STATE, "no components")
    slabs.components_release()
    assert slabs.advance(1e9, max_steps=2).steps_done == 2
    slabs.close()
    thin = _engine(p, _variant(s, None, 0.9), 8)                                   # H < h
    _refused(thin.components_build, ERR_STATE, "H < h")
    assert thin.advance(1e9, max_steps=1).steps_done == 1
    _refused(thin.components_build, ERR_STATE, "H < h")
    assert thin.advance(1e9, max_steps=2).steps_done == 2
    thin.close()


def test_errors_rank_mode(request):
    """A rank-mode handle holds one slab of the rows per process: refused like a multi-device handle, and it goes on advancing.
    (Its own test: bringing up the communicator of a rank-mode handle takes most of the time.)"""
    p, s = _state("dam_break_2d", request)
    from sphexample_amd.engine import rccl_unique_id
    rk = _engine(p, s, 8, rank=0, world=1, unique_id=rccl_unique_id())
    for _ in range(2):                                                             # before the first step, and with a cell list
        with pytest.raises(SphmiError) as ei:
            rk.components_build()
        assert ei.value.status == ERR_STATE and "single-device" in str(ei.value) and "rank-mode" in str(ei.value), str(ei.value)
        _refused(rk.components_read, ERR_STATE, "no components")
        rk.components_release()
        assert rk.advance(1e9, max_steps=2).steps_done == 2                         # the handle still advances
    rk.close()


# ---- 9. agrees with the neighbour list -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fb", [8, 4])
def test_agrees_with_the_neighbour_list(fb, request):
    p, s = _state("dam_break_2d", request)
    eng = _engine(p, s, fb)
    assert eng.advance(1e9, max_steps=30).iteration == 30
    link = 1.2 * s.SimConstants.dx
    got = eng.components(link, FLUID)
    off, nbr = eng.neighbor_list(half=True)
    d = eng.download(("Position", "Type"))
    X, sel = np.asarray(d["Position"], np.float64), _selected(d["Type"], FLUID)
    i, j = neighbors.pairs(off, nbr)
    dx, dy = X[i, 0] - X[j, 0], X[i, 1] - X[j, 1]
    keep = (dx * dx + dy * dy <= link * link) & sel[i] & sel[j]
    root = _union_find(len(X), i[keep], j[keep], sel)
    firsts = np.unique(root[sel])
    label = np.where(sel, np.searchsorted(firsts, root), -1).astype(np.int32)
    print(f"fp{8 * fb}: {int(keep.sum())} of {len(nbr)} pairs are links, {len(firsts)} components")
    np.testing.assert_array_equal(got["label"], label)
    np.testing.assert_array_equal(got["first_row"], firsts.astype(np.int32))
    eng.close()
