"""Host side of the row selection (sphmi_select_build / _read / _download* / _release, csrc/sphmi_select.h): the plain C++ predicate
the device runs — compiled for the host under the sanitizers and run as a child process — against `selection.restate`, `restate`
against a row-by-row loop on the 2-D dam-break fixture, the prototypes, the export and the binding, the RunSimulation plumbing with
a stand-in backend, and what the built code object says about the new kernels.  No GPU.

    a row is selected iff every enabled clause holds; the boxes are ORed; lo <= x < hi; field_lo <= value <= field_hi; NaN never
"""
import copy
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from sphexample_amd import _abi, selection
from sphexample_amd.selection import Selection, every, restate, slab, where
from test_field_grid_host import _backend, _header, _prototype, _StandIn
from test_step_series_host import CSRC, SANITIZE, host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "host_select", "select_main.cpp")
INF, NAN = float("inf"), float("nan")


# ---- 1. the plain C++ part against selection.py -----------------------------------------------------------------------------------
def edge_rows(dims):
    """Rows made to sit on every edge of the rule: coordinates ON lo and ON hi of the box [0.25, 0.75) x [-0.0, 1.0) (x [2, 3)), one
    ulp to either side, -0.0 and +0.0, NaN positions, NaN field values, all three Types and a Type that is none, IDs 0 … and a
    negative one."""
    rng = np.random.default_rng(5)
    xs = [0.25, np.nextafter(0.25, 0), np.nextafter(0.25, 1), 0.75, np.nextafter(0.75, 0), np.nextafter(0.75, 1), -0.0, 0.0, NAN, 0.5, -INF, INF]
    ys = [-0.0, 0.0, np.nextafter(0.0, -1), 1.0, np.nextafter(1.0, 0), 0.5, NAN]
    zs = [2.0, 3.0, np.nextafter(3.0, 0), 2.5, NAN] if dims == 3 else [0.0]
    pos = np.array([(x, y, z) for x in xs for y in ys for z in zs], dtype=np.float64)
    n = len(pos)
    vel = rng.uniform(-2, 2, (n, 3))
    vel[::7, 0] = NAN
    vel[3::11] = [-0.0, 0.0, -0.0]
    vel[5::13] = [0.5, -0.5, 0.25]                                                  # SPEED2 = 0.5 + 0.0625 (3-D), 0.5 (2-D): exactly on a bound below
    rho = rng.uniform(990, 1010, n)
    rho[::5] = 1000.0
    rho[2::9] = NAN
    press = rng.uniform(-50, 500, n)
    press[1::6] = -0.0
    press[4::10] = NAN
    typ = rng.integers(1, 4, n).astype(np.uint8)
    typ[::17] = 0
    typ[8::19] = 4
    ids = np.arange(n, dtype=np.int64) * 3 + 1
    ids[-1] = -5
    grp = rng.integers(1, 5, n).astype(np.uint64)
    grp[::23] = np.uint64(2 ** 63 + 7)
    fields = {"Position": np.ascontiguousarray(pos[:, :dims]), "Velocity": np.ascontiguousarray(vel[:, :dims]), "Density": rho, "Pressure": press,
              "Type": typ, "ID": ids, "GroupMarker": grp}
    return fields, pos, vel


def specs(dims, n, ids):
    box = lambda *b: (np.array(b[:dims], dtype=np.float64), np.array(b[3:3 + dims], dtype=np.float64))          # noqa: E731
    the_box = box(0.25, -0.0, 2.0, 0.75, 1.0, 3.0)
    rng = np.random.default_rng(9)
    some = rng.integers(0, 2, n).astype(np.uint8) * 3
    out = {
        "everything": Selection(),
        "fluid": Selection(types=("Fluid",)),
        "fixed_and_moving": Selection(types=("Fixed", 3)),
        "half_open_box": Selection(boxes=(the_box,)),
        "infinite_box": Selection(boxes=(box(-INF, -INF, -INF, INF, INF, INF),)),
        "half_infinite": Selection(boxes=(box(-INF, 0.0, -INF, 0.25, INF, INF),)),
        "empty_box": Selection(boxes=(box(0.75, 0.0, 2.0, 0.25, 1.0, 3.0),)),        # lo > hi on x
        "point_box": Selection(boxes=(box(0.5, 0.5, 2.5, 0.5, 0.5, 2.5),)),          # lo == hi: half-open, holds nothing
        "union": Selection(boxes=(the_box, box(-INF, 0.5, -INF, 0.0, INF, INF), box(0.75, 0.0, 2.0, 0.25, 1.0, 3.0))),
        "markers": Selection(markers=(2, 2 ** 63 + 7)),
        "stride_1": Selection(id_stride=1),
        "stride_2": Selection(id_stride=2, id_phase=1),
        "stride_7": Selection(id_stride=7, id_phase=3),
        "stride_beyond": Selection(id_stride=int(ids.max()) + 10, id_phase=4),       # larger than every ID: ID == phase alone (and the negative one, mod 2^64)
        "density": Selection(field="Density", field_lo=1000.0, field_hi=1000.0),
        "pressure": Selection(field="Pressure", field_lo=0.0, field_hi=INF),           # -0.0 is kept: 0.0 <= -0.0
        "pressure_below": Selection(field="Pressure", field_lo=-INF, field_hi=-0.0),
        "speed2": Selection(field="Speed2", field_lo=0.0, field_hi=0.5625 if dims == 3 else 0.5),
        "speed2_empty": Selection(field="Speed2", field_lo=1.0, field_hi=0.5),
        "mask_zeros": where(np.zeros(n, dtype=np.uint8)),
        "mask_ones": where(np.ones(n, dtype=bool)),
        "mask_some": where(some),
        "all_clauses": Selection(types=("Fluid", "Moving"), boxes=(the_box, box(-INF, -INF, -INF, 0.3, INF, INF)), markers=(1, 2, 3), id_stride=2,
                                 id_phase=0, field="Speed2", field_lo=0.0, field_hi=6.0, mask=some),
    }
    return out


def case_text(spec, dims, fields, pos, vel):
    n = len(pos)
    lo, hi = spec.box_tables(dims)
    pad = lambda a: [float(v) for v in a] + [0.0] * (3 - dims)                        # noqa: E731
    m = spec.mask_bytes(n)
    h = lambda v: float(v).hex() if math.isfinite(v) else repr(float(v))              # noqa: E731
    lines = [f"case {spec.type_mask()} {dims} {len(lo)} {len(spec.markers)} {spec.id_stride} {spec.id_phase} {spec.field_code()} "
             f"{h(spec.field_lo)} {h(spec.field_hi)} {0 if m is None else 1} {n}"]
    for b in range(len(lo)):
        lines.append("box " + " ".join(h(v) for v in pad(lo[b]) + pad(hi[b])))
    lines += [f"marker {int(k)}" for k in spec.markers]
    for i in range(n):
        lines.append(f"row {int(fields['Type'][i])} " + " ".join(h(v) for v in (*pos[i], *vel[i], fields["Density"][i], fields["Pressure"][i]))
                     + f" {int(fields['ID'][i])} {int(fields['GroupMarker'][i])} {0 if m is None else int(m[i])}")
    return "\n".join(lines) + "\n"


def test_the_host_program_and_the_restatement_agree_exactly(tmp_path):
    main = [ln.split()[1] for ln in open(MAIN).read().splitlines() if ln.startswith("#include")]
    assert [i for i in main if i.startswith('"')] == ['"sphmi_select.h"']
    cxx = host_compiler()
    exe = str(tmp_path / "select_main")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I", CSRC, MAIN, "-o", exe]
    for extra in (SANITIZE + ("-static-libasan", "-static-libubsan"), SANITIZE, ()):
        built = subprocess.run(base + list(extra), capture_output=True, text=True)
        if built.returncode == 0:
            break
    assert built.returncode == 0, built.stderr
    print("sanitizers:", " ".join(extra) or "none")
    text, want, names = "", [], []
    for dims in (2, 3):
        fields, pos, vel = edge_rows(dims)
        for name, spec in specs(dims, len(pos), fields["ID"]).items():
            text += case_text(spec, dims, fields, pos, vel)
            want.append(restate(spec, fields))
            names.append((dims, name))
    run = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and not run.stderr.strip(), run.stdout[-2000:] + run.stderr
    lines = run.stdout.strip().splitlines()
    assert lines[-1] == "ok" and len(lines) == len(want) + 1
    counts = {}
    for (dims, name), ln, rows in zip(names, lines, want):
        w = ln.split()
        assert w[0] == "kept" and int(w[1]) == len(w) - 2, ln
        got = np.array(w[2:], dtype=np.int32)
        assert rows.dtype == np.int32 and np.array_equal(got, rows), (dims, name, got, rows)
        counts[(dims, name)] = len(rows)
    print(counts)
    for dims in (2, 3):
        n = len(edge_rows(dims)[1])
        c = lambda name: counts[(dims, name)]                                       # noqa: E731
        assert c("empty_box") == c("point_box") == c("mask_zeros") == c("speed2_empty") == 0
        assert c("mask_ones") == c("everything") == c("stride_1") and 0 < c("infinite_box") < c("everything")      # NaN and +inf lie in no box
        assert 0 < c("half_open_box") < c("union") < c("everything") < n             # rows of Type 0 and 4 are never kept
        assert 0 < c("stride_7") < c("stride_2") < c("everything") and c("stride_beyond") == 1
        assert 0 < c("density") and 0 < c("speed2") and 0 < c("pressure_below") and c("pressure") + c("pressure_below") > c("everything") * 0.8
        assert 0 < c("all_clauses") < c("fluid")


def test_the_edges_of_the_rule_one_by_one():
    """The half-open box, the inclusive field bounds, -0.0 and NaN, stated on single rows."""
    def one(spec, **row):
        f = {"Position": np.array([[0.5, 0.5]]), "Velocity": np.array([[0.0, 0.0]]), "Density": np.array([1000.0]), "Pressure": np.array([0.0]),
             "Type": np.array([1], np.uint8), "ID": np.array([10], np.int64), "GroupMarker": np.array([2], np.uint64)}
        f.update({k: np.array([v]) for k, v in row.items()})
        return len(restate(spec, f)) == 1
    b = Selection(boxes=((np.array([0.25, 0.0]), np.array([0.75, 1.0])),))
    assert one(b, Position=[0.25, 0.0]) and not one(b, Position=[0.75, 0.5]) and not one(b, Position=[0.5, 1.0])      # lo is inside, hi is not
    assert one(b, Position=[0.25, -0.0]) and not one(b, Position=[np.nextafter(0.25, 0), 0.5]) and not one(b, Position=[NAN, 0.5])
    assert one(slab(1, 0.5, 0.25), Position=[1e300, 0.375]) and not one(slab(1, 0.5, 0.25), Position=[0.0, 0.625])
    d = Selection(field="Density", field_lo=1000.0, field_hi=1001.0)
    assert one(d, Density=1000.0) and one(d, Density=1001.0) and not one(d, Density=np.nextafter(1001.0, 2000)) and not one(d, Density=NAN)
    assert one(Selection(field="Pressure", field_lo=0.0), Pressure=-0.0) and not one(Selection(field="Pressure", field_lo=-INF, field_hi=INF), Pressure=NAN)
    s2 = Selection(field="Speed2", field_lo=25.0, field_hi=25.0)
    assert one(s2, Velocity=[3.0, -4.0]) and not one(s2, Velocity=[3.0, np.nextafter(4.0, 5)])
    v = np.array([[0.1, 0.2, 0.3]])
    assert selection.speed2(v)[0] == (0.1 * 0.1 + 0.2 * 0.2) + 0.3 * 0.3 and selection.speed2(v[:, :2])[0] == 0.1 * 0.1 + 0.2 * 0.2
    assert one(every(5), ID=10) and not one(every(5, 1), ID=10) and one(every(3), ID=-1) and not one(every(3, 2), ID=-1)      # uint64(-1) = 2^64 - 1 = 3 · 6148914691236517205, not -1 mod 3 = 2
    assert one(Selection(markers=(2,))) and not one(Selection(markers=(1, 3)))
    assert not one(Selection(types=("Fixed",))) and one(Selection(types=(1,))) and not one(Selection(), Type=np.uint8(0))
    assert Selection(types=("Fluid",)).type_mask() == 1 and Selection(types=("Fixed", "Moving")).type_mask() == 6 and Selection().type_mask() == 7
    assert one(where([7])) and not one(where([0])) and one(where(np.array([True])))


# ---- 2. restate on the fixture against a row-by-row loop ----------------------------------------------------------------------------
def test_restate_on_the_fixture_against_a_row_loop():
    from conftest import load_dam_break_2d, perturbed
    p, s = load_dam_break_2d()
    p = perturbed(p, seed=3, vel_scale=3.0)
    n = len(p)
    assert n == 6881
    rng = np.random.default_rng(2)
    f = {"Position": p.Position.astype(np.float64), "Velocity": p.Velocity.astype(np.float64), "Density": p.Density.astype(np.float64),
         "Pressure": rng.uniform(-100, 3000, n), "Type": p.Type.astype(np.uint8), "ID": p.ID.astype(np.int64), "GroupMarker": p.GroupMarker.astype(np.uint64)}
    H = s.SimKernel.H
    mask = rng.integers(0, 2, n).astype(np.uint8)
    x_edge = float(np.sort(f["Position"][:, 0])[n // 2])                                # a coordinate a row sits on
    spec = Selection(types=("Fluid", "Fixed"), boxes=((np.array([x_edge, -INF]), np.array([x_edge + 20 * H, 0.5])), (np.array([0.0, 0.0]), np.array([0.2, 0.2]))),
                     markers=(1, 2), id_stride=3, id_phase=1, field="Speed2", field_lo=0.0, field_hi=9.0, mask=mask)
    for sp in (spec, slab(0, x_edge + H / 2, H, dims=2), every(8), Selection(field="Pressure", field_lo=1500.0), Selection(types=("Fixed",))):
        lo, hi = sp.box_tables(2)
        want = []
        for i in range(n):
            t = int(f["Type"][i])
            if not (1 <= t <= 3 and (sp.type_mask() >> (t - 1)) & 1):
                continue
            x, y = float(f["Position"][i, 0]), float(f["Position"][i, 1])
            if len(lo) and not any(lo[b, 0] <= x < hi[b, 0] and lo[b, 1] <= y < hi[b, 1] for b in range(len(lo))):
                continue
            if len(sp.markers) and int(f["GroupMarker"][i]) not in sp.markers:
                continue
            if sp.id_stride > 1 and (int(f["ID"][i]) % 2 ** 64) % sp.id_stride != sp.id_phase:
                continue
            if sp.field == "Speed2":
                vx, vy = float(f["Velocity"][i, 0]), float(f["Velocity"][i, 1])
                val = (vx * vx + vy * vy) + 0.0
            elif sp.field is not None:
                val = float(f[sp.field][i])
            if sp.field is not None and not (sp.field_lo <= val <= sp.field_hi):
                continue
            if sp.mask is not None and not sp.mask[i]:
                continue
            want.append(i)
        got = restate(sp, f)
        assert got.dtype == np.int32 and got.tolist() == want and 0 < len(want) < n, (sp, len(want))
    assert spec.type_mask() == 3 and (f["Position"][restate(slab(0, x_edge + H / 2, H, dims=2), f), 0] >= x_edge).all()


# ---- 3. the prototypes, the export and the binding -------------------------------------------------------------------------------------
def test_header_library_and_binding_agree():
    text = _header()
    assert re.search(r"#define\s+SPHMI_ABI_VERSION\s+5\b", text) and _abi.ABI_VERSION == 5      # append-only: the version stays
    assert re.search(r"enum\s*\{\s*SPHMI_SELECT_FIELD_NONE\s*=\s*0\s*,\s*SPHMI_SELECT_FIELD_DENSITY\s*,\s*SPHMI_SELECT_FIELD_PRESSURE\s*,\s*SPHMI_SELECT_FIELD_SPEED2\s*\}", text)
    assert (_abi.SELECT_FIELD_NONE, _abi.SELECT_FIELD_DENSITY, _abi.SELECT_FIELD_PRESSURE, _abi.SELECT_FIELD_SPEED2) == (0, 1, 2, 3)
    assert selection.FIELDS == {None: 0, "Density": 1, "Pressure": 2, "Speed2": 3}
    for name, value in (("SPHMI_MAX_SELECT_BOXES", _abi.MAX_SELECT_BOXES), ("SPHMI_MAX_SELECT_MARKERS", _abi.MAX_SELECT_MARKERS)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1)) == value == 16
    assert _prototype("sphmi_select_build") == ["sphmi_handle*", "const sphmi_selection*", "int64_t*", "int64_t*"]
    assert _prototype("sphmi_select_read") == ["sphmi_handle*", "int32_t*"]
    assert _prototype("sphmi_select_download") == _prototype("sphmi_download")
    assert _prototype("sphmi_select_download_columns") == _prototype("sphmi_download_columns")
    assert _prototype("sphmi_select_release") == ["sphmi_handle*"]
    # the struct, member for member
    m = re.search(r"typedef\s+struct\s+sphmi_selection\s*\{(.*?)\}\s*sphmi_selection\s*;", re.sub(r"/\*.*?\*/", " ", text, flags=re.S), flags=re.S)
    members = []
    for decl in m.group(1).split(";"):
        w = decl.replace("*", " * ").replace("const", " ").split()
        if w:
            members += [(name.strip(), w[0] + ("*" if "*" in w else "")) for name in " ".join(w[1:]).replace("*", "").split(",")]
    ctype = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}
    assert [(k, t) for k, t in _abi.SphmiSelection._fields_] == [(k, C.c_void_p if t.endswith("*") else ctype[t]) for k, t in members]
    assert [k for k, _ in members] == ["type_mask", "n_boxes", "box_lo", "box_hi", "n_markers", "markers", "id_stride", "id_phase", "field", "field_lo",
                                       "field_hi", "row_mask"]
    assert C.sizeof(_abi.SphmiSelection) == 88
    # the binding: what travels
    b = _backend(2)
    b._ft = np.float64
    assert b.has_select()
    mask = np.zeros(10, dtype=bool)
    mask[3] = True
    spec = Selection(types=("Fluid", "Moving"), boxes=(([0.0, -INF], [1.0, 2.0]),), markers=(2, 5), id_stride=8, id_phase=3, field="Speed2", field_lo=0.5,
                     field_hi=4.0, mask=mask)
    seen = {}
    fns = b._lib.fns

    def build(h, sel, rows, kept):
        s = C.cast(sel, C.POINTER(_abi.SphmiSelection)).contents
        seen.update(type_mask=s.type_mask, n_boxes=s.n_boxes, n_markers=s.n_markers, stride=s.id_stride, phase=s.id_phase, field=s.field, lo=s.field_lo,
                    hi=s.field_hi, box_lo=np.ctypeslib.as_array(C.cast(s.box_lo, C.POINTER(C.c_double)), (2,)).copy(),
                    box_hi=np.ctypeslib.as_array(C.cast(s.box_hi, C.POINTER(C.c_double)), (2,)).copy(),
                    markers=np.ctypeslib.as_array(C.cast(s.markers, C.POINTER(C.c_uint64)), (2,)).copy(),
                    mask=np.ctypeslib.as_array(C.cast(s.row_mask, C.POINTER(C.c_uint8)), (10,)).copy())
        rows._obj.value, kept._obj.value = 10, 4
        return _abi.OK
    build.argtypes = None
    fns["sphmi_select_build"] = build
    b._column_widths = [4, 33]
    rows, got, cols = b.select(spec, fields=("Position", "ID", "Type"), columns=True, components=3)
    assert seen["type_mask"] == 5 and seen["n_boxes"] == 1 and seen["n_markers"] == 2 and (seen["stride"], seen["phase"]) == (8, 3)
    assert seen["field"] == 3 and (seen["lo"], seen["hi"]) == (0.5, 4.0) and seen["box_lo"].tolist() == [0.0, -INF] and seen["box_hi"].tolist() == [1.0, 2.0]
    assert seen["markers"].tolist() == [2, 5] and seen["mask"].tolist() == [0, 0, 0, 1, 0, 0, 0, 0, 0, 0]
    assert build.argtypes == [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    assert rows.dtype == np.int32 and rows.shape == (4,)
    assert set(got) == {"Position", "ID", "Type"} and got["Position"].shape == (4, 3) and got["ID"].dtype == np.int64 and got["Type"].shape == (4,)
    assert [c.shape for c in cols] == [(4, 4), (4, 33)] and all(c.dtype == np.uint8 for c in cols)
    dl = fns["sphmi_select_download"].calls[0]
    assert len(dl) == 11 and [a is not None for a in dl[1:]] == [True, False, False, False, False, True, True, False, False, False]
    assert [c[1] for c in fns["sphmi_set_output_components"].calls] == [3, 2]          # padded for the call, put back after it
    assert [len(fns[f"sphmi_select_{k}"].calls) for k in ("read", "download", "download_columns", "release")] == [1, 1, 1, 1]
    assert fns["sphmi_select_download"].argtypes == [C.c_void_p] * 11 and fns["sphmi_select_read"].argtypes == [C.c_void_p] * 2
    # after the release this object holds nothing: a read asks the library (which words the refusal) and then refuses itself
    with pytest.raises(RuntimeError, match="did not build"):
        b.select_read()
    with pytest.raises(RuntimeError, match="did not build"):
        b.select_download()
    with pytest.raises(ValueError, match="one entry per row"):
        b.select_build(where(np.zeros(9)))
    with pytest.raises(ValueError, match="unknown type"):
        b.select_build(Selection(types=("Water",)))
    with pytest.raises(ValueError, match="unknown field"):
        b.select_build(Selection(field="Speed"))


def test_the_julia_shim_binds_the_symbols():
    import test_julia_shim as tj
    calls = {c[0]: c for c in tj.shim_ccalls()}
    assert {"sphmi_select_build", "sphmi_select_read", "sphmi_select_download", "sphmi_select_release"} <= set(calls)
    assert "function select_rows(P;" in tj.shim_text()
    body = re.search(r"struct\s+SphmiSelection\b(.*?)\nend", tj.shim_text(), flags=re.S).group(1)
    jl = re.findall(r"(\w+)::([\w{}]+)", body)
    width = {"UInt32": C.c_uint32, "Int32": C.c_int32, "Int64": C.c_int64, "Float64": C.c_double}
    assert [(k, C.c_void_p if t.startswith("Ptr{") else width[t]) for k, t in jl] == list(_abi.SphmiSelection._fields_)


# ---- 4. RunSimulation -----------------------------------------------------------------------------------------------------------------
class _SelectStandIn(_StandIn):
    def select(self, spec, fields=None):
        self.log.append(("select", self.iteration))
        return np.array([1, 4], dtype=np.int32) + self.iteration, {"spec": spec, "fields": fields}

    def neighbor_list(self, half=False):
        self.log.append(("neighbor_list", self.iteration))
        return np.array([0, 1, 2], dtype=np.int64), np.array([1, 0], dtype=np.int32)


def test_run_simulation_hands_the_subset_to_the_callback():
    from conftest import load_dam_break_2d
    from sphexample_amd import simulation
    p, s = load_dam_break_2d()

    def run(**kw):
        meta = copy.deepcopy(s.SimMetaData)
        meta.SimulationTime, meta.OutputTimes = 0.002, 0.001
        got = []
        _StandIn.instances.clear()
        steps = simulation.RunSimulation(SimGeometry=None, SimMetaData=meta, SimConstants=s.SimConstants, SimKernel=s.SimKernel, SimLogger=None,
                                         SimParticles=p.copy(), SimViscosity=s.SimViscosity, SimDensityDiffusion=s.SimDensityDiffusion,
                                         backend_factory=_SelectStandIn, on_output=lambda m, pp, *extra: got.append((m.Iteration, extra)), **kw)
        return steps, got, _StandIn.instances[0]

    spec = every(8)
    steps, got, eng = run(output_select=spec)
    assert len(got) == len(steps) + 1 >= 3
    for iteration, extra in got:                                                    # the first call too: a selection needs no step
        assert len(extra) == 1
        rows, d = extra[0]
        assert rows.tolist() == [1 + iteration, 4 + iteration] and d["spec"] is spec and d["fields"] is None      # taken on the rows of THIS output
    seq = [e for e in eng.log if isinstance(e, tuple)]
    assert [e[0] for e in seq] == ["select"] + ["advance", "select", "download"] * len(steps)      # no step between the selection and the download
    # with the fields named, behind the neighbour list, whose plumbing is as it was
    _, got2, eng2 = run(neighbor_list=True, output_select=(spec, ("Position",)))
    assert all(len(extra) == 2 for _, extra in got2) and got2[0][1][0] is None and got2[0][1][1][1]["fields"] == ("Position",)
    assert got2[1][1][0][0].tolist() == [0, 1, 2] and got2[1][1][1][1]["spec"] is spec
    assert [e[0] for e in eng2.log if isinstance(e, tuple)][:5] == ["select", "advance", "neighbor_list", "select", "download"]
    # without the keyword the callback keeps its arguments and nothing is selected
    _, got3, eng3 = run()
    assert all(extra == () for _, extra in got3) and not any(e[0] == "select" for e in eng3.log if isinstance(e, tuple))


# ---- 5. the library --------------------------------------------------------------------------------------------------------------------
def test_the_kernels_are_built_for_gfx950_without_scratch(tmp_path):
    """The library exports the five entry points; the code object's metadata — read the way tests/test_bench_contract.py reads it —
    shows every new kernel without scratch: k_sel_flag<float | double>, k_sel_fill, the four k_pack_selected<T, H> and
    k_gather_selected_columns, next to the k_pack_output and k_gather_columns they share their bodies with."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_report
    from sphexample_amd import build
    lib = build.build()
    dll = C.CDLL(lib)
    assert all(hasattr(dll, f"sphmi_select_{k}") for k in ("build", "read", "download", "download_columns", "release"))
    co = isa_report.code_object(lib, str(tmp_path))
    meta = isa_report.metadata(co)
    names = isa_report.demangle(list(meta))
    for kernel, count in (("k_sel_flag<", 2), ("k_sel_fill(", 1), ("k_pack_selected<", 4), ("k_gather_selected_columns(", 1), ("k_pack_output<", 4),
                          ("k_gather_columns(", 1)):
        mine = {names[k]: v for k, v in meta.items() if kernel in names[k]}
        assert len(mine) == count, (kernel, sorted(mine))
        for d, v in mine.items():
            print(d.split("(")[0], v)
            assert v["scratch_bytes"] == 0, (d, v)
            assert v["max_flat_workgroup_size"] == 256, (d, v)
    flag = [v for k, v in meta.items() if "k_sel_flag<" in names[k]]
    assert all(v["lds_bytes"] == 0 and v["vgprs"] + v["agprs"] <= 64 for v in flag), flag      # a streaming pass: eight waves per SIMD
