"""CPU-side checks of the per-bin maps (sphmi_maps_enable / sphmi_maps_read / sphmi_maps_disable): `sphexample_amd.maps.update` against
an independent per-row Python loop on random clouds (rows on bin edges and on the outer faces, a collapsed axis with rows below the
origin, NaN positions, non-finite velocities, an empty step); the integer images round-trip and the int64 sums do not depend on the
row order; the header's index and record arithmetic, compiled for the host with the address and undefined-behaviour sanitizers
(tests/host_maps/maps_main.cpp, a program of its own), agrees with `maps.update` bit for bit on a dumped case; the three prototypes
are declared with the arity the bindings use, exported, wrapped and bound by the Julia shim; the ABI version stays 5."""
import ctypes as C
import inspect
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from test_step_series_host import CSRC, SANITIZE, host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "host_maps", "maps_main.cpp")
SYMBOLS = {"sphmi_maps_enable": 5, "sphmi_maps_disable": 1, "sphmi_maps_read": 17}
WINDOW = ["steps", "t_begin", "t_end", "duration"]
FIELDS = ["top_max", "t_top_max", "bottom_min", "t_arrival", "wet", "fill", "flux", "speed2_max", "t_speed2_max", "n_max"]
LAST = ["last_n", "last_top", "last_bottom", "last_velocity_sum"]
INF, NAN = np.inf, np.nan


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---- an independent restatement: one row at a time, Python floats and ints, struct for the bit patterns ---------------------------
def _image(x):
    b = struct.unpack("<Q", struct.pack("<d", x))[0]
    return b ^ 0xFFFFFFFFFFFFFFFF if b >> 63 else b | (1 << 63)


def _value(u):
    b = u & ~(1 << 63) if u >> 63 else u ^ 0xFFFFFFFFFFFFFFFF
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def _div(a, b):
    """IEEE division of two Python floats (Python raises where IEEE answers)"""
    return float(np.float64(a) / np.float64(b))


def loop_start(lat, t_begin=0.0):
    B = lat["bins"]
    rec = [[-INF, 0.0, INF, INF, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0] for _ in range(B)]
    return {"rec": rec, "steps": 0, "t_begin": t_begin, "t_end": t_begin, "duration": 0.0, "last": None, "bins": B}


def loop_update(st, lat, position, velocity, is_fluid, t, dt):
    B, dims = st["bins"], len(lat["origin"])
    n, top, bottom, S = [0] * B, [0] * B, [(1 << 64) - 1] * B, [[0, 0, 0] for _ in range(B)]
    for x, v, fluid in zip(position, velocity, is_fluid):
        if not fluid or not all(math.isfinite(c) for c in v):
            continue
        k = []
        for d in range(dims):
            with np.errstate(invalid="ignore"):
                q = _div(float(x[d]) - float(lat["origin"][d]), float(lat["spacing"][d]))
            if math.isnan(q):
                break
            q = math.floor(q) if math.isfinite(q) else q
            if not (0.0 <= q < float(lat["counts"][d])):
                break
            k.append(int(q))
        if len(k) < dims:
            continue
        b, stride = 0, 1
        for d in range(dims):
            b += stride * k[d]
            stride *= int(lat["counts"][d])
        im = _image(float(x[lat["up_axis"]]))
        n[b] += 1
        top[b], bottom[b] = max(top[b], im), min(bottom[b], im)
        for d in range(len(v)):
            S[b][d] += round(float(v[d]) * 4294967296.0)          # Python's round(): half to even, an int
    for b in range(B):
        if not n[b]:
            continue
        r = st["rec"][b]
        tp, bt, nd = _value(top[b]), _value(bottom[b]), float(n[b])
        if tp > r[0]:
            r[0], r[1] = tp, t
        if bt < r[2]:
            r[2] = bt
        if r[3] == INF:
            r[3] = t
        r[4] = r[4] + dt
        r[5] = r[5] + nd * dt
        sd = [float(s) * 2.0 ** -32 for s in S[b]]
        for d in range(3):
            r[6 + d] = r[6 + d] + sd[d] * dt
        u = [s / nd for s in sd]
        s2 = (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]
        if s2 > r[9]:
            r[9], r[10] = s2, t
        if nd > r[11]:
            r[11] = nd
    st["steps"] += 1
    st["t_end"] = t
    st["duration"] = st["duration"] + dt
    st["last"] = (n, [_value(top[b]) if n[b] else -INF for b in range(B)], [_value(bottom[b]) if n[b] else INF for b in range(B)],
                  [[float(s) * 2.0 ** -32 for s in S[b]] for b in range(B)])


def loop_result(st):
    rec = np.array(st["rec"], dtype=np.float64).reshape(st["bins"], 12)
    out = {k: st[k] for k in WINDOW}
    for k, slot in (("top_max", 0), ("t_top_max", 1), ("bottom_min", 2), ("t_arrival", 3), ("wet", 4), ("fill", 5), ("speed2_max", 9), ("t_speed2_max", 10),
                    ("n_max", 11)):
        out[k] = rec[:, slot].copy()
    out["flux"] = rec[:, 6:9].copy()
    n, top, bottom, sd = st["last"]
    out.update(last_n=np.array(n, dtype=np.int64), last_top=np.array(top), last_bottom=np.array(bottom), last_velocity_sum=np.array(sd, dtype=np.float64).reshape(-1, 3))
    return out


def assert_same(got, want, label):
    for k in WINDOW:
        assert _bits([got[k]])[0] == _bits([want[k]])[0] if k != "steps" else got[k] == want[k], (label, k, got[k], want[k])
    for k in FIELDS + LAST:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape, (label, k, a.shape, b.shape)
        if k == "last_n":
            assert a.dtype == np.int64 and np.array_equal(a, b), (label, k)
        else:
            bad = np.nonzero(_bits(a).reshape(-1) != _bits(b).reshape(-1))[0]
            assert len(bad) == 0, (label, k, len(bad), a.reshape(-1)[bad[:3]], b.reshape(-1)[bad[:3]])


# ---- the clouds --------------------------------------------------------------------------------------------------------------------
def cloud(rng, lat, n, dims):
    """n rows around the lattice: most inside, some outside every face, some EXACTLY on bin edges and on the outer faces, some with a
    NaN or infinite coordinate, some with a non-finite velocity, some that are no fluid"""
    o, c = lat["origin"], lat["counts"]
    s = np.where(np.isfinite(lat["spacing"]), lat["spacing"], 1.0)
    span = s * c
    x = o + rng.uniform(-0.25, 1.25, (n, dims)) * span
    edge = rng.random(n) < 0.25                                   # exactly origin + k · spacing on one axis, k = 0 … counts (both faces)
    for i in np.nonzero(edge)[0]:
        d = rng.integers(dims)
        x[i, d] = o[d] + float(rng.integers(0, c[d] + 1)) * s[d]
    v = rng.normal(0.0, 2.0, (n, dims))
    v[rng.random(n) < 0.05] *= 1e-12                              # near the unit of the fixed-point image
    half = rng.random(n) < 0.1
    v[half, 0] = (rng.integers(-8, 8, int(half.sum())) + 0.5) / 4294967296.0        # exact ties: half to even
    fluid = rng.random(n) < 0.8
    for i in np.nonzero(rng.random(n) < 0.04)[0]:
        x[i, rng.integers(dims)] = [NAN, INF, -INF][rng.integers(3)]
    for i in np.nonzero(rng.random(n) < 0.04)[0]:
        v[i, rng.integers(dims)] = [NAN, INF, -INF][rng.integers(3)]
    return x, v, fluid


LATTICES = {
    "2-D column map": (2, ([0.125, -0.5], [0.0625, INF], [9, 1], 1)),
    "2-D full, up = x": (2, ([-1.0, 0.25], [0.3, 0.07], [5, 7], 0)),
    "3-D floor map": (3, ([0.0, -0.25, 0.5], [0.1, 0.05, INF], [6, 5, 1], 2)),
    "3-D full, up = y": (3, ([0.1, 0.2, -0.3], [0.11, 0.13, 0.17], [4, 3, 5], 1)),
    "one bin": (3, ([0.0, 0.0, 0.0], [INF, INF, INF], [1, 1, 1], 2)),
}


@pytest.mark.parametrize("name", list(LATTICES))
def test_update_against_a_per_row_loop(name):
    from sphexample_amd import maps
    dims, (origin, spacing, counts, up) = LATTICES[name]
    lat = maps.lattice(origin, spacing, counts, up)
    rng = np.random.default_rng(sum(map(ord, name)))
    st, ref = maps.start(lat, t_begin=0.5), loop_start(lat, 0.5)
    t = 0.5
    moved = False
    for step in range(6):
        n = 0 if step == 3 else 150                               # an empty step: the window moves on, every bin is dry
        x, v, fluid = cloud(rng, lat, n, dims)
        if name.endswith("column map") or name.endswith("floor map") or name == "one bin":
            x[: n // 3, -1] = lat["origin"][-1] - rng.uniform(0.0, 3.0, n // 3)      # below the origin of the collapsed axis: −0, inside
            x[: n // 3, -1][rng.random(n // 3) < 0.2] = -0.0
        dt = float(rng.uniform(1e-5, 3e-5))
        t = t + dt
        assert maps.update(st, lat, x, v, fluid, t, dt) is st
        loop_update(ref, lat, x, v, fluid, t, dt)
        moved = moved or int(st["last_n"].sum()) > 0
        assert_same(maps.result(st), loop_result(ref), f"{name}, step {step}")
        if step == 3:
            assert int(st["last_n"].sum()) == 0 and (st["last_top"] == -INF).all() and (st["last_bottom"] == INF).all() and not st["last_velocity_sum"].any()
    assert moved and st["steps"] == 6
    r = maps.result(st)
    assert list(r) == WINDOW + FIELDS + LAST
    wet = r["t_arrival"] < INF
    assert wet.any() and (r["wet"][wet] > 0).all() and (r["wet"][~wet] == 0).all() and (r["top_max"][wet] >= r["bottom_min"][wet]).all()
    assert (r["top_max"][~wet] == -INF).all() and (r["n_max"][~wet] == 0).all()


def test_the_edge_rule_and_the_collapsed_axis():
    from sphexample_amd import maps
    lat = maps.lattice([0.25, -1.0, 0.0], [0.5, 0.25, INF], [4, 8, 1], 2)
    x = [[0.25, -1.0, 0.0], [0.75, -1.0, 5.0], [0.7499999999999999, -1.0, 5.0], [2.25, -1.0, 0.0], [0.25, 1.0, 0.0], [2.2499999999999996, 0.99, 0.0],
         [0.2499999999999999, 0.0, 0.0], [1.0, 0.0, -7.0], [1.0, 0.0, -1e300], [NAN, 0.0, 0.0], [1.0, 0.0, NAN], [1.0, 0.0, INF], [1.0, 0.0, -INF], [-INF, 0.0, 0.0]]
    np.testing.assert_array_equal(maps.bin_index(lat, x), [0, 1, 0, -1, -1, 31, -1, 17, 17, -1, -1, -1, -1, -1])
    # a 2-D lattice reads two coordinates
    lat2 = maps.lattice([0.0, 0.0], [1.0, INF], [3, 1])
    assert lat2["up_axis"] == 1 and lat2["bins"] == 3
    np.testing.assert_array_equal(maps.bin_index(lat2, [[0.5, -4.0], [2.999, 1e9], [3.0, 0.0], [-0.0, -0.0]]), [0, 2, -1, 0])
    with pytest.raises(ValueError):
        maps.lattice([0.0], [1.0], [1])
    with pytest.raises(ValueError):
        maps.lattice([0.0, 0.0], [1.0, 1.0], [1, 1], 2)


def test_the_images_round_trip_and_the_sums_ignore_the_row_order():
    from sphexample_amd import maps
    v = np.array([-INF, -1e300, -2.5, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, 2.5, 1e300, INF])
    im = maps.image(v)
    assert im.dtype == np.uint64 and (np.diff(im.astype(object)) > 0).all()                  # strictly increasing: −0 below +0
    assert (_bits(maps.value(im)) == _bits(v)).all()
    assert [int(u) for u in im] == [_image(float(x)) for x in v] and [_value(int(u)) for u in im[1:-1]] == [float(x) for x in v[1:-1]]
    rng = np.random.default_rng(5)
    w = rng.normal(0.0, 1e3, 4000) * 10.0 ** rng.integers(-12, 3, 4000)
    assert (_bits(maps.value(maps.image(w))) == _bits(w)).all()
    assert (np.argsort(maps.image(w), kind="stable") == np.argsort(w, kind="stable")).all()
    # the fixed-point image: half to even, an exact inverse on what it produced
    np.testing.assert_array_equal(maps.fixed(np.array([1.0, -1.0, 0.5, 1.5, 2.5, -0.5, -1.5]) * np.array([1, 1] + [2.0 ** -32] * 5)), [1 << 32, -(1 << 32), 0, 2, 2, 0, -2])
    f = maps.fixed(w[np.abs(w) < 1e5])
    assert (maps.fixed(f.astype(np.float64) * 2.0 ** -32) == f).all()
    # a shuffled input gives equal bits — and a float sum of the same rows would not
    lat = maps.lattice([0.0, 0.0, 0.0], [0.5, INF, INF], [2, 1, 1], 2)
    n = 5000
    x = rng.uniform(0.0, 1.0, (n, 3))
    vel = rng.normal(0.0, 3.0, (n, 3)) * 10.0 ** rng.integers(-6, 2, (n, 1))
    fluid = np.ones(n, dtype=bool)
    a = maps.update(maps.start(lat), lat, x, vel, fluid, 0.1, 0.1)
    floats_differ = False
    for seed in range(3):
        p = np.random.default_rng(seed).permutation(n)
        b = maps.update(maps.start(lat), lat, x[p], vel[p], fluid[p], 0.1, 0.1)
        assert_same(maps.result(b), maps.result(a), f"shuffle {seed}")
        floats_differ = floats_differ or np.add.reduce(vel[p][:, 0]) != np.add.reduce(vel[:, 0]) or float(sum(vel[p][:, 0])) != float(sum(vel[:, 0]))
    assert floats_differ                                         # (what the integer sums are for)
    assert int(a["last_n"].sum()) == n


def test_the_host_program_under_the_sanitizers_agrees_bit_for_bit(tmp_path):
    """maps_main.cpp includes sphmi_maps.h alone, is built with the sanitizers as a program of its own and run as a child process — no
    sanitizer is loaded into python — first its self checks, then a dumped case against `maps.update`."""
    from sphexample_amd import maps
    main = [ln.split()[1] for ln in open(MAIN).read().splitlines() if ln.startswith("#include")]
    assert [i for i in main if i.startswith('"')] == ['"sphmi_maps.h"']
    cxx = host_compiler()
    exe = str(tmp_path / "maps_main")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I", CSRC, MAIN, "-o", exe]
    for extra in (SANITIZE + ("-static-libasan", "-static-libubsan"), SANITIZE, ()):
        built = subprocess.run(base + list(extra), capture_output=True, text=True)
        if built.returncode == 0:
            break
    assert built.returncode == 0, built.stderr
    print("sanitizers:", " ".join(extra) or "none")
    for name in ("3-D floor map", "3-D full, up = y", "2-D column map"):
        dims, (origin, spacing, counts, up) = LATTICES[name]
        lat = maps.lattice(origin, spacing, counts, up)
        rng = np.random.default_rng(41 + dims)
        st, t = maps.start(lat, t_begin=0.25), 0.25
        pad = lambda a, fill: list(a) + [fill] * (3 - dims)      # noqa: E731
        blob = [struct.pack("<3d3d3qqdq", *pad(origin, 0.0), *pad(spacing, INF), *pad(counts, 1), up, 0.25, 5)]
        for step in range(5):
            n = 0 if step == 2 else 257
            x, v, fluid = cloud(rng, lat, n, dims)
            x[: n // 4, -1] = lat["origin"][-1] - rng.uniform(0.0, 2.0, n // 4) if not np.isfinite(lat["spacing"][-1]) else x[: n // 4, -1]
            dt = float(rng.uniform(1e-5, 3e-5))
            t = t + dt
            maps.update(st, lat, x, v, fluid, t, dt)
            rows = np.zeros((n, 7))
            rows[:, :dims], rows[:, 3:3 + dims], rows[:, 6] = x, v, fluid
            blob.append(struct.pack("<ddq", t, dt, n) + rows.tobytes())
        src, dst = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
        with open(src, "wb") as f:
            f.write(b"".join(blob))
        run = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=60)
        assert run.returncode == 0, run.stdout + run.stderr
        assert run.stdout.strip().splitlines()[-1] == "ok", run.stdout
        assert not run.stderr.strip(), run.stderr               # a sanitizer report would be here
        B = lat["bins"]
        raw = np.fromfile(dst, dtype=np.float64)
        assert len(raw) == 12 * B + 4 + 6 * B
        rec, header, last = raw[:12 * B].reshape(12, B), raw[12 * B:12 * B + 4], raw[12 * B + 4:]
        got = {"steps": int(header[:1].view(np.int64)[0]), "t_begin": header[1], "t_end": header[2], "duration": header[3]}
        for k, slot in (("top_max", 0), ("t_top_max", 1), ("bottom_min", 2), ("t_arrival", 3), ("wet", 4), ("fill", 5), ("speed2_max", 9), ("t_speed2_max", 10),
                        ("n_max", 11)):
            got[k] = rec[slot]
        got["flux"] = rec[6:9].T
        got.update(last_n=last[:B].view(np.int64), last_top=last[B:2 * B], last_bottom=last[2 * B:3 * B], last_velocity_sum=last[3 * B:].reshape(B, 3))
        assert_same(got, maps.result(st), name)
        assert got["steps"] == 5 and (got["t_arrival"] < INF).any()


def test_the_derived_quantities():
    from sphexample_amd import maps
    lat = maps.lattice([0.0, 0.0, 0.0], [0.5, 0.25, INF], [2, 2, 1], 2)
    m = {"steps": 4, "t_begin": 1.0, "t_end": 3.0, "duration": 2.0,
         "top_max": np.array([0.5, -INF, 1.0, 0.25]), "bottom_min": np.array([0.0, INF, 0.5, 0.25]), "t_arrival": np.array([1.5, INF, 3.0, 1.0]),
         "fill": np.array([8.0, 0.0, 2.0, 1.0]), "flux": np.array([[4.0, 0.0, -8.0], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0.0, 0.5, 0.0]]),
         "speed2_max": np.array([4.0, 0.0, 9.0, 0.25]), "last_top": np.array([0.25, -INF, -INF, 0.25]), "last_bottom": np.array([0.0, INF, INF, 0.25])}
    assert maps.crest(lat, m).shape == (2, 2, 1)                 # [k0, k1, k2], the collapsed axis included
    crest = maps.crest(lat, m)[..., 0]
    assert crest[0, 0] == 0.5 and np.isnan(crest[1, 0]) and crest[0, 1] == 1.0 and crest[1, 1] == 0.25      # [k0, k1]: x fastest
    np.testing.assert_array_equal(maps.depth(lat, m, 0.125)[..., 0], [[0.625, 0.625], [0.0, 0.125]])
    np.testing.assert_array_equal(maps.depth(lat, m, 0.125, last=True)[..., 0], [[0.375, 0.0], [0.0, 0.125]])
    np.testing.assert_array_equal(maps.mean_depth(lat, m, m0=0.5, rho0=1000.0)[..., 0], np.array([[8.0, 2.0], [0.0, 1.0]]) * 0.5 / 1000.0 / (0.125 * 2.0))
    assert maps.mean_velocity(lat, m).shape == (2, 2, 1, 3)
    mv = maps.mean_velocity(lat, m)[:, :, 0]
    np.testing.assert_array_equal(mv[0, 0], [0.5, 0.0, -1.0])
    np.testing.assert_array_equal(mv[1, 0], [0.0, 0.0, 0.0])
    np.testing.assert_array_equal(mv[1, 1], [0.0, 0.5, 0.0])
    np.testing.assert_array_equal(maps.max_speed(lat, m)[..., 0], [[2.0, 3.0], [0.0, 0.5]])
    arrival = maps.arrival_map(lat, m)[..., 0]
    assert arrival[0, 0] == 0.5 and np.isnan(arrival[1, 0]) and arrival[0, 1] == 2.0 and arrival[1, 1] == 0.0


def test_the_entry_points_are_declared_and_exported():
    from test_julia_shim import c_class, c_prototypes
    from sphexample_amd.engine import load_library
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sphmi.h")).read(), flags=re.S)
    protos = c_prototypes()
    lib = load_library()
    for s, arity in SYMBOLS.items():
        assert s in protos, f"{s} is not declared in include/sphmi.h"
        assert protos[s][0] == "int" and len(protos[s][1]) == arity, protos[s]
        assert hasattr(lib, s), f"libsphmi.so does not export {s}"
    assert [c_class(a) for a in protos["sphmi_maps_enable"][1]] == ["ptr"] * 4 + ["i4"]
    assert [c_class(a) for a in protos["sphmi_maps_read"][1]] == ["ptr"] * 17
    assert re.search(r"#define\s+SPHMI_MAX_MAP_BINS\s+\(1 << 20\)", text)
    assert re.search(r"#define\s+SPHMI_ABI_VERSION\s+5\b", text)             # additions only: the version stays, as for the envelopes


def test_the_ctypes_wrappers_bind_them_with_the_header_arity():
    from sphexample_amd import _abi
    seen = []

    class Fn:
        def __init__(self, name):
            self.name, self.argtypes = name, None

        def __call__(self, *args):
            seen.append((self.name, len(self.argtypes), len(args)))
            if self.name == "x_maps_enable":
                seen.append(tuple(np.ctypeslib.as_array((C.c_int64 * 2).from_address(args[3].value))) + (args[4],))
            if self.name == "x_maps_read":
                args[1]._obj.value = 7
                np.ctypeslib.as_array((C.c_double * 3).from_address(args[2].value))[:] = [0.5, 2.0, 1.5]
                np.ctypeslib.as_array((C.c_double * 18).from_address(args[9].value))[:] = np.arange(18.0)        # flux: the seventh array
                np.ctypeslib.as_array((C.c_int64 * 6).from_address(args[13].value))[:] = np.arange(6)            # last_n
            return 0

    class Lib:
        def __init__(self):
            self.fns = {n: Fn(n) for n in ("x_maps_enable", "x_maps_read", "x_maps_disable")}

        def __getattr__(self, n):
            try:
                return self.__dict__["fns"][n]
            except KeyError:
                raise AttributeError(n)

    b = _abi.Backend.__new__(_abi.Backend)
    b._lib, b._p, b._h, b.D, b.N = Lib(), "x_", None, 2, 5
    assert b.has_maps()
    assert inspect.signature(_abi.Backend.maps_enable).parameters["up_axis"].default is None
    b.maps_enable([0.0, 0.0], [0.5, INF], [6, 1])
    out = b.maps_read()
    b.maps_enable([0.0, 0.0], [0.5, 0.5], [2, 3], up_axis=0)
    b.maps_disable()
    assert seen == [("x_maps_enable", 5, 5), (6, 1, 1), ("x_maps_read", 17, 17), ("x_maps_enable", 5, 5), (2, 3, 0), ("x_maps_disable", 1, 1)]
    assert list(out) == WINDOW + FIELDS + LAST
    assert out["steps"] == 7 and (out["t_begin"], out["t_end"], out["duration"]) == (0.5, 2.0, 1.5)
    for k in FIELDS + LAST:
        assert out[k].shape == ((6, 3) if k in ("flux", "last_velocity_sum") else (6,)), k
        assert out[k].dtype == (np.int64 if k == "last_n" else np.float64), k
    np.testing.assert_array_equal(out["flux"], np.arange(18.0).reshape(6, 3))
    np.testing.assert_array_equal(out["last_n"], np.arange(6))
    with pytest.raises(ValueError):
        b.maps_enable([0.0, 0.0, 0.0], [0.5, 0.5, 0.5], [2, 3, 1])          # the handle's dims


def test_the_julia_shim_binds_the_calls_behind_an_opt_in():
    from test_julia_shim import shim_ccalls
    called = [c[0] for c in shim_ccalls()]
    assert called.count("sphmi_maps_enable") == 1 and called.count("sphmi_maps_read") == 1 and called.count("sphmi_maps_disable") == 1
    shim = open(os.path.join(ROOT, "julia", "SPHExampleMI355X.jl")).read()
    assert 'ENV, "SPHMI_MAPS", ""' in shim                       # unset: no enable, no read
    assert "haskey(MAPS, P) && read_maps!" in shim
    assert "function maps_enable(" in shim and "function maps_read(" in shim and "function maps_disable(" in shim


def test_the_kernels_use_integer_atomics_only_and_no_scratch(tmp_path):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_report
    from sphexample_amd import build
    text = open(os.path.join(ROOT, "sphexample_amd", "csrc", "sphmi_maps.h")).read()
    code = text.split("#pragma once", 1)[1]
    assert "sqrt" not in code and "SPHMI_NO_CONTRACT" in code and "#pragma clang fp contract(off)" in code
    lib = build.build()
    co = isa_report.code_object(lib, str(tmp_path))
    meta, isa = isa_report.metadata(co), isa_report.kernels(co)
    names = isa_report.demangle(list(meta))
    for kernel, variants in (("k_mp_bin", 2), ("k_mp_fold", 1), ("k_mp_fill", 1)):
        mine = [k for k, d in names.items() if re.search(r"\b%s\b" % kernel, d)]
        assert len(mine) == variants, (kernel, mine)             # k_mp_bin: fp32 and fp64 handles
        for k in mine:
            assert meta[k]["scratch_bytes"] == 0 and meta[k]["lds_bytes"] == 0, kernel
            assert meta[k]["vgprs"] <= 64, (kernel, meta[k]["vgprs"])
            atomics = [ln for ln in isa[k] if "atomic" in ln]
            assert not [ln for ln in atomics if re.search(r"atomic_\w*(f16|f32|f64|pk)", ln)], (kernel, atomics)      # no float atomic anywhere
            assert bool(atomics) == (kernel == "k_mp_bin"), (kernel, atomics)
            assert not [ln for ln in isa[k] if re.search(r"v_sqrt|v_rsq", ln)], kernel


def test_run_simulation_default_keeps_the_callback(dam_break_2d):
    """maps=None: the oracle-backed driver (which has no such entry points) runs as before and calls back with two arguments."""
    import copy
    from oracle.oracle import Oracle
    from sphexample_amd import simulation
    assert inspect.signature(simulation.RunSimulation).parameters["maps"].default is None
    p, s = dam_break_2d
    meta = copy.deepcopy(s.SimMetaData)
    meta.SimulationTime, meta.OutputTimes = 0.0004, 0.0002
    shapes = []
    simulation.RunSimulation(SimGeometry=None, SimMetaData=meta, SimConstants=s.SimConstants, SimKernel=s.SimKernel, SimLogger=None,
                             SimParticles=p.copy(), SimViscosity=s.SimViscosity, SimDensityDiffusion=s.SimDensityDiffusion, backend_factory=Oracle,
                             on_output=lambda *a: shapes.append(len(a)))
    assert len(shapes) >= 2 and set(shapes) == {2}
