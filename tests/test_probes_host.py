"""Host side of the probes (sphmi_probes_enable / sphmi_probes_read): the prototypes, the gauge helpers of
sphexample_amd/probes.py, and the brute-force reference tests/test_probes_gpu.py holds the device against.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sphexample_amd import _abi
from sphexample_amd.probes import gauge_column, water_level
from test_probes_gpu import brute_force_probes, kernel_w

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CTYPES = {"sphmi_handle*": C.c_void_p, "int32_t": C.c_int32, "int64_t": C.c_int64, "const double*": C.c_void_p, "double*": C.c_void_p,
          "int64_t*": (C.c_void_p, C.POINTER(C.c_int64))}


def _prototype(name):
    text = open(os.path.join(ROOT, "include", "sphmi.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, re.S)
    assert m, f"{name} is not declared in include/sphmi.h"
    args = []
    for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(","):
        a = " ".join(a.split())
        star = "*" if "*" in a else ""
        args.append(" ".join(a.replace("*", " ").split()[:-1]) + star)
    return args


class _Recorder:
    """Stands in for the library: remembers the argtypes a Backend method sets and answers OK."""
    def __init__(self):
        self.fns = {}

    def __getattr__(self, name):
        if name.startswith("sphmi_"):
            fn = self.fns.setdefault(name, _Fn())
            return fn
        raise AttributeError(name)


class _Fn:
    argtypes = None

    def __call__(self, *a):
        return _abi.OK


def _backend():
    b = _abi.Backend.__new__(_abi.Backend)
    b._lib, b._p, b._h, b.N, b.D = _Recorder(), "sphmi_", C.c_void_p(), 10, 3
    return b


def test_header_and_abi_prototypes_agree():
    text = open(os.path.join(ROOT, "include", "sphmi.h")).read()
    assert int(re.search(r"#define SPHMI_MAX_PROBES (\d+)", text).group(1)) == _abi.MAX_PROBES == 1024
    assert int(re.search(r"#define SPHMI_ABI_VERSION (\d+)", text).group(1)) == _abi.ABI_VERSION == 5
    b = _backend()
    b.probes_enable(np.zeros((4, 3)), capacity=8)
    b.probes_read()
    for name, want_n in (("sphmi_probes_enable", 4), ("sphmi_probes_read", 12)):
        proto, got = _prototype(name), b._lib.fns[name].argtypes
        assert len(proto) == len(got) == want_n, (name, proto, got)
        for k, (c_type, py_type) in enumerate(zip(proto, got)):
            allowed = CTYPES[c_type]
            assert py_type in (allowed if isinstance(allowed, tuple) else (allowed,)), (name, k, c_type, py_type)
    assert _prototype("sphmi_probes_read") == ["sphmi_handle*", "int64_t", "int64_t*", "double*", "double*", "double*", "int64_t*",
                                               "double*", "double*", "double*", "int64_t*", "int64_t*"]
    # the shapes the binding hands out
    out = _backend()
    out.probes_enable(np.zeros((5, 3)))
    r = out.probes_read()
    assert r["weight"].shape == (0, 5) and r["velocity"].shape == (0, 5, 3) and r["count"].dtype == np.int64


def test_gauge_column():
    g = gauge_column([0.5, 0.1, 0.0], [0.5, 0.1, 0.4], 0.05)
    assert g.shape == (9, 3) and np.allclose(g[:, 2], np.arange(9) * 0.05) and (g[:, :2] == [0.5, 0.1]).all()
    g = gauge_column([1.0, 0.0], [1.0, 0.33], 0.1)                       # the spacing closes up so that both ends are probes
    assert g.shape == (5, 2) and g[0, 1] == 0.0 and g[-1, 1] == 0.33 and np.allclose(np.diff(g[:, 1]), 0.0825)
    for bad in (lambda: gauge_column([0, 0], [0, 0], 0.1), lambda: gauge_column([0, 0], [0, 1], 0.0), lambda: gauge_column([0, 0], [0, 0, 1], 0.1)):
        with pytest.raises(ValueError):
            bad()


def test_water_level_on_synthetic_profiles():
    z = np.linspace(0.0, 1.0, 11)
    assert water_level(z, np.zeros(11)) == 0.0                                            # dry: the base
    assert water_level(z, np.full(11, 0.3)) == 0.0                                        # … spray everywhere below the threshold too
    assert water_level(z, np.ones(11)) == 1.0                                             # submerged: the top
    assert water_level(z, np.r_[np.zeros(10), 0.5]) == 1.0                                # … decided by the top probe alone
    S = np.where(z <= 0.4, 1.0, 0.0)                                                      # one crossing between 0.4 and 0.5
    assert water_level(z, S) == pytest.approx(0.45)
    S = np.clip(1.0 - (z - 0.3) / 0.2, 0.0, 1.0)                                          # a linear ramp 1 → 0 over [0.3, 0.5]: ½ at 0.4
    assert water_level(z, S) == pytest.approx(0.4)
    assert water_level(z, S, threshold=0.25) == pytest.approx(0.45)
    S = np.array([1, 1, 1, 0, 0, 1, 1, 0.2, 0, 0, 0], dtype=float)                        # several crossings: the topmost counts
    assert water_level(z, S) == pytest.approx(0.6 + 0.1 * (1 - 0.5) / (1 - 0.2))
    S = np.array([0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0], dtype=float)                          # a dry base under a blob
    assert water_level(z, S) == pytest.approx(0.35)
    both = water_level(z, np.stack([np.zeros(11), np.ones(11), np.where(z <= 0.4, 1.0, 0.0)]))
    assert both.shape == (3,) and both[0] == 0.0 and both[1] == 1.0 and both[2] == pytest.approx(0.45)
    for bad in (lambda: water_level(z[::-1], np.zeros(11)), lambda: water_level(z, np.zeros(10)), lambda: water_level(z[:1], np.zeros(1))):
        with pytest.raises(ValueError):
            bad()


class _Cfg:
    pass


@pytest.mark.parametrize("dims", [2, 3])
@pytest.mark.parametrize("kernel", [0, 1])
def test_brute_force_reproduces_a_closed_form(dims, kernel):
    """Shepard interpolation is exact for a linear field wherever the neighbourhood is symmetric about the probe: on a node of
    a uniform lattice of Fluid rows of equal density, with P(x) = a + b·x, SP / S = P(x_p), Sv / S = v(x_p), Sρ / S = ρ —
    and S = (m0/ρ) Σ W is the lattice sum, which the test forms on its own from the node offsets."""
    dp, h = 0.1, 0.13                                                  # (H² / dp² = 6.76: no lattice distance sits at the cut)
    H = 2 * h
    cfg = _Cfg()
    cfg.h, cfg.h_inv, cfg.H, cfg.H2, cfg.kernel, cfg.m0 = h, 1 / h, H, H * H, kernel, 1000 * dp ** dims
    cfg.alphaD = {(0, 2): 7 / (4 * np.pi * h ** 2), (0, 3): 21 / (16 * np.pi * h ** 3), (1, 2): 10 / (7 * np.pi * h ** 2), (1, 3): 1 / (np.pi * h ** 3)}[(kernel, dims)]
    ax = np.arange(-6, 7) * dp
    pos = np.stack(np.meshgrid(*[ax] * dims, indexing="ij"), -1).reshape(-1, dims)
    b = np.array([3.0, -2.0, 0.5])[:dims]
    press = 7.0 + pos @ b
    vel = np.stack([1.0 + pos @ b, 2.0 - pos[:, 0], 0.25 * pos[:, -1]], 1)[:, :dims]
    rho = np.full(len(pos), 1000.0)
    typ = np.ones(len(pos), dtype=np.uint8)
    probes = np.array([[0.0] * dims, [dp, -2 * dp, dp][:dims], [0.37, 3.0, 0.0][:dims]])           # two nodes, and one far outside
    r = brute_force_probes(cfg, probes, pos, vel, rho, press, typ)
    for k in (0, 1):
        xp = probes[k]
        assert r["n"][k] > 0
        assert r["SP"][k] / r["S"][k] == pytest.approx(7.0 + xp @ b, rel=1e-12)
        assert r["Srho"][k] / r["S"][k] == pytest.approx(1000.0, rel=1e-13)
        assert r["Sv"][k, 0] / r["S"][k] == pytest.approx(1.0 + xp @ b, rel=1e-12)
        assert r["Sv"][k, 1] / r["S"][k] == pytest.approx(2.0 - xp[0], rel=1e-12)
        if dims == 2:
            assert r["Sv"][k, 2] == 0.0
        # the lattice sum, from the offsets of the nodes within H (the inclusive cut)
        off = np.stack(np.meshgrid(*[np.arange(-3, 4)] * dims, indexing="ij"), -1).reshape(-1, dims) * dp
        rr = np.sqrt((off ** 2).sum(1))
        rr = rr[rr ** 2 <= H * H]
        assert r["n"][k] == len(rr)
        assert r["S"][k] == pytest.approx(cfg.m0 / 1000.0 * kernel_w(cfg, rr / h).sum(), rel=1e-12)
        assert 0.9 < r["S"][k] < 1.1                                                     # a partition of unity, to the lattice's accuracy
    assert r["n"][2] == 0 and r["S"][2] == 0 and r["SP"][2] == 0                         # empty space
    # Fixed rows do not count, and r = 0 is legal: the probe on a particle sees that particle
    typ2 = typ.copy(); typ2[np.abs(pos).sum(1) < 1e-12] = 2
    r2 = brute_force_probes(cfg, probes[:1], pos, vel, rho, press, typ2)
    assert r2["n"][0] == r["n"][0] - 1
    assert r["S"][0] - r2["S"][0] == pytest.approx(cfg.m0 / 1000.0 * cfg.alphaD, rel=1e-10)          # W(0) = αD for both kernels
