"""The ctypes prototype table of sphexample_amd/_abi.py (PROTOTYPES, applied by `bind` / `Backend._fn`) against the headers: every
entry has the arity and the argument classes include/sphmi.h and include/sphmi_internal.h declare, every entry point the package and
the tools call is in the table, nothing outside _abi.py declares a prototype, `_fn` re-applies the table on every lookup, and a
handle-less call that fails reports the library's text.  No GPU, no library."""
import ctypes as C
import glob
import os
import re

import pytest

import test_julia_shim as tj
from sphexample_amd import _abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what may stand for a C argument that is no pointer (a pointer: see admissible())
SCALARS = {"int64_t": C.c_int64, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "int": C.c_int, "double": C.c_double}
POINTEES = {"int64_t": C.c_int64, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "uint8_t": C.c_uint8, "int": C.c_int,
            "double": C.c_double, "sphmi_config": _abi.SphmiConfig, "sphmi_progress": _abi.SphmiProgress, "sphmi_multi_info": _abi.SphmiMultiInfo,
            "char*": C.c_char_p, "void*": C.c_void_p, "sphmi_handle*": C.c_void_p}


def admissible(decl):
    """The ctypes types that may stand for the C argument `decl` ("const double* lo", "int32_t n", "sphmi_handle** out")."""
    words = decl.replace("*", " * ").replace("const", " ").split()
    if words[-1] != "*":
        words = words[:-1]                                   # the argument's name
    base, stars = words[0], words.count("*")
    if stars == 0:
        return {SCALARS[base]}
    ok = {C.c_void_p, C.c_char_p}                            # any pointer may travel untyped
    pointee = POINTEES.get(base if stars == 1 else base + "*" * (stars - 1))
    if pointee is not None:
        ok.add(C.POINTER(pointee))
    return ok


def header_prototypes(monkeypatch):
    protos = dict(tj.c_prototypes())                         # include/sphmi.h
    monkeypatch.setattr(tj, "HEADER", os.path.join(ROOT, "include", "sphmi_internal.h"))
    protos.update(tj.c_prototypes())
    return protos


def split(proto):
    return proto if isinstance(proto, tuple) else (proto, C.c_int)


def test_every_entry_agrees_with_the_headers(monkeypatch):
    protos = header_prototypes(monkeypatch)
    assert {"sphmi_create", "sphmi_cast_rays", "sphmi_plan_slabs", "sphmi_multi_halo_info"} <= set(protos)
    for name, proto in _abi.PROTOTYPES.items():
        argtypes, restype = split(proto)
        assert "sphmi_" + name in protos, f"{name}: not declared in include/sphmi.h or include/sphmi_internal.h"
        c_ret, c_args = protos["sphmi_" + name]
        assert len(argtypes) == len(c_args), f"{name}: the table lists {len(argtypes)} arguments, the header declares {len(c_args)}"
        for k, (t, decl) in enumerate(zip(argtypes, c_args)):
            assert t in admissible(decl), f"{name}: argument {k + 1} is {t.__name__} in the table and `{decl}` in the header"
        assert restype is (C.c_char_p if "*" in c_ret else SCALARS[c_ret]), f"{name}: returns `{c_ret}`, the table says {restype.__name__}"
    # the mask of sphmi_envelopes_enable is an int32_t in the header, whatever a raw caller passes
    assert _abi.PROTOTYPES["envelopes_enable"] == [C.c_void_p, C.c_int32]


def test_admissible_tells_the_classes_apart():
    assert admissible("sphmi_handle* h") == {C.c_void_p, C.c_char_p}
    assert admissible("const int64_t* counts") == {C.c_void_p, C.c_char_p, C.POINTER(C.c_int64)}
    assert admissible("sphmi_handle** out") == {C.c_void_p, C.c_char_p, C.POINTER(C.c_void_p)}
    assert admissible("const char** names_out") == {C.c_void_p, C.c_char_p, C.POINTER(C.c_char_p)}
    assert admissible("uint32_t type_mask") == {C.c_uint32} and admissible("int reset") == {C.c_int}
    assert admissible("int64_t capacity") == {C.c_int64} and admissible("double dp") == {C.c_double}


def sources():
    return sorted(glob.glob(os.path.join(ROOT, "sphexample_amd", "*.py")) + glob.glob(os.path.join(ROOT, "tools", "*.py")))


def test_every_entry_point_called_is_in_the_table():
    called = {}
    for path in sources():
        text = open(path).read()
        names = re.findall(r"""_fn\(\s*["'](\w+)["']""", text) + re.findall(r"""\bbind\([^,()]+,\s*["'](\w+)["']""", text)
        names += re.findall(r"\.sphmi_(\w+)\(", text)
        if path.endswith(os.path.join("sphexample_amd", "engine.py")):
            names += re.findall(r"""\b_call\(\s*["'](\w+)["']""", text)
        for n in names:
            called.setdefault(n, path)
    assert {"create", "advance", "download", "last_error", "rccl_probe", "multi_halo_info", "sample_grid"} <= set(called)
    missing = {n: os.path.relpath(p, ROOT) for n, p in called.items() if n not in _abi.PROTOTYPES}
    assert not missing, f"called, but without a prototype in _abi.PROTOTYPES: {missing}"


def test_only_the_table_declares_prototypes():
    for path in glob.glob(os.path.join(ROOT, "sphexample_amd", "*.py")):
        hits = re.findall(r"\.(?:argtypes|restype)\s*=[^=]", open(path).read())
        if os.path.basename(path) == "_abi.py":
            assert len(hits) == 2, hits                      # the two assignments of `bind`
        else:
            assert not hits, f"{os.path.relpath(path, ROOT)} assigns a prototype of its own"


class _Fn:
    argtypes = None

    def __init__(self, rc=_abi.OK):
        self.calls, self.rc = [], rc

    def __call__(self, *a):
        self.calls.append(a)
        return self.rc


class _Recorder:
    """Stands in for the library: remembers the prototype and the arguments it is handed and answers what `answers` says, else OK."""
    def __init__(self, **answers):
        self.fns = {"sphmi_" + k: _Fn(v) for k, v in answers.items()}

    def __getattr__(self, name):
        if name.startswith("sphmi_"):
            return self.fns.setdefault(name, _Fn())
        raise AttributeError(name)


def test_fn_restores_the_prototype_on_every_lookup():
    b = _abi.Backend.__new__(_abi.Backend)
    b._lib, b._p, b._h, b.N, b.D = _Recorder(), "sphmi_", C.c_void_p(), 10, 3
    fe = b._fn("probes_enable")
    assert fe.argtypes == _abi.PROTOTYPES["probes_enable"] == [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]
    fe.argtypes = None                                       # a raw caller widens it …
    b.probes_enable([[0.0, 0.0, 0.0]])
    assert fe is b._lib.fns["sphmi_probes_enable"] and fe.argtypes == _abi.PROTOTYPES["probes_enable"]      # … the wrapper runs under its own
    fe.argtypes.append(C.c_int)                              # what a caller does to the list it was handed stays with that caller
    assert len(_abi.PROTOTYPES["probes_enable"]) == 4 and b._fn("probes_enable").argtypes == _abi.PROTOTYPES["probes_enable"]
    assert b._fn("last_error").restype is C.c_char_p and _abi.bind(b._lib, "backend_info").restype is C.c_char_p
    with pytest.raises(KeyError):
        b._fn("no_such_entry_point")


def test_a_failing_call_without_a_handle_reports_the_text_of_the_library(monkeypatch):
    lib = _Recorder(rccl_probe=_abi.ERR_DEVICE, last_error=b"no rccl")
    monkeypatch.setattr(engine, "_lib", lib)
    with pytest.raises(engine.SphmiError, match="no rccl") as err:
        engine.rccl_probe()
    assert err.value.status == _abi.ERR_DEVICE
    assert lib.fns["sphmi_last_error"].restype is C.c_char_p and lib.fns["sphmi_last_error"].calls == [(None,)]
    assert lib.fns["sphmi_rccl_probe"].argtypes == [] and lib.fns["sphmi_rccl_probe"].calls == [()]
