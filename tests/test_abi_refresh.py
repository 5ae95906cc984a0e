"""cgamd_solver_refresh_values / cgamd_dist_refresh_values (new matrix VALUES on the same pattern, in place on the device) and their
_last_refresh accessors through the layers that need no GPU: header, ctypes table, exported symbols, the returns of the C entries that
need no device, and the checks the Python layer makes before it touches the device.  Mirrors test_abi_until.py."""
import ctypes
import inspect
import os
import re
import subprocess
import types

import numpy as np
import pytest

from conftest import ROOT

ENTRIES = {
    "cgamd_solver_refresh_values": (["cgamd_solver *s", "const void *aValues", "int on_device"], ["vp", "vp", "ci"]),
    "cgamd_solver_last_refresh": (["cgamd_solver *s"], ["vp"]),
    "cgamd_solver_graph_captures": (["cgamd_solver *s"], ["vp"]),
    "cgamd_dist_refresh_values": (["cgamd_dist *d"], ["vp"]),
    "cgamd_dist_last_refresh": (["cgamd_dist *d"], ["vp"]),
}
CTYPES = {"vp": ctypes.c_void_p, "ci": ctypes.c_int}


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_header_declares_the_entry(entry):
    src = open(os.path.join(ROOT, "include", "cgamd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + entry + r"\s*\(([^;{]*)\)\s*;", src)
    assert m, f"cgamd.h does not declare {entry}"
    assert [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")] == ENTRIES[entry][0]


def test_header_states_the_contract_of_borrowed_values():
    """at CGAMD_MATRIX_ON_DEVICE: changed only between solves, every change followed by the refresh before the next set_rhs"""
    src = open(os.path.join(ROOT, "include", "cgamd.h")).read()
    m = re.search(r"#define CGAMD_MATRIX_ON_DEVICE 1\s*/\*(.*?)\*/", src, flags=re.S)
    assert m
    text = re.sub(r"[\s*]+", " ", m.group(1))
    assert "only between solves" in text and "cgamd_solver_refresh_values" in text and "cgamd_solver_set_rhs" in text
    doc = re.sub(r"\s+", " ", open(os.path.join(ROOT, "INTEGRATION.md")).read())
    assert "only between solves" in doc and "refresh_values" in doc


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_ctypes_table_lists_the_entry(pkg, entry):
    src = inspect.getsource(pkg._lib)
    m = re.search(r'"' + entry + r'":\s*\(ci,\s*\[([^\]]*)\]\)', src)
    assert m, f"_lib.py does not list {entry}"
    assert [a.strip() for a in m.group(1).split(",")] == ENTRIES[entry][1]


def test_built_library_exports_them_and_the_signatures_are_bound(pkg):
    for path in (pkg.LIB_PATH, pkg.LEGACY_LIB_PATH):
        if not os.path.exists(path):
            continue                                # not built here: test_abi_and_host asks for the build
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        names = {line.split()[-1] for line in out.splitlines() if " T " in line}
        assert set(ENTRIES) <= names, (path, set(ENTRIES) - names)
    lib = pkg._lib.load()
    for entry, (_, args) in ENTRIES.items():
        fn = getattr(lib, entry)
        assert fn.restype is ctypes.c_int
        assert list(fn.argtypes) == [CTYPES[a] for a in args]


def test_null_handles(pkg):
    """no device is needed to refuse a NULL handle; the accessors answer with the negative status, as the other accessors do"""
    lib, L = pkg._lib.load(), pkg._lib
    values = np.ones(4)
    for v, on_device in ((None, 0), (None, 1), (values.ctypes.data_as(ctypes.c_void_p), 0)):
        assert lib.cgamd_solver_refresh_values(None, v, on_device) == L.ERR_INVALID
        assert b"NULL" in lib.cgamd_last_error()
    assert lib.cgamd_solver_last_refresh(None) == -L.ERR_INVALID
    assert lib.cgamd_solver_graph_captures(None) == -L.ERR_INVALID
    assert lib.cgamd_dist_refresh_values(None) == L.ERR_INVALID
    assert b"null" in lib.cgamd_last_error().lower()
    assert lib.cgamd_dist_last_refresh(None) == -L.ERR_INVALID


class _NoLibrary:
    """stands for the loaded library of a stub handle: any entry that is asked for fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f"the library was asked for {name}")


def _stub(pkg, on_device, batched=False):
    stub = types.SimpleNamespace(n_rhs=3 if batched else 1, size=4, non_zeros=10, dtype=np.dtype(np.float64), handle=None, _lib=_NoLibrary(),
                                 batched=batched, _on_device=on_device)
    stub._check_batched_values = types.MethodType(pkg.Solver._check_batched_values, stub)
    return stub


def test_the_wrappers_exist(pkg):
    assert list(inspect.signature(pkg.Solver.refresh_values).parameters) == ["self", "a_values"]
    assert inspect.signature(pkg.Solver.refresh_values).parameters["a_values"].default is None
    assert isinstance(pkg.Solver.last_refresh, property) and isinstance(pkg.Solver.graph_captures, property)
    dist = __import__("importlib").import_module(pkg.__name__ + ".dist")
    assert list(inspect.signature(dist.DistSolver.refresh_values).parameters) == ["self", "group"]
    assert inspect.signature(dist.DistSolver.refresh_values).parameters["group"].default is None
    assert isinstance(dist.DistSolver.last_refresh, property)


def test_none_is_refused_on_an_owning_handle_before_the_device(pkg):
    """None means 'the borrowed array changed in place': a handle that owns its matrix has no such array"""
    with pytest.raises(ValueError, match="owns its matrix"):
        pkg.Solver.refresh_values(_stub(pkg, on_device=False))
    with pytest.raises(ValueError, match="owns its matrix"):
        pkg.Solver.refresh_values(_stub(pkg, on_device=False, batched=True), None)


def test_none_orders_torchs_stream_first(pkg, monkeypatch):
    """the borrowed tensor was rewritten on torch's stream, which the handle's non-blocking stream does not wait for: the wrapper
    synchronises before the library reads the values"""
    import sys
    calls = []
    fake_torch = types.SimpleNamespace(cuda=types.SimpleNamespace(synchronize=lambda: calls.append("sync")))
    monkeypatch.setitem(sys.modules, "torch", fake_torch)
    lib = types.SimpleNamespace(cgamd_solver_refresh_values=lambda h, v, on_device: calls.append(("refresh", v, on_device)) or 0)
    stub = _stub(pkg, on_device=True)
    stub._lib = lib
    stub._keep = (types.SimpleNamespace(is_cuda=True), None, None)
    pkg.Solver.refresh_values(stub)
    assert calls == ["sync", ("refresh", None, 0)]


def test_lengths_are_checked_before_the_device(pkg):
    """a host array of the wrong length never reaches the library: nnz values, a batched handle n_rhs * nnz"""
    with pytest.raises(ValueError, match="10 non-zeros"):
        pkg.Solver.refresh_values(_stub(pkg, on_device=False), np.ones(9))
    with pytest.raises(ValueError, match="3 \\* 10 = 30"):
        pkg.Solver.refresh_values(_stub(pkg, on_device=False, batched=True), np.ones(10))
