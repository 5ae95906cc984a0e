"""cgamd_dist_iterate_until / cgamd_dist_iterations_done (tolerance stop on the device for the row-partitioned handle) through the
layers that need no GPU: header, ctypes table, exported symbols, the returns of the C entries that need no device, and the checks
DistSolver makes before it touches the library.  Mirrors test_abi_until.py / test_abi_refresh.py."""
import ctypes
import importlib
import inspect
import os
import re
import subprocess
import types

import numpy as np
import pytest

from conftest import ROOT

ENTRIES = {
    "cgamd_dist_iterate_until": (["cgamd_dist *d", "int maxIterations", "double tol", "int checkEvery", "int *iterations_run"],
                                 ["vp", "ci", "ctypes.c_double", "ci", "ctypes.POINTER(ci)"]),
    "cgamd_dist_iterations_done": (["cgamd_dist *d"], ["vp"]),
}
CTYPES = {"vp": ctypes.c_void_p, "ci": ctypes.c_int, "ctypes.c_double": ctypes.c_double, "ctypes.POINTER(ci)": ctypes.POINTER(ctypes.c_int)}


def _dist(pkg):
    return importlib.import_module(pkg.__name__ + ".dist")


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_header_declares_the_entry(entry):
    src = open(os.path.join(ROOT, "include", "cgamd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + entry + r"\s*\(([^;{]*)\)\s*;", src)
    assert m, f"cgamd.h does not declare {entry}"
    assert [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")] == ENTRIES[entry][0]


def test_header_states_the_contract():
    src = re.sub(r"[\s*]+", " ", open(os.path.join(ROOT, "include", "cgamd.h")).read())
    at = src.index("int cgamd_dist_iterate_until(")
    text = src[src.rindex("Tolerance stop on the device for the row-partitioned handle", 0, at):at]
    for phrase in ("every rank makes the same call", "!(sqrt|delta_k| >= tol)", "NaN stops", "still r.r, not rho", "never per iteration",
                   "does not depend on checkEvery", "until(a); until(b) leaves the bits of until(a + b)", "CGAMD_DIST_SINGLE_REDUCTION",
                   "COMMUNICATION NEVER DEPENDS ON THE STOP", "slab loop has no stop"):
        assert phrase in text, phrase
    # the stopped-handle case at cgamd_dist_iterate
    it = src[:src.index("int cgamd_dist_iterate(")]
    assert "cgamd_dist_iterate_until has stopped" in it[-400:]


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_ctypes_table_lists_the_entry(pkg, entry):
    src = inspect.getsource(pkg._lib)
    m = re.search(r'"' + entry + r'":\s*\(ci,\s*\[(.*)\]\)', src)
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


def test_null_handle_and_bad_arguments_need_no_device(pkg):
    lib, L = pkg._lib.load(), pkg._lib
    its = ctypes.c_int(-7)
    assert lib.cgamd_dist_iterate_until(None, 10, 1e-6, 8, ctypes.byref(its)) == L.ERR_INVALID
    assert b"NULL" in lib.cgamd_last_error()
    assert its.value == -7
    # what can be judged without the handle is judged first
    for maxit, tol, every in ((-1, 1e-6, 8), (10, 1e-6, -1), (10, 0.0, 8), (10, -1.0, 8), (10, float("nan"), 8)):
        assert lib.cgamd_dist_iterate_until(None, maxit, tol, every, ctypes.byref(its)) == L.ERR_INVALID
        assert b"NULL" not in lib.cgamd_last_error()
    assert lib.cgamd_dist_iterations_done(None) == -L.ERR_INVALID


def test_the_wrappers_exist(pkg):
    D = _dist(pkg).DistSolver
    sig = inspect.signature(D.iterate_until)
    assert list(sig.parameters) == ["self", "tol", "maxit", "check_every", "group"]
    assert sig.parameters["check_every"].default == 8 and sig.parameters["group"].default is None
    sig = inspect.signature(D.solve_until)
    assert list(sig.parameters) == ["self", "b_local", "x0_local", "tol", "maxit", "check_every", "group"]
    assert [sig.parameters[k].default for k in ("x0_local", "tol", "maxit", "check_every", "group")] == [None, 1e-5, 1000, 8, None]
    assert isinstance(D.iterations_done, property)
    d = _dist(pkg)
    assert list(inspect.signature(d.cg_loop_until).parameters) == ["ops", "comm", "plan", "b_local", "x0_local", "tol", "maxit"]
    assert list(inspect.signature(d.pcg_loop_until).parameters) == ["ops", "comm", "plan", "b_local", "x0_local", "tol", "maxit", "apply_m"]


class _NoLibrary:
    """stands for the loaded library of a stub handle: any entry that is asked for fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f"the library was asked for {name}")


def _stub(pkg):
    D = _dist(pkg).DistSolver
    stub = types.SimpleNamespace(handle=None, _lib=_NoLibrary(), plan=types.SimpleNamespace(world=1), iterations=0, dtype=np.dtype(np.float64))
    stub._until_args = D._until_args
    stub.set_rhs = lambda *a: (_ for _ in ()).throw(AssertionError("set_rhs was reached"))
    stub.iterate_until = types.MethodType(D.iterate_until, stub)
    return stub


@pytest.mark.parametrize("kw", [dict(tol=0.0), dict(tol=-1e-3), dict(tol=float("nan")), dict(tol="small"), dict(maxit=-1), dict(maxit=2.5),
                                dict(check_every=-1), dict(check_every=None)])
def test_bad_arguments_are_refused_before_the_library(pkg, kw):
    D = _dist(pkg).DistSolver
    args = dict(tol=1e-6, maxit=10, check_every=8)
    args.update(kw)
    with pytest.raises(ValueError):
        D.iterate_until(_stub(pkg), args["tol"], args["maxit"], args["check_every"])
    with pytest.raises(ValueError):
        D.solve_until(_stub(pkg), np.ones(4), None, args["tol"], args["maxit"], args["check_every"])


def test_good_arguments_reach_the_library_and_set_the_count(pkg):
    """(so the refusals above are the wrapper's, not a stub that refuses everything)"""
    D = _dist(pkg).DistSolver
    calls = []

    def until(handle, maxit, tol, every, its):
        calls.append((maxit, tol, every))
        its._obj.value = 13
        return 0
    stub = _stub(pkg)
    stub._lib = types.SimpleNamespace(cgamd_dist_iterate_until=until, cgamd_last_error=lambda: b"")
    assert D.iterate_until(stub, 1e-6, 24, 0) == 13
    assert calls == [(24, 1e-6, 0)] and stub.iterations == 13
