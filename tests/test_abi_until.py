"""cgamd_solver_iterate_until (the per-right-hand-side tolerance stop of the launched loops) through the layers that need no GPU:
header, ctypes table, exported symbol, the argument checks of the C entry that need no handle, and the checks the Python layer makes
before it touches the device.  Mirrors test_abi_batched_pcg.py."""
import ctypes
import inspect
import os
import re
import subprocess
import types

import numpy as np
import pytest

from conftest import ROOT

ENTRY = "cgamd_solver_iterate_until"
C_ARGS = ["cgamd_solver *s", "int maxIterations", "const double *tol", "int nTol", "int checkEvery", "int *iterations_run"]
PY_ARGS = ["vp", "ci", "ctypes.POINTER(ctypes.c_double)", "ci", "ci", "ctypes.POINTER(ci)"]


def test_header_declares_the_entry():
    src = open(os.path.join(ROOT, "include", "cgamd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + ENTRY + r"\s*\(([^;{]*)\)\s*;", src)
    assert m, f"cgamd.h does not declare {ENTRY}"
    assert [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")] == C_ARGS


def test_ctypes_table_lists_the_entry(pkg):
    src = inspect.getsource(pkg._lib)
    m = re.search(r'"' + ENTRY + r'":\s*\(ci,\s*\[([^\]]*)\]\)', src)
    assert m, f"_lib.py does not list {ENTRY}"
    assert [a.strip() for a in m.group(1).split(",")] == PY_ARGS


def test_built_library_exports_it_and_the_signature_is_bound(pkg):
    for path in (pkg.LIB_PATH, pkg.LEGACY_LIB_PATH):
        if not os.path.exists(path):
            continue                                # not built here: test_abi_and_host asks for the build
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        assert any(line.split()[-1] == ENTRY and " T " in line for line in out.splitlines()), path
    fn = getattr(pkg._lib.load(), ENTRY)
    assert fn.restype is ctypes.c_int
    assert list(fn.argtypes) == [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.c_int, ctypes.c_int,
                                 ctypes.POINTER(ctypes.c_int)]


def _call(lib, handle, maxit, tol, ntol, chunk, its):
    t = tol.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if tol is not None else None
    i = its.ctypes.data_as(ctypes.POINTER(ctypes.c_int)) if its is not None else None
    return lib.cgamd_solver_iterate_until(handle, maxit, t, ntol, chunk, i)


def test_invalid_arguments(pkg):
    """every one of these is CGAMD_ERR_INVALID, and cgamd_last_error names what was wrong; the stand-in handle of the last four is
    never read (the argument is refused first)"""
    lib, L = pkg._lib.load(), pkg._lib
    tol, its = np.array([1e-5]), np.zeros(1, np.intc)
    assert _call(lib, None, 10, tol, 1, 8, its) == L.ERR_INVALID
    assert b"NULL" in lib.cgamd_last_error()
    junk = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(8)))
    assert _call(lib, None, 10, None, 1, 8, its) == L.ERR_INVALID
    assert _call(lib, None, 10, tol, 1, 8, None) == L.ERR_INVALID
    for ntol in (0, -1):
        assert _call(lib, junk, 10, tol, ntol, 8, its) == L.ERR_INVALID
        assert b"nTol" in lib.cgamd_last_error()
    assert _call(lib, junk, -1, tol, 1, 8, its) == L.ERR_INVALID
    assert b"negative" in lib.cgamd_last_error()
    assert _call(lib, junk, 10, tol, 1, -1, its) == L.ERR_INVALID
    assert b"negative" in lib.cgamd_last_error()
    assert its[0] == 0


class _NoLibrary:
    """stands for the loaded library of a stub handle: any entry that is asked for fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f"the library was asked for {name}")


def _reached_the_device(*args, **kwargs):
    raise AssertionError("the call went on to the device")


def _stub(pkg, n_rhs):
    stub = types.SimpleNamespace(n_rhs=n_rhs, size=4, dtype=np.dtype(np.complex64), handle=None, _lib=_NoLibrary(),
                                 set_rhs=_reached_the_device, iterate_until=_reached_the_device, x=_reached_the_device,
                                 history=_reached_the_device)
    stub._tolerances = types.MethodType(pkg.Solver._tolerances, stub)
    return stub


@pytest.mark.parametrize("count", [0, 2, 4])
def test_solve_until_checks_the_length_of_tol_first(pkg, count):
    """3 right-hand sides take a scalar, 1 or 3 tolerances"""
    stub = _stub(pkg, 3)
    with pytest.raises(ValueError, match="n_rhs = 3"):
        pkg.Solver.solve_until(stub, np.ones(12, np.complex64), tol=np.full(count, 1e-5))
    with pytest.raises(ValueError, match="n_rhs = 3"):
        pkg.Solver.iterate_until(stub, np.full(count, 1e-5), 10)


@pytest.mark.parametrize("tol", [0.0, -1e-5, float("nan"), [1e-5, 0.0, 1e-5]])
def test_solve_until_refuses_a_tolerance_that_is_not_positive(pkg, tol):
    with pytest.raises(ValueError, match="positive"):
        pkg.Solver.solve_until(_stub(pkg, 3), np.ones(12, np.complex64), tol=tol)


def test_tolerances_are_passed_as_float64(pkg):
    stub = _stub(pkg, 3)
    for tol, want in ((1e-5, [1e-5]), (np.float32(0.5), [0.5]), ([1, 2, 3], [1.0, 2.0, 3.0]), (np.array([[1e-3], [1e-4], [1e-5]]), [1e-3, 1e-4, 1e-5])):
        t = stub._tolerances(tol)
        assert t.dtype == np.float64 and t.flags.c_contiguous and t.tolist() == want


def _csr(indptr, indices, data):
    return types.SimpleNamespace(indptr=np.asarray(indptr, np.int32), indices=np.asarray(indices, np.int32),
                                 data=np.asarray(data, np.complex64))


def test_solve_subdomains_checks_tol_before_the_device(pkg):
    """two residuals take a scalar or two tolerances; ctx is None here, so anything that reached the device would fail otherwise"""
    A = _csr([0, 2, 3], [0, 1, 1], [2, 1, 3])
    r = [np.ones(2, np.complex64), np.ones(2, np.complex64)]
    for bad in (np.full(3, 1e-5), np.zeros(0)):
        with pytest.raises(ValueError, match="one entry per sub-domain"):
            pkg.solve_subdomains(None, A, r, 5, tol=bad)
        with pytest.raises(ValueError, match="one entry per sub-domain"):
            pkg.solve_subdomains(None, [A, A], r, 5, tol=bad, return_iterations=True)
    with pytest.raises(ValueError, match="positive"):
        pkg.solve_subdomains(None, A, r, 5, tol=[1e-5, -1.0])


def test_solve_subdomains_keeps_its_signature_for_fixed_counts(pkg):
    sig = inspect.signature(pkg.solve_subdomains)
    assert list(sig.parameters)[:7] == ["ctx", "P0", "residuals", "n_iterations", "dtype", "solver", "preconditioner"]
    assert sig.parameters["tol"].default is None and sig.parameters["return_iterations"].default is False
