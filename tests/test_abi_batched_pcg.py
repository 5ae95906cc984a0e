"""Preconditioned CG on the batched handle (cgamd_solver_set_preconditioner_batched / _batched_jacobi / _batched_line: one M per system)
through the layers that need no GPU: header, ctypes table, exported symbols, argument checks of the C entries and of the Python
layer.  Mirrors test_abi_batched.py."""
import inspect
import os
import re
import subprocess
import types

import numpy as np
import pytest

from conftest import ROOT

ENTRIES = {
    "cgamd_solver_set_preconditioner_batched": (["cgamd_solver *s", "const void *m", "int on_device"], ["vp", "vp", "ci"]),
    "cgamd_solver_set_preconditioner_batched_jacobi": (["cgamd_solver *s"], ["vp"]),
    "cgamd_solver_set_preconditioner_batched_line": (["cgamd_solver *s", "int stride"], ["vp", "ci"]),
}


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_header_declares_the_entry(entry):
    src = open(os.path.join(ROOT, "include", "cgamd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + entry + r"\s*\(([^;{]*)\)\s*;", src)
    assert m, f"cgamd.h does not declare {entry}"
    args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
    assert args == ENTRIES[entry][0]


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_ctypes_table_lists_the_entry(pkg, entry):
    src = inspect.getsource(pkg._lib)
    m = re.search(r'"' + entry + r'":\s*\(ci,\s*\[([^\]]*)\]\)', src)
    assert m, f"_lib.py does not list {entry}"
    assert [a.strip() for a in m.group(1).split(",")] == ENTRIES[entry][1]


def test_built_library_exports_them(pkg):
    for path in (pkg.LIB_PATH, pkg.LEGACY_LIB_PATH):
        if not os.path.exists(path):
            continue                                # not built here: test_abi_and_host asks for the build
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        for entry, (_, argtypes) in ENTRIES.items():
            assert any(line.split()[-1] == entry and " T " in line for line in out.splitlines()), (path, entry)
            assert len(getattr(pkg._lib.load(), entry).argtypes) == len(argtypes)


def test_a_null_handle_is_invalid(pkg):
    lib, L = pkg._lib.load(), pkg._lib
    m = np.ones(4, np.float64)
    assert lib.cgamd_solver_set_preconditioner_batched(None, L.ptr(m), 0) == L.ERR_INVALID
    assert lib.cgamd_solver_set_preconditioner_batched(None, None, 0) == L.ERR_INVALID
    assert lib.cgamd_solver_set_preconditioner_batched_jacobi(None) == L.ERR_INVALID
    assert lib.cgamd_solver_set_preconditioner_batched_line(None, 1) == L.ERR_INVALID
    assert b"NULL" in lib.cgamd_last_error()


class _NoLibrary:
    """stands for the loaded library of a stub handle: any entry that is asked for fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f"the library was asked for {name}")


@pytest.mark.parametrize("count", [0, 4, 11, 13, 24])
def test_set_preconditioner_checks_the_length_first(pkg, count):
    """3 systems of 4 rows take 12 diagonal entries, 1-D or (3, 4); any other length raises before the library is asked"""
    stub = types.SimpleNamespace(batched=True, n_rhs=3, size=4, dtype=np.dtype(np.float64), handle=None, _lib=_NoLibrary())
    with pytest.raises(ValueError, match="12"):
        pkg.Solver.set_preconditioner(stub, np.ones(count))
    with pytest.raises(ValueError, match="12"):
        pkg.Solver.set_preconditioner(stub, np.ones((2, 4)))
    with pytest.raises(ValueError, match="12"):
        pkg.Solver.set_preconditioner(stub, [1.0] * count)


def test_set_preconditioner_refuses_what_has_no_meaning_per_system(pkg):
    """a name that is none, an object that is no array: ValueError pointing at ("line", stride), the library untouched"""
    stub = types.SimpleNamespace(batched=True, n_rhs=3, size=4, dtype=np.dtype(np.float64), handle=None, _lib=_NoLibrary())
    for m in ("ilu", ("lines", 2), object()):
        with pytest.raises(ValueError, match="line"):
            pkg.Solver.set_preconditioner(stub, m)


def _csr(indptr, indices, data):
    return types.SimpleNamespace(indptr=np.asarray(indptr, np.int32), indices=np.asarray(indices, np.int32),
                                 data=np.asarray(data, np.complex64))


def test_solve_subdomains_refuses_a_preconditioner_for_a_shared_matrix(pkg):
    """one matrix for all residuals has no per-system M: ValueError before anything touches the device (ctx is None here)"""
    A = _csr([0, 2, 3], [0, 1, 1], [2, 1, 3])
    r = [np.ones(2, np.complex64), np.ones(2, np.complex64)]
    with pytest.raises(ValueError, match="batched"):
        pkg.solve_subdomains(None, A, r, 5, preconditioner="jacobi")
    with pytest.raises(ValueError, match="batched"):
        pkg.solve_subdomains(None, (A.indptr, A.indices, A.data), r, 5, preconditioner=("line", 1))
    plain = types.SimpleNamespace(batched=False)
    with pytest.raises(ValueError, match="batched"):
        pkg.solve_subdomains(None, [A, A], r, 5, solver=plain, preconditioner="jacobi")
