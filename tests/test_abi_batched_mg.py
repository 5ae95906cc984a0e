"""Multigrid PCG on the batched handle (cgamd_solver_set_preconditioner_batched_multigrid, cgamd_solver_mg_level_bounds) through the
layers that need no GPU: header, ctypes table, exported symbols, the NULL-handle answer and the Python layer's argument check.
The scheme of test_abi_batched_pcg.py."""
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
    "cgamd_solver_set_preconditioner_batched_multigrid": (
        ["cgamd_solver *s", "int nx", "int ny", "int nz", "int smooth_steps", "double over_correction", "int min_rows"],
        ["vp", "ci", "ci", "ci", "ci", "ctypes.c_double", "ci"]),
    "cgamd_solver_mg_level_bounds": (["cgamd_solver *s", "int level", "double *lmax", "int count"],
                                     ["vp", "ci", "ctypes.POINTER(ctypes.c_double)", "ci"]),
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
    assert lib.cgamd_solver_set_preconditioner_batched_multigrid(None, 4, 4, 1, 0, ctypes.c_double(0.0), 0) == L.ERR_INVALID
    assert b"set_preconditioner_batched_multigrid" in lib.cgamd_last_error() and b"NULL" in lib.cgamd_last_error()
    out = (ctypes.c_double * 1)()
    assert lib.cgamd_solver_mg_level_bounds(None, 0, out, 1) == L.ERR_INVALID
    assert b"NULL" in lib.cgamd_last_error()


class _NoLibrary:
    """stands for the loaded library of a stub handle: any entry that is asked for fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f"the library was asked for {name}")


def test_set_preconditioner_checks_the_options_first(pkg):
    """the option names and the ValueError text of the single-system form, before the library is asked"""
    stub = types.SimpleNamespace(batched=True, n_rhs=3, size=24, dtype=np.dtype(np.float64), handle=None, _lib=_NoLibrary())
    for m in (("multigrid", (4, 3, 2), {"steps": 2}), ("multigrid", (4, 3, 2, 1))):
        with pytest.raises(ValueError, match=r'\("multigrid", \(nx, ny, nz\)\[, \{"smooth_steps": 1, "over_correction": 1.6, "min_rows": 512\}\]\)'):
            pkg.Solver.set_preconditioner(stub, m)


def test_set_preconditioner_calls_the_batched_entry(pkg):
    """("multigrid", (nx, ny)[, opts]) on a batched handle reaches the batched entry with nz = 1 and 0 for every option left out"""
    calls = []
    lib = types.SimpleNamespace(cgamd_solver_set_preconditioner_batched_multigrid=lambda *a: calls.append(a) or 0)
    stub = types.SimpleNamespace(batched=True, n_rhs=3, size=12, dtype=np.dtype(np.float64), handle=7, _lib=lib)
    pkg.Solver.set_preconditioner(stub, ("multigrid", (4, 3)))
    pkg.Solver.set_preconditioner(stub, ("multigrid", (2, 3, 2), {"min_rows": 32, "over_correction": 1.0}))
    assert calls == [(7, 4, 3, 1, 0, 0.0, 0), (7, 2, 3, 2, 0, 1.0, 32)]
