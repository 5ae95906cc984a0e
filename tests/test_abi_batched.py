"""The batched handle (cgamd_solver_create_batched / cgamd_solver_systems: one pattern, a matrix of its own per right-hand side)
through the layers that need no GPU: header, ctypes table, exported symbols, Makefile, argument checks of the C entries and of the
Python layer."""
import inspect
import os
import re
import subprocess
import types

import numpy as np
import pytest

from conftest import ROOT, PKG_NAME

ENTRIES = {
    "cgamd_solver_create_batched": (["cgamd_ctx *ctx", "int dtype", "int size", "long long nnz", "const void *aValues",
                                     "const int *aPointers", "const int *aCols", "int nSystems", "int flags", "cgamd_solver **out"],
                                    ["vp", "ci", "ci", "ll", "vp", "vp", "vp", "ci", "ci", "pvp"]),
    "cgamd_solver_systems": (["cgamd_solver *s"], ["vp"]),
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


def test_makefile_builds_the_kernel_file():
    mk = open(os.path.join(ROOT, PKG_NAME, "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    assert "batched.hip" in srcs
    assert os.path.exists(os.path.join(ROOT, PKG_NAME, "csrc", "batched.hip"))


def test_family_six_is_appended(pkg):
    assert pkg.Solver.SPMV_FAMILIES[:6] == ("stream", "rowblock", "vc", "vcp", "chunked", "spmm")
    assert pkg.Solver.SPMV_FAMILIES[6] == "batched" and len(pkg.Solver.SPMV_FAMILIES) == 7


def test_create_rejects_bad_arguments(pkg):
    import ctypes
    lib = pkg._lib.load()
    ip = np.array([0, 1], np.int32)
    ix = np.zeros(1, np.int32)
    a = np.ones(1, np.float64)
    args = (pkg._lib.F64, 1, 1, pkg._lib.ptr(a), pkg._lib.ptr(ip), pkg._lib.ptr(ix))
    h = ctypes.c_void_p(1234)
    assert lib.cgamd_solver_create_batched(None, *args, 1, 0, ctypes.byref(h)) == pkg._lib.ERR_INVALID      # NULL ctx
    assert h.value is None                                                                                   # *out is cleared
    fake_ctx = ctypes.c_void_p(1)           # never dereferenced: the argument checks come first
    assert lib.cgamd_solver_create_batched(fake_ctx, *args, 1, 0, None) == pkg._lib.ERR_INVALID             # NULL out
    for nsys in (0, -3):
        h = ctypes.c_void_p(1234)
        assert lib.cgamd_solver_create_batched(fake_ctx, *args, nsys, 0, ctypes.byref(h)) == pkg._lib.ERR_INVALID
        assert h.value is None
        assert b"nSystems" in lib.cgamd_last_error()


def test_systems_of_a_null_handle_is_negative(pkg):
    assert pkg._lib.load().cgamd_solver_systems(None) < 0


@pytest.mark.parametrize("count", [0, 6, 17, 19, 36])
def test_solver_checks_the_value_count(pkg, count):
    """3 systems x 6 non-zeros take 18 values; the check comes before the library is asked for anything"""
    ip = np.array([0, 2, 4, 6], np.int32)
    ix = np.array([0, 1, 0, 1, 1, 2], np.int32)
    with pytest.raises(ValueError, match="18"):
        pkg.Solver(None, 3, 6, np.ones(count, np.float64), ip, ix, 3, batched=True)


def _csr(indptr, indices, data):
    return types.SimpleNamespace(indptr=np.asarray(indptr, np.int32), indices=np.asarray(indices, np.int32),
                                 data=np.asarray(data, np.complex64))


def test_solve_subdomains_checks_the_pattern_first(pkg):
    """a matrix on another pattern is refused before anything touches the device (ctx is None here)"""
    A = _csr([0, 2, 3], [0, 1, 1], [2, 1, 3])
    B_cols = _csr([0, 2, 3], [1, 0, 1], [2, 1, 3])          # same row lengths, other columns
    B_ptr = _csr([0, 1, 3], [0, 0, 1], [2, 1, 3])           # other row pointers
    r = [np.ones(2, np.complex64), np.ones(2, np.complex64)]
    for B in (B_cols, B_ptr):
        with pytest.raises(ValueError, match="pattern"):
            pkg.solve_subdomains(None, [A, B], r, 5)
    with pytest.raises(ValueError, match="residuals"):
        pkg.solve_subdomains(None, [A, A], r + r, 5)
