"""cgamd_solver_replace_residual and the mixed-precision entries (cgamd_mixed_*) through the layers that need no GPU: header, ctypes
table, exported symbols, the argument checks that are made before a device is touched, and the numpy restatement of the scheme
(tests/mixed_ref.py) on the system of the device tests."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import mixed_ref

PD, PI = "ctypes.POINTER(ctypes.c_double)", "ctypes.POINTER(ci)"
# entry: (C return type, C arguments, the table's result, the table's arguments)
ENTRIES = {
    "cgamd_solver_replace_residual": ("int", ["cgamd_solver *s", "const void *r_new"], "ci", ["vp", "vp"]),
    "cgamd_mixed_create": ("int", ["cgamd_ctx *ctx", "int dtype_hi", "int size", "long long nnz", "const void *aValues_hi", "const int *aPointers",
                                   "const int *aCols", "int nRHS", "int flags", "cgamd_mixed **out"],
                           "ci", ["vp", "ci", "ci", "ll", "vp", "vp", "vp", "ci", "ci", "pvp"]),
    "cgamd_mixed_destroy": ("int", ["cgamd_mixed *m"], "ci", ["vp"]),
    "cgamd_mixed_outer": ("cgamd_solver *", ["cgamd_mixed *m"], "vp", ["vp"]),
    "cgamd_mixed_inner": ("cgamd_solver *", ["cgamd_mixed *m"], "vp", ["vp"]),
    "cgamd_mixed_solve": ("int", ["cgamd_mixed *m", "const void *b", "void *x", "int on_device", "const double *tol", "int nTol", "int maxIterations",
                                  "double delta", "int maxSegment", "int checkEvery", "int *iterations", "double *resnorm", "int *status",
                                  "int *replacements"],
                          "ci", ["vp", "vp", "vp", "ci", PD, "ci", "ci", "ctypes.c_double", "ci", "ci", PI, PD, PI, PI]),
    "cgamd_mixed_scales": ("int", ["cgamd_mixed *m", "double *scales"], "ci", ["vp", PD]),
}


def _header():
    src = open(os.path.join(ROOT, "include", "cgamd.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_header_declares_the_entry(entry):
    ret, c_args, _, _ = ENTRIES[entry]
    m = re.search(r"(\bint\s+|\bcgamd_solver\s*\*\s*)" + entry + r"\s*\(([^;{]*)\)\s*;", _header())
    assert m, f"cgamd.h does not declare {entry}"
    assert re.sub(r"\s+", " ", m.group(1)).strip() == ret
    assert [re.sub(r"\s+", " ", a.strip()) for a in m.group(2).split(",")] == c_args


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_ctypes_table_lists_the_entry(pkg, entry):
    _, _, res, py_args = ENTRIES[entry]
    src = inspect.getsource(pkg._lib)
    m = re.search(r'"' + entry + r'":\s*\((\w+),\s*\[(.*?)\]\)', src, flags=re.S)
    assert m, f"_lib.py does not list {entry}"
    assert m.group(1) == res
    assert [re.sub(r"\s+", " ", a.strip()) for a in m.group(2).split(",")] == py_args


def test_built_libraries_export_the_entries(pkg):
    for path in (pkg.LIB_PATH, pkg.LEGACY_LIB_PATH):
        assert os.path.exists(path), "run __graft_entry__.build() first"
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
        assert set(ENTRIES) <= exported, (path, sorted(set(ENTRIES) - exported))
    lib = pkg._lib.load()
    assert lib.cgamd_mixed_outer.restype is ctypes.c_void_p and lib.cgamd_mixed_solve.restype is ctypes.c_int
    assert len(lib.cgamd_mixed_solve.argtypes) == 14 and len(lib.cgamd_mixed_create.argtypes) == 10


def test_python_layer_has_the_surface(pkg):
    assert list(inspect.signature(pkg.MixedSolver.__init__).parameters)[:9] == ["self", "ctx", "size", "non_zeros", "a_values", "a_pointers",
                                                                                 "a_cols", "n_rhs", "flags"]
    sig = inspect.signature(pkg.MixedSolver.solve)
    assert list(sig.parameters) == ["self", "b", "x0", "tol", "maxit", "delta", "max_segment", "check_every"]
    assert sig.parameters["delta"].default == 0.1 and sig.parameters["max_segment"].default == 0 and sig.parameters["check_every"].default == 8
    assert callable(pkg.Solver.replace_residual)


def test_null_arguments_are_invalid(pkg):
    lib, L = pkg._lib.load(), pkg._lib
    junk = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    assert lib.cgamd_solver_replace_residual(None, junk) == L.ERR_INVALID
    assert b"null" in lib.cgamd_last_error().lower()
    assert lib.cgamd_mixed_create(None, L.F64, 4, 4, junk, junk, junk, 1, 0, None) == L.ERR_INVALID
    h = ctypes.c_void_p()
    assert lib.cgamd_mixed_create(None, L.F64, 4, 4, junk, junk, junk, 1, 0, ctypes.byref(h)) == L.ERR_INVALID
    assert b"ctx" in lib.cgamd_last_error() and not h.value
    tol, its, res = np.array([1e-5]), np.zeros(1, np.intc), np.zeros(1)
    pd, pi = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    args = [None, junk, junk, 0, tol.ctypes.data_as(pd), 1, 10, 0.1, 0, 8, its.ctypes.data_as(pi), res.ctypes.data_as(pd), its.ctypes.data_as(pi),
            its.ctypes.data_as(pi)]
    assert lib.cgamd_mixed_solve(*args) == L.ERR_INVALID
    assert b"null" in lib.cgamd_last_error().lower()
    assert lib.cgamd_mixed_scales(None, res.ctypes.data_as(pd)) == L.ERR_INVALID
    assert lib.cgamd_mixed_destroy(None) == L.OK
    assert not lib.cgamd_mixed_outer(None) and not lib.cgamd_mixed_inner(None)


def test_bad_dtype_and_flags_are_refused_before_any_device_is_touched(pkg):
    """ctx is NULL in every call: a refusal that names the dtype or the flags was made before the context was looked at"""
    lib, L = pkg._lib.load(), pkg._lib
    junk = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    h = ctypes.c_void_p()
    for dt in (L.F32, L.C64, -1, 4):
        assert lib.cgamd_mixed_create(None, dt, 4, 4, junk, junk, junk, 1, 0, ctypes.byref(h)) == L.ERR_INVALID
        assert b"dtype_hi" in lib.cgamd_last_error() and not h.value
    for flags in (L.UNFUSED, L.HERMITIAN, L.UNFUSED | L.NO_GRAPH, L.HERMITIAN | L.MATRIX_ON_DEVICE, L.DIST_P2P):
        for dt in (L.F64, L.C128):
            assert lib.cgamd_mixed_create(None, dt, 4, 4, junk, junk, junk, 1, flags, ctypes.byref(h)) == L.ERR_INVALID
            assert b"flags" in lib.cgamd_last_error() and not h.value
    for flags in (0, L.NO_GRAPH, L.MATRIX_ON_DEVICE, L.NO_GRAPH | L.MATRIX_ON_DEVICE):     # accepted: the next check (ctx) answers
        assert lib.cgamd_mixed_create(None, L.F64, 4, 4, junk, junk, junk, 1, flags, ctypes.byref(h)) == L.ERR_INVALID
        assert b"ctx" in lib.cgamd_last_error()


def test_the_restated_scheme_reaches_the_tolerance_on_the_true_residual():
    """Poisson 33 x 29 to 1e-10 ||b||: float32 alone stalls near 3e-6 ||b||; the mixed scheme gets there in about the fp64 count"""
    indptr, indices, data = mixed_ref.poisson2d_rect(33, 29)
    assert len(indptr) - 1 == 957
    b = np.random.default_rng(3).standard_normal(957)
    tol = 1e-10 * float(np.sqrt(abs(b @ b)))
    x, info = mixed_ref.mixed_cg(indptr, indices, data, b, tol=tol, maxit=1000)
    r = b - mixed_ref.csr_matvec(indptr, indices, data, x)
    absx = mixed_ref.csr_matvec(indptr, indices, np.abs(data), np.abs(x))
    slack = float(np.linalg.norm(8 * np.finfo(np.float64).eps * (absx + np.abs(b))))
    assert info["status"] == 0 and float(np.sqrt(abs(r @ r))) <= tol + slack
    assert abs(info["resnorm"] - float(np.sqrt(abs(r @ r)))) <= slack
    _, k64 = mixed_ref.cg_hi(indptr, indices, data, b, tol, 1000)
    assert info["iterations"] <= 1.3 * k64, (info, k64)
    assert 2 <= info["replacements"] <= 40
    assert info["scale"] == 2.0 ** np.floor(np.log2(np.linalg.norm(b)))
