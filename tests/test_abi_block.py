"""The block CG entries through the layers that need no GPU: the header, the ctypes table, the Makefile, the exported symbols, the
refusals a call makes before it touches a device, and the argument checks of the Python interface.  Mirrors test_abi_shifts.py."""
import inspect
import os
import re
import subprocess
import types

import numpy as np
import pytest

from conftest import PKG_NAME, ROOT

ENTRIES = {
    "cgamd_solver_set_block": ["cgamd_solver *s", "int on"],
    "cgamd_solver_block_status": ["cgamd_solver *s", "int *info", "double *min_pivot_ratio"],
    "cgamd_solver_block_state": ["cgamd_solver *s", "int which", "void *out_host"],
    "cgamd_block_gram_grid": ["int size"],
    "cgamd_block_gram": ["cgamd_ctx *ctx", "int dtype", "int size", "long long ld", "int s", "const void *a", "const void *b", "void *partials"],
    "cgamd_block_update_xw": ["cgamd_ctx *ctx", "int dtype", "int size", "long long ld", "int s", "const void *p", "const void *ap", "void *x",
                              "void *q", "const void *m", "const void *alpha", "void *partials"],
    "cgamd_block_update_qp": ["cgamd_ctx *ctx", "int dtype", "int size", "long long ld", "int s", "void *q", "void *p", "const void *tau_inv",
                              "const void *tau", "int init"],
}


def _header():
    return open(os.path.join(ROOT, "include", "cgamd.h")).read()


def test_header_declares_the_entries():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for entry, args in ENTRIES.items():
        m = re.search(r"\bint\s+" + entry + r"\s*\(([^;{]*)\)\s*;", code)
        assert m, f"cgamd.h does not declare {entry}"
        assert [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")] == args


def test_header_states_the_contract():
    text = re.sub(r"\s+", " ", _header().replace("*", " "))
    for phrase in ("x = X, r = Q, d = P, q = A P", "No n-sized buffer is allocated", "C = R0^T R0 = L L^T; xi = L^T; Q = R0 xi^-1; P = Q",
                   "delta_0[j] = |xi e_j|^2", "SIX launches whatever s, a linear chain", "its fused dot unused",
                   "G = L L^T, alpha = G^-1, M = alpha xi", "X += P M ; W = Q - (A P) alpha over Q", "xi <- tau xi",
                   "Q <- W tau^-1 ; P <- Q + P tau^T", "each rounded once to the value type", "one rounding per operation",
                   "Captured graphs and CGAMD_NO_GRAPH give the same bits", "iterate(a); iterate(b) gives the bits of iterate(a + b)",
                   "not v > s eps_value max_j C_jj", "2^-23 (float) or 2^-52 (double)", "a condition, not a tuned number",
                   "freezes the loop", "writes nothing", "a failed G freezes before step 4, a failed W^T W after X is updated",
                   "NaN freezes the same way", "Takes effect at the next cgamd_solver_set_rhs (x0 is allowed)",
                   "the bits of one that never had it",
                   "complex types", "batched handles, CGAMD_UNFUSED, the row-major layout, nRHS outside 2 ... 16, a preconditioner in force, shifts in force",
                   "cgamd_solver_set_shifts, cgamd_solver_iterate_tol, cgamd_solver_replace_residual and cgamd_mixed_solve",
                   "cgamd_solver_set_rhs_projected stays served", "stops ALL columns in the first iteration in which every column satisfies its own tolerance",
                   "iterations_run[r] are all equal", "a breakdown ends the call with the count reached",
                   "the result does not depend on checkEvery", "1 G failed, 2 W^T W failed", "3 NaN",
                   "14 vector passes per right-hand side", "cgamd_solver_loop_launches is 6",
                   "are neither read nor written", "p = j (j + 1) / 2 + i"):
        assert phrase in text, phrase


def test_ctypes_table_and_python_interface(pkg):
    src = inspect.getsource(pkg._lib)
    assert re.search(r'"cgamd_solver_set_block":\s*\(ci,\s*\[vp,\s*ci\]\)', src)
    assert re.search(r'"cgamd_solver_block_status":\s*\(ci,\s*\[vp,\s*ctypes\.POINTER\(ci\),\s*ctypes\.POINTER\(ctypes\.c_double\)\]\)', src)
    assert re.search(r'"cgamd_solver_block_state":\s*\(ci,\s*\[vp,\s*ci,\s*vp\]\)', src)
    assert re.search(r'"cgamd_block_gram_grid":\s*\(ci,\s*\[ci\]\)', src)
    assert re.search(r'"cgamd_block_gram":\s*\(ci,\s*\[vp,\s*ci,\s*ci,\s*ll,\s*ci,\s*vp,\s*vp,\s*vp\]\)', src)
    assert re.search(r'"cgamd_block_update_xw":\s*\(ci,\s*\[vp,\s*ci,\s*ci,\s*ll,\s*ci,\s*vp,\s*vp,\s*vp,\s*vp,\s*vp,\s*vp,\s*vp\]\)', src)
    assert re.search(r'"cgamd_block_update_qp":\s*\(ci,\s*\[vp,\s*ci,\s*ci,\s*ll,\s*ci,\s*vp,\s*vp,\s*vp,\s*vp,\s*ci\]\)', src)
    for name in ("set_block", "block_status", "block_state", "solve_block"):
        assert callable(getattr(pkg.Solver, name)), name
    assert pkg.Solver.MAX_BLOCK == 16
    p = inspect.signature(pkg.Solver.solve_block).parameters
    assert list(p) == ["self", "b", "x0", "tol", "maxit", "check_every"]
    assert (p["x0"].default, p["tol"].default, p["maxit"].default, p["check_every"].default) == (None, 1e-6, 1000, 8)
    assert inspect.signature(pkg.Solver.set_block).parameters["on"].default is True


def test_makefile_builds_the_file():
    mk = open(os.path.join(ROOT, PKG_NAME, "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    assert "block_cg.hip" in srcs and os.path.exists(os.path.join(ROOT, PKG_NAME, "csrc", "block_cg.hip"))


def test_built_library_exports_them(pkg):
    for path in (pkg.LIB_PATH, pkg.LEGACY_LIB_PATH):
        if not os.path.exists(path):
            continue                                # not built here: test_abi_and_host asks for the build
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        for entry in ENTRIES:
            assert any(line.split()[-1] == entry and " T " in line for line in out.splitlines()), (path, entry)


def test_null_handle_needs_no_device(pkg):
    lib = pkg._lib.load()
    E = pkg._lib.ERR_INVALID
    one = np.ones(4)
    info = np.zeros(4, dtype=np.intc)
    assert lib.cgamd_solver_set_block(None, 1) == E
    assert b"set_block" in lib.cgamd_last_error()
    assert lib.cgamd_solver_block_status(None, info.ctypes.data_as(pkg._lib.ctypes.POINTER(pkg._lib.ctypes.c_int)), None) == E
    assert b"block_status" in lib.cgamd_last_error()
    assert lib.cgamd_solver_block_state(None, 0, pkg._lib.ptr(one)) == E
    assert b"block_state" in lib.cgamd_last_error()
    assert lib.cgamd_block_gram_grid(0) == -E
    assert [lib.cgamd_block_gram_grid(n) for n in (1, 256, 257, 957, 512 * 256, 512 * 256 + 1, 10 ** 7)] == [1, 1, 2, 4, 512, 512, 512]
    assert lib.cgamd_block_gram(None, 1, 4, 4, 2, None, None, None) == E
    assert b"block_gram" in lib.cgamd_last_error()
    assert lib.cgamd_block_update_xw(None, 1, 4, 4, 2, None, None, None, None, None, None, None) == E
    assert b"block_update_xw" in lib.cgamd_last_error()
    assert lib.cgamd_block_update_qp(None, 1, 4, 4, 2, None, None, None, None, 0) == E
    assert b"block_update_qp" in lib.cgamd_last_error()


def _stub(pkg, dtype, n_rhs, size=4):
    """what the argument checks of Solver read, without a handle: they raise before anything touches the device"""
    s = types.SimpleNamespace(dtype=np.dtype(dtype), n_rhs=n_rhs, size=size, MAX_BLOCK=pkg.Solver.MAX_BLOCK)
    for name in ("_block_check", "_block_tolerances", "_tolerances"):
        setattr(s, name, types.MethodType(getattr(pkg.Solver, name), s))
    return s


def test_python_argument_checks(pkg):
    b = np.arange(8.0)
    for bad in (_stub(pkg, np.complex64, 2), _stub(pkg, np.complex128, 4), _stub(pkg, np.float64, 1), _stub(pkg, np.float32, 17)):
        with pytest.raises(ValueError):
            pkg.Solver.set_block(bad, True)
        with pytest.raises(ValueError):
            pkg.Solver.solve_block(bad, np.ones(bad.n_rhs * 4))
    ok = _stub(pkg, np.float32, 2)
    for kw in ({"tol": 0.0}, {"tol": -1.0}, {"tol": [1e-3, 1e-3, 1e-3]}, {"maxit": -1}, {"check_every": -1}):
        with pytest.raises(ValueError):
            pkg.Solver.solve_block(ok, b, **kw)
    with pytest.raises(ValueError):
        pkg.Solver.solve_block(ok, np.ones(7))          # not n_rhs x size values
    got, tol = ok._block_tolerances(b, 1e-3)
    assert got.dtype == np.float32 and got.flags.c_contiguous
    np.testing.assert_allclose(tol, 1e-3 * np.array([np.sqrt(14.0), np.sqrt(126.0)]), rtol=1e-12)
    _, tol = ok._block_tolerances(b, [1e-2, 1e-4])
    np.testing.assert_allclose(tol, np.array([1e-2 * np.sqrt(14.0), 1e-4 * np.sqrt(126.0)]), rtol=1e-12)
    assert ok._block_tolerances(np.zeros(8), 1e-3)[1].min() > 0       # a zero column still gets a positive tolerance
