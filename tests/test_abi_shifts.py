"""The multi-shift entries through the layers that need no GPU: the header, the ctypes table, the Makefile, the exported symbols, the
refusals a call makes before it touches a device, and the argument checks of the Python interface.  Mirrors test_abi_projection.py."""
import inspect
import os
import re
import subprocess
import types

import numpy as np
import pytest

from conftest import PKG_NAME, ROOT

ENTRIES = {
    "cgamd_solver_set_shifts": ["cgamd_solver *s", "const void *sigma", "int nShifts"],
    "cgamd_solver_shifts": ["cgamd_solver *s"],
    "cgamd_solver_get_x_shifted": ["cgamd_solver *s", "int j", "void *x", "int on_device"],
    "cgamd_solver_shift_history": ["cgamd_solver *s", "void *out", "int max_entries"],
    "cgamd_solver_shift_scalars": ["cgamd_solver *s", "int which", "void *out_host"],
    "cgamd_shift_update": ["cgamd_ctx *ctx", "int dtype", "int size", "long long ld", "int nRHS", "int nShifts", "const void *r", "void *xs",
                           "void *ds", "const void *alpha_s", "const void *beta_s", "const void *zeta_s"],
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
    for phrase in ("r_k^j = zeta_k^j r_k", "the seed's x and history keep their bits",
                   "theta' = alpha_{k-1} / (alpha_k beta_{k-1} (1 - theta) + alpha_{k-1} (1 + sigma_j alpha_k))",
                   "zeta' = zeta theta'", "alpha_j = alpha_k theta'", "beta_j = beta_k theta' theta'",
                   "x_j = x_j + alpha_j d_j", "d_j = zeta' r_{k+1} + beta_j d_j", "theta = zeta = 1", "alpha_{-1} = 1, beta_{-1} = 0",
                   "This is the RATIO form", "divides 0 / 0", "zeta = 0 only switches the r term off",
                   "in double / complex double", "each rounded once to the value type", "one rounding per operation",
                   "ONE vector launch for all shifts", "that loop's count plus 2, whatever nShifts",
                   "Captured graphs and CGAMD_NO_GRAPH give the same bits", "the SEED's delta_k per right-hand side",
                   "the bits of cgamd_solver_iterate(its_r)", "|zeta| <= 1", "nShifts 1 ... 16",
                   "sigma == NULL or nShifts == 0 removes the shifts", "the bits of one that never had any",
                   "Takes effect at the next cgamd_solver_set_rhs", "Allocates 2 nShifts nRHS ld values",
                   "A failed call leaves the handle unchanged", "layout [k][j][r]", "row 0 all ones",
                   "delta_k^j = (zeta_k^j)^2 delta_k", "unconjugated, like it",
                   "cgamd_solver_refresh_values and cgamd_solver_reload_matrix keep the shifts",
                   "batched handles, CGAMD_HERMITIAN on a complex type, CGAMD_UNFUSED, the row-major layout, and with a preconditioner in force",
                   "a preconditioned operator is not a shift of anything", "a sigma that is not finite",
                   "(except removal with NULL)", "cgamd_solver_iterate_tol, cgamd_solver_replace_residual and cgamd_solver_set_rhs_projected",
                   "CGAMD_ERR_INVALID from cgamd_solver_set_rhs with x0 != NULL", "(4 nShifts + 1) size V nRHS",
                   "are neither read nor written"):
        assert phrase in text, phrase


def test_ctypes_table_and_python_interface(pkg):
    src = inspect.getsource(pkg._lib)
    assert re.search(r'"cgamd_solver_set_shifts":\s*\(ci,\s*\[vp,\s*vp,\s*ci\]\)', src)
    assert re.search(r'"cgamd_solver_shifts":\s*\(ci,\s*\[vp\]\)', src)
    assert re.search(r'"cgamd_solver_get_x_shifted":\s*\(ci,\s*\[vp,\s*ci,\s*vp,\s*ci\]\)', src)
    assert re.search(r'"cgamd_solver_shift_history":\s*\(ci,\s*\[vp,\s*vp,\s*ci\]\)', src)
    assert re.search(r'"cgamd_solver_shift_scalars":\s*\(ci,\s*\[vp,\s*ci,\s*vp\]\)', src)
    assert re.search(r'"cgamd_shift_update":\s*\(ci,\s*\[vp,\s*ci,\s*ci,\s*ll,\s*ci,\s*ci,\s*vp,\s*vp,\s*vp,\s*vp,\s*vp,\s*vp\]\)', src)
    for name in ("set_shifts", "shifts", "x_shifted", "shift_history", "shift_scalars", "solve_shifted"):
        assert callable(getattr(pkg.Solver, name)), name
    p = inspect.signature(pkg.Solver.solve_shifted).parameters
    assert list(p)[:5] == ["self", "b", "sigmas", "iterations", "tol"] and p["iterations"].default is None and p["tol"].default is None


def test_makefile_builds_the_file():
    mk = open(os.path.join(ROOT, PKG_NAME, "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    assert "shifts.hip" in srcs and os.path.exists(os.path.join(ROOT, PKG_NAME, "csrc", "shifts.hip"))


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
    one = np.ones(1)
    assert lib.cgamd_solver_set_shifts(None, pkg._lib.ptr(one), 1) == E
    assert b"set_shifts" in lib.cgamd_last_error()
    assert lib.cgamd_solver_shifts(None) == -E
    assert lib.cgamd_solver_get_x_shifted(None, 0, pkg._lib.ptr(one), 0) == E
    assert b"get_x_shifted" in lib.cgamd_last_error()
    assert lib.cgamd_solver_shift_history(None, pkg._lib.ptr(one), 1) == -E
    assert b"shift_history" in lib.cgamd_last_error()
    assert lib.cgamd_solver_shift_scalars(None, 0, pkg._lib.ptr(one)) == E
    assert b"shift_scalars" in lib.cgamd_last_error()
    assert lib.cgamd_shift_update(None, 1, 4, 4, 1, 1, None, None, None, None, None, None) == E
    assert b"shift_update" in lib.cgamd_last_error()


def _stub(pkg, dtype, n_rhs=1):
    """what the argument checks of Solver read, without a handle: they raise before anything touches the device"""
    s = types.SimpleNamespace(dtype=np.dtype(dtype), n_rhs=n_rhs, MAX_SHIFTS=pkg.Solver.MAX_SHIFTS)
    s._shift_values = types.MethodType(pkg.Solver._shift_values, s)
    s._tolerances = types.MethodType(pkg.Solver._tolerances, s)
    return s


def test_python_argument_checks(pkg):
    assert pkg.Solver.MAX_SHIFTS == 16
    real, cplx = _stub(pkg, np.float32), _stub(pkg, np.complex128)
    got = real._shift_values([0.5, 2])
    assert got.dtype == np.float32 and got.tolist() == [0.5, 2.0] and got.flags.c_contiguous
    assert real._shift_values(np.array([1 + 0j])).dtype == np.float32        # a complex array without an imaginary part
    got = cplx._shift_values([0.5, 1 - 2j])
    assert got.dtype == np.complex128 and got.tolist() == [0.5, 1 - 2j]
    for bad in ([], np.zeros(17), [1.0, np.inf], [np.nan]):
        with pytest.raises(ValueError):
            real._shift_values(bad)
    with pytest.raises(ValueError):
        real._shift_values([1 + 1j])                # a complex shift on a real handle
    with pytest.raises(ValueError):
        cplx._shift_values([complex(0, np.inf)])
    b = np.ones(4)
    for kw in ({}, {"iterations": 3, "tol": 1e-3}, {"iterations": -1}, {"tol": 0.0}, {"tol": [1e-3, 1e-3]}):
        with pytest.raises(ValueError):
            pkg.Solver.solve_shifted(real, b, [1.0], **kw)
    with pytest.raises(ValueError):
        pkg.Solver.solve_shifted(real, b, [], iterations=3)
