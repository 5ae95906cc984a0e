"""The preconditioned block CG entries through the layers that need no GPU: the header, the ctypes table, the Makefile, the exported
symbols, the refusals a call makes before it touches a device, and the argument checks of the Python interface.  Mirrors
test_abi_block.py."""
import inspect
import os
import re
import subprocess
import types

import numpy as np
import pytest

from conftest import PKG_NAME, ROOT

ENTRIES = {
    "cgamd_solver_set_block_pcg": ["cgamd_solver *s", "int on"],
    "cgamd_block_gram_weighted": ["cgamd_ctx *ctx", "int dtype", "int size", "long long ld", "int s", "const void *w", "const void *m", "void *partials"],
    "cgamd_block_update_qp_z": ["cgamd_ctx *ctx", "int dtype", "int size", "long long ld", "int s", "void *q", "void *p", "const void *z", "const void *m",
                                "const void *tau_inv", "const void *tau", "int init"],
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
    for phrase in ("R = Q xi with Q^T M^-1 Q = I", "q's storage also holds Z = M^-1 W", "No n-sized buffer is added",
                   "Z0 = M^-1 R0 into q; C = R0^T Z0 = L L^T; xi = L^T; Q = R0 xi^-1; P = Z0 xi^-1", "delta_0[j] = (R0^T R0)_jj",
                   "for a diagonal M NOTHING runs here", "w_i . (m w_j) with m w_j rounded once in the value type",
                   "delta_k[j] = (xi e_j)^T (W^T W) (xi e_j) with the OLD xi", "Q <- W tau^-1 ; P <- Z tau^-1 + P tau^T",
                   "cgamd_solver_loop_launches is 7 plus the launches of z = M^-1 w (0 for a diagonal M)",
                   "Captured graphs and CGAMD_NO_GRAPH give the same bits", "iterate(a); iterate(b) gives the bits of iterate(a + b)",
                   "not v > s eps_value max_j C_jj", "freezes the loop with status 2", "run unguarded", "legal only WITH a preconditioner in force",
                   "the bits of the scalar PCG handle it was", "and on CGAMD_HERMITIAN", "exclude each other", "removal with NULL too",
                   "cgamd_solver_set_rhs_projected stays served", "rebuild an M that was built from the matrix", "info[0] is 2 for the preconditioned one",
                   "which = 7 is W^T Z as summed; 4 stays W^T W", "15, and m read twice", "17, and the preconditioner's own bytes",
                   "exactly one of z (the block) and m"):
        assert phrase in text, phrase
    # what the block CG section pinned stays as it was
    for phrase in ("a preconditioner in force, shifts in force", "(except removal with NULL)", "cgamd_solver_loop_launches is 6"):
        assert phrase in text, phrase


def test_ctypes_table_and_python_interface(pkg):
    src = inspect.getsource(pkg._lib)
    assert re.search(r'"cgamd_solver_set_block_pcg":\s*\(ci,\s*\[vp,\s*ci\]\)', src)
    assert re.search(r'"cgamd_block_gram_weighted":\s*\(ci,\s*\[vp,\s*ci,\s*ci,\s*ll,\s*ci,\s*vp,\s*vp,\s*vp\]\)', src)
    assert re.search(r'"cgamd_block_update_qp_z":\s*\(ci,\s*\[vp,\s*ci,\s*ci,\s*ll,\s*ci,\s*vp,\s*vp,\s*vp,\s*vp,\s*vp,\s*vp,\s*ci\]\)', src)
    for name in ("set_block_pcg", "solve_block_pcg"):
        assert callable(getattr(pkg.Solver, name)), name
    p = inspect.signature(pkg.Solver.solve_block_pcg).parameters
    assert list(p) == ["self", "b", "M", "x0", "tol", "maxit", "check_every"]
    assert p["M"].default is inspect.Parameter.empty
    assert (p["x0"].default, p["tol"].default, p["maxit"].default, p["check_every"].default) == (None, 1e-6, 1000, 8)
    assert inspect.signature(pkg.Solver.set_block_pcg).parameters["on"].default is True
    # set_block's and solve_block's signatures do not change
    assert list(inspect.signature(pkg.Solver.solve_block).parameters) == ["self", "b", "x0", "tol", "maxit", "check_every"]
    assert list(inspect.signature(pkg.Solver.set_block).parameters) == ["self", "on"]


def test_makefile_builds_the_file():
    mk = open(os.path.join(ROOT, PKG_NAME, "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    assert "block_pcg.hip" in srcs and os.path.exists(os.path.join(ROOT, PKG_NAME, "csrc", "block_pcg.hip"))
    assert "block_cg.hip" in srcs


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
    for on in (0, 1):
        assert lib.cgamd_solver_set_block_pcg(None, on) == E
        assert b"set_block_pcg" in lib.cgamd_last_error()
    assert lib.cgamd_block_gram_weighted(None, 1, 4, 4, 2, None, None, None) == E
    assert b"block_gram_weighted" in lib.cgamd_last_error()
    assert lib.cgamd_block_update_qp_z(None, 1, 4, 4, 2, None, None, None, None, None, None, 0) == E
    assert b"block_update_qp_z" in lib.cgamd_last_error()


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
            pkg.Solver.set_block_pcg(bad, True)
        with pytest.raises(ValueError):
            pkg.Solver.solve_block_pcg(bad, np.ones(bad.n_rhs * 4), "jacobi")
    ok = _stub(pkg, np.float32, 2)
    for kw in ({"tol": 0.0}, {"tol": -1.0}, {"tol": [1e-3, 1e-3, 1e-3]}, {"maxit": -1}, {"check_every": -1}):
        with pytest.raises(ValueError):
            pkg.Solver.solve_block_pcg(ok, b, "jacobi", **kw)
    with pytest.raises(ValueError):
        pkg.Solver.solve_block_pcg(ok, np.ones(7), "jacobi")          # not n_rhs x size values
    with pytest.raises(TypeError):
        pkg.Solver.solve_block_pcg(ok, b)                              # M has no default: None is said, not implied
