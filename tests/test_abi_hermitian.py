"""CGAMD_HERMITIAN (the conjugated recurrence for complex Hermitian positive-definite matrices) through the layers that need no GPU:
the header, the ctypes table, the exported symbols, the entry that needs no handle, the host restatement the GPU tests compare against
(herm_ref) and the refusal DistSolver makes before it touches a device.  Mirrors test_abi_until.py."""
import ctypes
import importlib
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import herm_ref
from conftest import ROOT

ENTRIES = {"cgamd_solver_hermitian": ["cgamd_solver *s"],
           "cgamd_solver_hermitian_scalars": ["cgamd_solver *s", "void *alpha_host", "void *beta_host"]}


def _header():
    return open(os.path.join(ROOT, "include", "cgamd.h")).read()


def test_header_declares_the_flag_and_the_accessors():
    src = _header()
    m = re.search(r"^#define\s+CGAMD_HERMITIAN\s+(\d+)\b", src, flags=re.M)
    assert m and int(m.group(1)) == 16
    others = {name: int(v) for name, v in re.findall(r"^#define\s+(CGAMD_[A-Z0-9_]+)\s+(\d+)\s+/\*", src, flags=re.M)
              if name != "CGAMD_HERMITIAN" and name != "CGAMD_H"}
    assert others and all(v & 16 == 0 for v in others.values()), others        # the bit was free among the flags
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for entry, args in ENTRIES.items():
        m = re.search(r"\bint\s+" + entry + r"\s*\(([^;{]*)\)\s*;", code)
        assert m, f"cgamd.h does not declare {entry}"
        assert [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")] == args


def test_header_states_the_contract():
    text = re.sub(r"\s+", " ", _header().replace("*", " "))
    for phrase in ("sum conj(a_i) b_i", "alpha = rho / Re(d^H q)", "cgamd_solver_loop_launches() == 4", "neither is validated",
                   "CGAMD_UNFUSED | CGAMD_HERMITIAN", "12 vector passes, 14 with a diagonal M"):
        assert phrase in text, phrase


def test_python_constant_and_ctypes_table(pkg):
    assert pkg._lib.HERMITIAN == 16
    src = inspect.getsource(pkg._lib)
    assert re.search(r'"cgamd_solver_hermitian":\s*\(ci,\s*\[vp\]\)', src)
    assert re.search(r'"cgamd_solver_hermitian_scalars":\s*\(ci,\s*\[vp,\s*vp,\s*vp\]\)', src)
    sig = inspect.signature(pkg.Solver.__init__)
    assert sig.parameters["hermitian"].default is False
    assert isinstance(pkg.Solver.hermitian, property)


def test_built_library_exports_them(pkg):
    for path in (pkg.LIB_PATH, pkg.LEGACY_LIB_PATH):
        if not os.path.exists(path):
            continue                                # not built here: test_abi_and_host asks for the build
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        for entry in ENTRIES:
            assert any(line.split()[-1] == entry and " T " in line for line in out.splitlines()), (path, entry)


def test_null_handle_needs_no_device(pkg):
    lib = pkg._lib.load()
    assert lib.cgamd_solver_hermitian(None) < 0
    assert lib.cgamd_solver_hermitian_scalars(None, None, None) == pkg._lib.ERR_INVALID


def test_the_restatement_solves_the_7x5_system():
    """herm_ref.cg is CG: on the 35-row system it reaches numpy.linalg.solve's answer, with a real, decreasing-to-zero history"""
    A = herm_ref.magnetic(7, 5, 0.13, 0.05)
    dense = A.toarray()
    assert np.array_equal(dense, dense.conj().T) and not np.allclose(dense, dense.T)
    assert np.linalg.eigvalsh(dense).min() > 0
    rng = np.random.default_rng(7)
    b = rng.standard_normal(35) + 1j * rng.standard_normal(35)
    want = np.linalg.solve(dense, b)
    for m in (None, 1.0 / dense.diagonal().real):
        out = herm_ref.cg(A, b, 35, m=m)
        assert np.linalg.norm(out["x"] - want) / np.linalg.norm(want) < 1e-12
        assert out["history"].dtype == np.float64 and np.all(out["history"] >= 0) and out["history"][-1] < 1e-24 * out["history"][0]
        assert out["alpha"].dtype == np.float64 and out["beta"].dtype == np.float64
    stop = herm_ref.cg(A, b, 35, tol=1e-4 * np.linalg.norm(b))
    assert 0 < stop["its"] < 35 and np.sqrt(stop["history"][-1]) < 1e-4 * np.linalg.norm(b) <= np.sqrt(stop["history"][-2])
    assert np.array_equal(stop["history"], herm_ref.cg(A, b, stop["its"])["history"])


def test_the_unconjugated_recurrence_does_not_solve_it():
    """what the flag is for: the same loop with a.b in place of a^H b stalls on the 33 x 29 system (the issue's table: never below 0.35)"""
    A = herm_ref.magnetic(33, 29, 0.13, 0.05)
    rng = np.random.default_rng(1)
    b = rng.standard_normal(957) + 1j * rng.standard_normal(957)
    x, r = np.zeros_like(b), b.copy()
    d, dn, best = r.copy(), r @ r, 1.0
    for _ in range(40):
        q = A @ d
        al = dn / (d @ q)
        x, r = x + al * d, r - al * q
        dn, do = r @ r, dn
        d = r + (dn / do) * d
        best = min(best, np.linalg.norm(b - A @ x) / np.linalg.norm(b))
    assert best > 0.1
    out = herm_ref.cg(A, b, 20)
    assert np.linalg.norm(b - A @ out["x"]) / np.linalg.norm(b) < 1e-5


def test_dist_solver_refuses_the_flag_before_any_device(pkg):
    D = importlib.import_module(pkg.__name__ + ".dist").DistSolver
    with pytest.raises(ValueError, match="HERMITIAN"):
        D(None, None, None, None, np.complex128, flags=pkg._lib.HERMITIAN)
    with pytest.raises(ValueError, match="HERMITIAN"):
        D(None, None, None, None, np.complex128, flags=pkg._lib.HERMITIAN | pkg._lib.DIST_P2P, comm="p2p")
    lib = pkg._lib.load()       # the C entry as well: it judges the flag before it looks at the context
    out = ctypes.c_void_p()
    assert lib.cgamd_dist_create(None, None, 0, 1, 3, 4, 0, 4, None, None, None, 0, None, None, None, None, pkg._lib.HERMITIAN,
                                 ctypes.byref(out)) == pkg._lib.ERR_INVALID
    assert b"CGAMD_HERMITIAN" in lib.cgamd_last_error()
