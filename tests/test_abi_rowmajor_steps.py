"""CPU tests of cgamd_solver_rowmajor_plan, the read-only record of what the row-major loop launches: declared, exported by both
libraries, bound with the header's signature, loud about null arguments (nothing is written then).  What it reports needs a handle:
tests/test_gpu_rowmajor_steps.py asserts it in every case."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _exports(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def _header():
    return open(os.path.join(ROOT, "include", "cgamd.h")).read()


def test_entry_is_declared_exported_and_bound(pkg):
    assert re.search(r"^int cgamd_solver_rowmajor_plan\(cgamd_solver \*s, int \*out, int n_out\);", _header(), re.M)
    assert "cgamd_solver_rowmajor_plan" in _exports(pkg.LIB_PATH)
    assert "cgamd_solver_rowmajor_plan" in _exports(pkg.LEGACY_LIB_PATH)
    f = pkg._lib.load().cgamd_solver_rowmajor_plan
    assert f.restype is ctypes.c_int
    assert f.argtypes == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    assert callable(pkg.Solver.rowmajor_plan)
    assert len(pkg.Solver.ROWMAJOR_PLAN_FIELDS) == 17 and len(set(pkg.Solver.ROWMAJOR_PLAN_FIELDS)) == 17
    assert "min(n_out, 17)" in _header()


def test_host_restatement_names_the_same_fields(pkg):
    import rowmajor_ref as M
    assert tuple(M.PLAN_KEYS) == tuple(pkg.Solver.ROWMAJOR_PLAN_FIELDS)
    ip, _ = M.pattern("grid5")
    assert set(M.host_plan(ip, "float64", 16)) == set(M.PLAN_KEYS)


def test_null_arguments_are_errors_and_nothing_is_written(pkg):
    lib = pkg._lib.load()
    f = lib.cgamd_solver_rowmajor_plan
    out = (ctypes.c_int * 17)(*([-7] * 17))
    assert f(None, out, 17) == -1 and b"rowmajor_plan" in lib.cgamd_last_error()          # -CGAMD_ERR_INVALID
    assert f(None, None, 0) == -1
    assert list(out) == [-7] * 17
