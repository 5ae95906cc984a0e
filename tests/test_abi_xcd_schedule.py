"""CPU tests of the plane-matched schedule's interface: cgamd_solver_spmv_schedule is declared, exported by both libraries and bound
with its ctypes signature, a null handle is an error that writes nothing; dev.spmv_plane is a development key that takes -1, 0 and 1;
Solver.spmv_schedule is a property and last_spmv_form() keeps its fields."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _exports(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_spmv_schedule_entry_is_declared_exported_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "cgamd.h")).read()
    assert re.search(r"^int cgamd_solver_spmv_schedule\(cgamd_solver \*s, int \*kind, int \*grid, long long \*unit_rows\);", header, re.M)
    assert "cgamd_solver_spmv_schedule" in _exports(pkg.LIB_PATH)
    assert "cgamd_solver_spmv_schedule" in _exports(pkg.LEGACY_LIB_PATH)
    lib = pkg._lib.load()
    f = lib.cgamd_solver_spmv_schedule
    assert f.restype is ctypes.c_int
    assert f.argtypes == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_longlong)]
    kind, grid, unit = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_longlong(-7)
    assert f(None, ctypes.byref(kind), ctypes.byref(grid), ctypes.byref(unit)) == 1         # CGAMD_ERR_INVALID
    assert (kind.value, grid.value, unit.value) == (-7, -7, -7)
    assert b"spmv_schedule" in lib.cgamd_last_error()
    assert isinstance(pkg.Solver.spmv_schedule, property)


def test_spmv_plane_is_a_development_key(pkg):
    lib = pkg._lib.load()
    assert lib.cgamd_tune(b"spmv_plane", 1) == 1            # not public
    try:
        assert all(lib.cgamd_tune(b"dev.spmv_plane", v) == 0 for v in (1, 0))
        assert all(lib.cgamd_tune(b"dev.spmv_plane", v) == 1 for v in (2, -2, 7))
    finally:
        assert lib.cgamd_tune(b"dev.spmv_plane", -1) == 0   # (the default: the rule)


def test_last_spmv_form_keeps_its_fields(pkg):
    assert pkg.Solver.SPMV_FORM_FIELDS == ("family", "vec", "width", "index_bits", "value_codes", "nt", "fused", "wide", "grid", "partials")
