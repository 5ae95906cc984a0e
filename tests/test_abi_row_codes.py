"""CPU tests of the row-pattern-code entry: cgamd_solver_row_codes is declared, exported by both libraries and bound; the SpMV family
names of the Python layer keep their numbers (family 7 is named from SPMV_FAMILIES_EXTRA); the two development keys exist."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _exports(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_row_codes_entry_is_declared_exported_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "cgamd.h")).read()
    assert re.search(r"^int cgamd_solver_row_codes\(cgamd_solver \*s\);", header, re.M)
    assert "cgamd_solver_row_codes" in _exports(pkg.LIB_PATH)
    assert "cgamd_solver_row_codes" in _exports(pkg.LEGACY_LIB_PATH)
    lib = pkg._lib.load()
    assert lib.cgamd_solver_row_codes.restype is ctypes.c_int and lib.cgamd_solver_row_codes.argtypes == [ctypes.c_void_p]
    assert lib.cgamd_solver_row_codes(None) == -1          # -CGAMD_ERR_INVALID, as the other code accessors answer a null handle
    assert isinstance(pkg.Solver.row_codes, property)


def test_spmv_family_names(pkg):
    assert pkg.Solver.SPMV_FAMILIES == ("stream", "rowblock", "vc", "vcp", "chunked", "spmm", "batched")
    assert pkg.Solver.SPMV_FAMILIES_EXTRA[0] == "rowcode"
    assert (pkg.Solver.SPMV_FAMILIES + pkg.Solver.SPMV_FAMILIES_EXTRA)[7] == "rowcode"


def test_row_code_keys_are_development_keys(pkg):
    lib = pkg._lib.load()
    assert lib.cgamd_tune(b"row_codes", 1) == 1 and lib.cgamd_tune(b"row_codes_min_mb", 32) == 1      # not public
    assert lib.cgamd_tune(b"dev.row_codes", 1) == 0 and lib.cgamd_tune(b"dev.row_codes_min_mb", 32) == 0      # (the defaults)
