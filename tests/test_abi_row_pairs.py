"""CPU tests of the row-pair SpMV's interface: cgamd_solver_row_pairs is declared, exported by both libraries and bound with its ctypes
signature, a null handle is answered like by the other code accessors; dev.row_pairs and dev.row_pairs_min_mb are development keys;
family 8 is named "rowpair" and the earlier families keep their numbers."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _exports(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_row_pairs_entry_is_declared_exported_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "cgamd.h")).read()
    assert re.search(r"^int cgamd_solver_row_pairs\(cgamd_solver \*s\);", header, re.M)
    assert "cgamd_solver_row_pairs" in _exports(pkg.LIB_PATH)
    assert "cgamd_solver_row_pairs" in _exports(pkg.LEGACY_LIB_PATH)
    lib = pkg._lib.load()
    assert lib.cgamd_solver_row_pairs.restype is ctypes.c_int and lib.cgamd_solver_row_pairs.argtypes == [ctypes.c_void_p]
    assert lib.cgamd_solver_row_pairs(None) == -1         # -CGAMD_ERR_INVALID
    assert isinstance(pkg.Solver.row_pairs, property)


def test_row_pairs_keys_are_development_keys(pkg):
    lib = pkg._lib.load()
    assert lib.cgamd_tune(b"row_pairs", 1) == 1           # not public
    assert lib.cgamd_tune(b"row_pairs_min_mb", 256) == 1
    try:
        assert all(lib.cgamd_tune(b"dev.row_pairs", v) == 0 for v in (1, 0))
        assert all(lib.cgamd_tune(b"dev.row_pairs", v) == 1 for v in (2, -2, 7))
        assert lib.cgamd_tune(b"dev.row_pairs_min_mb", 0) == 0
    finally:
        assert lib.cgamd_tune(b"dev.row_pairs", -1) == 0  # (the defaults: the rule by value size, 256 MB)
        assert lib.cgamd_tune(b"dev.row_pairs_min_mb", 256) == 0


def test_family_names_keep_their_numbers(pkg):
    names = pkg.Solver.SPMV_FAMILIES + pkg.Solver.SPMV_FAMILIES_EXTRA
    assert pkg.Solver.SPMV_FAMILIES_EXTRA == ("rowcode", "rowpair")
    assert names[7] == "rowcode" and names[8] == "rowpair" and len(names) == 9
