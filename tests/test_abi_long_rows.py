"""CPU tests of the CGAMD_SPLIT_LONG_ROWS interface: the flag, cgamd_solver_long_rows and the two tuning keys are declared, exported by
both libraries and bound; the flag's bit is no other create flag's."""
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


def test_flag_collides_with_no_other_create_flag(pkg):
    flags = {}
    for name, value in re.findall(r"^#define (CGAMD_[A-Z0-9_]+) (\d+)\s+/\*", _header(), re.M):
        if re.match(r"CGAMD_(F32|F64|C64|C128|OK|ERR_)", name):
            continue
        flags[name] = int(value)
    assert {"CGAMD_MATRIX_ON_DEVICE", "CGAMD_NO_GRAPH", "CGAMD_UNFUSED", "CGAMD_HERMITIAN", "CGAMD_DIST_GRAPH", "CGAMD_DIST_RESIDENT",
            "CGAMD_SPLIT_LONG_ROWS"} <= set(flags)
    mine = flags.pop("CGAMD_SPLIT_LONG_ROWS")
    assert mine > 0 and mine & (mine - 1) == 0
    assert all(mine & v == 0 for v in flags.values()), flags
    assert pkg._lib.SPLIT_LONG_ROWS == mine


def test_entry_is_declared_exported_and_bound(pkg):
    assert re.search(r"^int cgamd_solver_long_rows\(cgamd_solver \*s, int \*out, int n_out\);", _header(), re.M)
    assert "cgamd_solver_long_rows" in _exports(pkg.LIB_PATH)
    assert "cgamd_solver_long_rows" in _exports(pkg.LEGACY_LIB_PATH)
    lib = pkg._lib.load()
    f = lib.cgamd_solver_long_rows
    assert f.restype is ctypes.c_int and f.argtypes == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    out = (ctypes.c_int * 6)()
    assert f(None, out, 6) == -1          # -CGAMD_ERR_INVALID
    assert isinstance(pkg.Solver.long_rows, property)
    names = pkg.Solver.SPMV_FAMILIES + pkg.Solver.SPMV_FAMILIES_EXTRA + pkg.Solver.SPMV_FAMILIES_SPLIT
    assert names[9] == "split" and len(names) == 10


def test_tuning_keys(pkg):
    lib = pkg._lib.load()
    for key in (b"dev.long_row_bytes", b"dev.long_row_segment"):
        assert lib.cgamd_tune(key[4:], 0) == 1            # not public
        assert lib.cgamd_tune(key, 0) == 0                # (the default)
    try:
        assert lib.cgamd_tune(b"dev.long_row_bytes", -1) == 1
        assert lib.cgamd_tune(b"dev.long_row_bytes", 2400) == 0
        assert all(lib.cgamd_tune(b"dev.long_row_segment", v) == 0 for v in (256, 1024, 8192))
        assert all(lib.cgamd_tune(b"dev.long_row_segment", v) == 1 for v in (-4, 255, 2050))
    finally:
        assert lib.cgamd_tune(b"dev.long_row_bytes", 0) == 0 and lib.cgamd_tune(b"dev.long_row_segment", 0) == 0
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "dev.long_row_bytes" in doc and "dev.long_row_segment" in doc
