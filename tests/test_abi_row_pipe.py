"""CPU tests of the row-coded SpMV's pipeline-depth entry: cgamd_solver_row_pipe is declared, exported by both libraries and bound with
its ctypes signature, a null handle is answered like by the other code accessors, and dev.row_pipe is a development key."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _exports(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_row_pipe_entry_is_declared_exported_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "cgamd.h")).read()
    assert re.search(r"^int cgamd_solver_row_pipe\(cgamd_solver \*s\);", header, re.M)
    assert "cgamd_solver_row_pipe" in _exports(pkg.LIB_PATH)
    assert "cgamd_solver_row_pipe" in _exports(pkg.LEGACY_LIB_PATH)
    lib = pkg._lib.load()
    assert lib.cgamd_solver_row_pipe.restype is ctypes.c_int and lib.cgamd_solver_row_pipe.argtypes == [ctypes.c_void_p]
    assert lib.cgamd_solver_row_pipe(None) == -1          # -CGAMD_ERR_INVALID
    assert isinstance(pkg.Solver.row_pipe, property)


def test_row_pipe_key_is_a_development_key(pkg):
    lib = pkg._lib.load()
    assert lib.cgamd_tune(b"row_pipe", 0) == 1            # not public
    assert lib.cgamd_tune(b"dev.row_pipe", 0) == 0        # (the default)


def test_row_pipe_takes_the_depths_only(pkg):
    lib = pkg._lib.load()
    try:
        assert all(lib.cgamd_tune(b"dev.row_pipe", v) == 0 for v in (1, 2, 4))
        assert all(lib.cgamd_tune(b"dev.row_pipe", v) == 1 for v in (-1, 3, 8))
    finally:
        assert lib.cgamd_tune(b"dev.row_pipe", 0) == 0
