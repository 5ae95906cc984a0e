"""CPU tests of cgamd_dist_slab_plan, the read-only report of the slab loop's plan: declared, exported by both libraries, bound, the
null-handle error.  The `cap` convention needs a handle: tests/test_gpu_slab_bits.py exercises it in every case."""
import ctypes
import importlib
import os
import re
import subprocess

from conftest import PKG_NAME

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _exports(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def _header():
    return open(os.path.join(ROOT, "include", "cgamd.h")).read()


def test_entry_is_declared_exported_and_bound(pkg):
    assert re.search(r"^int cgamd_dist_slab_plan\(cgamd_dist \*d, int info\[8\], int \*member_start, int cap\);", _header(), re.M)
    assert "cgamd_dist_slab_plan" in _exports(pkg.LIB_PATH)
    assert "cgamd_dist_slab_plan" in _exports(pkg.LEGACY_LIB_PATH)
    f = pkg._lib.load().cgamd_dist_slab_plan
    assert f.restype is ctypes.c_int
    assert f.argtypes == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    dmod = importlib.import_module(PKG_NAME + ".dist")
    assert callable(dmod.DistSolver.slab_plan)


def test_null_arguments_are_errors_and_nothing_is_written(pkg):
    f = pkg._lib.load().cgamd_dist_slab_plan
    info = (ctypes.c_int * 8)(*([-7] * 8))
    starts = (ctypes.c_int * 4)(*([-7] * 4))
    assert f(None, info, starts, 4) == -1          # -CGAMD_ERR_INVALID
    assert f(None, None, None, 0) == -1
    assert list(info) == [-7] * 8 and list(starts) == [-7] * 4

