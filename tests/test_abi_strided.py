"""The strided tridiagonal preconditioner's entry through the layers that need no GPU: header, ctypes table, exported symbol,
Makefile."""
import inspect
import os
import re
import subprocess

from conftest import ROOT, PKG_NAME

ENTRY = "cgamd_solver_set_preconditioner_tridiag_strided"


def test_header_declares_the_strided_entry():
    src = open(os.path.join(ROOT, "include", "cgamd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + ENTRY + r"\s*\(([^;{]*)\)\s*;", src)
    assert m, f"cgamd.h does not declare {ENTRY}"
    args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
    assert args == ["cgamd_solver *s", "int stride", "const void *lower", "const void *diag", "const void *upper", "int on_device"]


def test_ctypes_table_lists_it_with_six_arguments(pkg):
    src = inspect.getsource(pkg._lib)
    m = re.search(r'"' + ENTRY + r'":\s*\(ci,\s*\[([^\]]*)\]\)', src)
    assert m, f"_lib.py does not list {ENTRY}"
    assert [a.strip() for a in m.group(1).split(",")] == ["vp", "ci", "vp", "vp", "vp", "ci"]


def test_built_library_exports_it(pkg):
    for path in (pkg.LIB_PATH, pkg.LEGACY_LIB_PATH):
        if not os.path.exists(path):
            continue                                # not built here: test_abi_and_host asks for the build
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        assert any(line.split()[-1] == ENTRY and " T " in line for line in out.splitlines()), path
        fn = getattr(pkg._lib.load(), ENTRY)
        assert len(fn.argtypes) == 6


def test_makefile_builds_the_kernel_file():
    mk = open(os.path.join(ROOT, PKG_NAME, "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    assert "precond_strided.hip" in srcs
    assert os.path.exists(os.path.join(ROOT, PKG_NAME, "csrc", "precond_strided.hip"))
