"""The preconditioners built from the handle's own matrix (cgamd_solver_set_preconditioner_line / _jacobi and
cgamd_solver_preconditioner_source) through the layers that need no GPU: header, ctypes table, exported symbols, Makefile."""
import inspect
import os
import re
import subprocess

import pytest

from conftest import ROOT, PKG_NAME

ENTRIES = {
    "cgamd_solver_set_preconditioner_line": (["cgamd_solver *s", "int stride"], ["vp", "ci"]),
    "cgamd_solver_set_preconditioner_jacobi": (["cgamd_solver *s"], ["vp"]),
    "cgamd_solver_preconditioner_source": (["cgamd_solver *s"], ["vp"]),
}


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_header_declares_the_entry(entry):
    src = open(os.path.join(ROOT, "include", "cgamd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + entry + r"\s*\(([^;{]*)\)\s*;", src)
    assert m, f"cgamd.h does not declare {entry}"
    args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
    assert args == ENTRIES[entry][0]


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_ctypes_table_lists_the_entry(pkg, entry):
    src = inspect.getsource(pkg._lib)
    m = re.search(r'"' + entry + r'":\s*\(ci,\s*\[([^\]]*)\]\)', src)
    assert m, f"_lib.py does not list {entry}"
    assert [a.strip() for a in m.group(1).split(",")] == ENTRIES[entry][1]


def test_built_library_exports_them(pkg):
    for path in (pkg.LIB_PATH, pkg.LEGACY_LIB_PATH):
        if not os.path.exists(path):
            continue                                # not built here: test_abi_and_host asks for the build
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        for entry, (_, argtypes) in ENTRIES.items():
            assert any(line.split()[-1] == entry and " T " in line for line in out.splitlines()), (path, entry)
            assert len(getattr(pkg._lib.load(), entry).argtypes) == len(argtypes)


def test_makefile_builds_the_kernel_file():
    mk = open(os.path.join(ROOT, PKG_NAME, "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    assert "precond_build.hip" in srcs
    assert os.path.exists(os.path.join(ROOT, PKG_NAME, "csrc", "precond_build.hip"))


def test_host_route_switch_is_a_dev_key(pkg):
    """dev.line_host_route exists and is no public key (the public table stays at 15, test_abi_and_host)"""
    lib = pkg._lib.load()
    assert lib.cgamd_tune(b"line_host_route", 1) == pkg._lib.ERR_INVALID
    assert lib.cgamd_tune(b"dev.line_host_route", 0) == 0


def test_null_handles_are_rejected(pkg):
    lib = pkg._lib.load()
    assert lib.cgamd_solver_set_preconditioner_line(None, 1) == pkg._lib.ERR_INVALID
    assert lib.cgamd_solver_set_preconditioner_jacobi(None) == pkg._lib.ERR_INVALID
    assert lib.cgamd_solver_preconditioner_source(None) == 0
