"""The preconditioners of the row-partitioned handle (cgamd_dist_set_preconditioner, _jacobi, _line; DistSolver.set_preconditioner;
dist.pcg_loop) through the layers that need no GPU: header, ctypes table, exported symbols, Makefile, argument checks."""
import importlib
import inspect
import os
import re
import subprocess
import types

import pytest

from conftest import ROOT, PKG_NAME

ENTRIES = {
    "cgamd_dist_set_preconditioner": (["cgamd_dist *d", "const void *m_local"], ["vp", "vp"]),
    "cgamd_dist_set_preconditioner_jacobi": (["cgamd_dist *d"], ["vp"]),
    "cgamd_dist_set_preconditioner_line": (["cgamd_dist *d", "int stride"], ["vp", "ci"]),
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


def test_makefile_builds_the_shared_setup_unit():
    mk = open(os.path.join(ROOT, PKG_NAME, "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    assert "precond_setup.cpp" in srcs
    assert os.path.exists(os.path.join(ROOT, PKG_NAME, "csrc", "precond_setup.cpp"))


def test_null_handles_are_rejected(pkg):
    lib = pkg._lib.load()
    assert lib.cgamd_dist_set_preconditioner(None, None) == pkg._lib.ERR_INVALID
    assert lib.cgamd_dist_set_preconditioner_jacobi(None) == pkg._lib.ERR_INVALID
    assert lib.cgamd_dist_set_preconditioner_line(None, 1) == pkg._lib.ERR_INVALID


def test_dist_solver_set_preconditioner_rejects_other_arguments(pkg):
    """the argument is checked before any C call or collective: no handle is needed to see it"""
    dmod = importlib.import_module(PKG_NAME + ".dist")
    assert callable(dmod.pcg_loop)
    assert list(inspect.signature(dmod.pcg_loop).parameters) == ["ops", "comm", "plan", "b_local", "x0_local", "n_iterations", "apply_m"]
    s = object.__new__(dmod.DistSolver)
    s._lib, s.handle, s.plan, s.dtype = pkg._lib.load(), None, types.SimpleNamespace(n_local=10, world=1), None
    for bad in ("ilu", "line", ("line",), ("line", 1.5), ("line", "1"), ("rows", 2), ("line", 1, 2), 3, 2.5, [1.0, 2.0], ("line", True)):
        with pytest.raises(ValueError):
            s.set_preconditioner(bad)
    s.handle = None         # (nothing to close)
