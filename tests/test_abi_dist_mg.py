"""Multigrid on the row-partitioned handle (cgamd_dist_set_preconditioner_multigrid, _amg, cgamd_dist_mg_*; DistSolver.
set_preconditioner, mg_levels, mg_apply) through the layers that need no GPU: header, ctypes table, exported symbols, Makefile,
argument checks."""
import importlib
import os
import inspect
import re
import subprocess
import types

import pytest

from conftest import ROOT, PKG_NAME

ENTRIES = {
    "cgamd_dist_set_preconditioner_multigrid": (["cgamd_dist *d", "int nx", "int ny", "int nz", "int smooth_steps", "double over_correction",
                                                 "int min_rows"], ["vp", "ci", "ci", "ci", "ci", "ctypes.c_double", "ci"]),
    "cgamd_dist_set_preconditioner_amg": (["cgamd_dist *d", "int passes", "double strength", "int smooth_steps", "double over_correction",
                                           "int min_rows"], ["vp", "ci", "ctypes.c_double", "ci", "ctypes.c_double", "ci"]),
    "cgamd_dist_mg_levels": (["cgamd_dist *d"], ["vp"]),
    "cgamd_dist_mg_level": (["cgamd_dist *d", "int level", "long long info[6]"], ["vp", "ci", "ctypes.POINTER(ll)"]),
    "cgamd_dist_mg_level_matrix": (["cgamd_dist *d", "int level", "int *ptr", "int *cols", "void *vals"], ["vp", "ci", "vp", "vp", "vp"]),
    "cgamd_dist_mg_apply": (["cgamd_dist *d", "const void *r_dev", "void *z_dev"], ["vp", "vp", "vp"]),
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
    m = re.search(r'"' + entry + r'":\s*\(ci,\s*\[(.*)\]\)', src)
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


def test_makefile_builds_the_cut_kernels():
    mk = open(os.path.join(ROOT, PKG_NAME, "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    assert "dist_cut.hip" in srcs
    src = open(os.path.join(ROOT, PKG_NAME, "csrc", "dist_cut.hip")).read()
    assert "atomic" not in re.sub(r"//.*", "", src)            # a fixed order: the bits are the same on every run
    for kernel in ("cut_count_kernel", "cut_fill_kernel"):
        assert re.search(r"__global__[^;{]*\b" + kernel + r"\b", src), kernel


def test_null_handles_are_rejected(pkg):
    lib, L = pkg._lib.load(), pkg._lib
    assert lib.cgamd_dist_set_preconditioner_multigrid(None, 2, 2, 2, 0, 0.0, 0) == L.ERR_INVALID
    assert lib.cgamd_dist_set_preconditioner_amg(None, 0, 0.0, 0, 0.0, 0) == L.ERR_INVALID
    assert lib.cgamd_dist_mg_levels(None) == -L.ERR_INVALID
    assert lib.cgamd_dist_mg_level(None, 0, None) == L.ERR_INVALID
    assert lib.cgamd_dist_mg_level_matrix(None, 0, None, None, None) == L.ERR_INVALID
    assert lib.cgamd_dist_mg_apply(None, None, None) == L.ERR_INVALID


def test_dist_solver_takes_the_single_solvers_spellings(pkg):
    """the argument is checked before any C call or collective: no handle is needed to see what is refused, and the accepted
    spellings reach the C entry (which refuses the NULL handle)"""
    dmod = importlib.import_module(PKG_NAME + ".dist")
    for name in ("mg_levels", "mg_apply", "local_grid_dims"):
        assert callable(getattr(dmod.DistSolver, name, None) or getattr(dmod, name, None)), name
    s = object.__new__(dmod.DistSolver)
    s._lib, s.handle, s.plan, s.dtype = pkg._lib.load(), None, types.SimpleNamespace(n_local=10, world=1), None
    for bad in ("multigrid", ("multigrid",), ("multigrid", 5), ("multigrid", (5, 2), 3), ("multigrid", (5, 2.0)), ("multigrid", (5, 2, 1, 1)),
                ("multigrid", (5, 2), {"rows": 2}), ("multigrid", (5, 2), {}, 1), ("amg", 3), ("amg", {"depth": 2}), ("amg",), ("amg", {}, {}),
                "AMG", ("multigrid", (True, 2))):
        with pytest.raises(ValueError):
            s.set_preconditioner(bad)
    with pytest.raises(ValueError, match="multigrid.*amg"):
        s.set_preconditioner("ilu")
    for good in (("multigrid", (5, 2)), ("multigrid", (5, 2, 1), {"min_rows": 4}), ["multigrid", [5, 2, 1]], "amg",
                 ("amg", {"passes": 2, "strength": 0.5, "smooth_steps": 2, "over_correction": 1.2, "min_rows": 4})):
        with pytest.raises(pkg._lib.CgAmdError) as e:
            s.set_preconditioner(good)
        assert e.value.status == pkg._lib.ERR_INVALID and "null handle" in str(e.value)
    s.handle = None         # (nothing to close)
