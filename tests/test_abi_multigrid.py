"""The aggregation multigrid preconditioner through the layers that need no GPU: the header, the ctypes table, the exported symbols
and the refusals a call makes before it touches a device.  Mirrors test_abi_hermitian.py."""
import ctypes
import inspect
import os
import re
import subprocess

from conftest import PKG_NAME, ROOT

ENTRIES = {
    "cgamd_solver_set_preconditioner_multigrid": ["cgamd_solver *s", "int nx", "int ny", "int nz", "int smooth_steps",
                                                  "double over_correction", "int min_rows"],
    "cgamd_solver_mg_levels": ["cgamd_solver *s"],
    "cgamd_solver_mg_level": ["cgamd_solver *s", "int level", "long long info[6]"],
    "cgamd_solver_mg_level_matrix": ["cgamd_solver *s", "int level", "int *ptr", "int *cols", "void *vals"],
    "cgamd_solver_mg_apply": ["cgamd_solver *s", "const void *r_dev", "void *z_dev"],
}


def _header():
    return open(os.path.join(ROOT, "include", "cgamd.h")).read()


def test_header_declares_the_entries():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for entry, args in ENTRIES.items():
        m = re.search(r"\bint\s+" + entry + r"\s*\(([^;{]*)\)\s*;", code)
        assert m, f"cgamd.h does not declare {entry}"
        assert [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")] == args


def test_header_states_the_contract():
    text = re.sub(r"\s+", " ", _header().replace("*", " "))
    for phrase in ("(x >> 1, y >> 1, z >> 1)", "more than 64 distinct columns", "lmax = max_i |dinv_i| sum_j |a_ij|",
                   "kappa = 30 and 8 steps", "rho_k = 1 / (2 sigma - rho_{k-1})", "x[i] += over_correction e[agg(i)]",
                   "cgamd_solver_preconditioner_source() reports 2", "m_l = SpMVs of a cycle on level l"):
        assert phrase in text, phrase


def test_ctypes_table_and_python_interface(pkg):
    src = inspect.getsource(pkg._lib)
    assert re.search(r'"cgamd_solver_set_preconditioner_multigrid":\s*\(ci,\s*\[vp,\s*ci,\s*ci,\s*ci,\s*ci,\s*ctypes\.c_double,\s*ci\]\)', src)
    assert re.search(r'"cgamd_solver_mg_levels":\s*\(ci,\s*\[vp\]\)', src)
    assert re.search(r'"cgamd_solver_mg_level":\s*\(ci,\s*\[vp,\s*ci,\s*ctypes\.POINTER\(ll\)\]\)', src)
    assert re.search(r'"cgamd_solver_mg_level_matrix":\s*\(ci,\s*\[vp,\s*ci,\s*vp,\s*vp,\s*vp\]\)', src)
    assert re.search(r'"cgamd_solver_mg_apply":\s*\(ci,\s*\[vp,\s*vp,\s*vp\]\)', src)
    assert '"multigrid"' in inspect.getsource(pkg.Solver.set_preconditioner)
    assert callable(pkg.Solver.mg_levels)


def test_makefile_builds_the_two_files():
    mk = open(os.path.join(ROOT, PKG_NAME, "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    for name in ("multigrid.hip", "multigrid_setup.cpp"):
        assert name in srcs and os.path.exists(os.path.join(ROOT, PKG_NAME, "csrc", name))
    assert "--multigrid" in open(os.path.join(ROOT, PKG_NAME, "csrc", "cli_main.cpp")).read()


def test_built_library_exports_them(pkg):
    for path in (pkg.LIB_PATH, pkg.LEGACY_LIB_PATH):
        if not os.path.exists(path):
            continue                                # not built here: test_abi_and_host asks for the build
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        for entry in ENTRIES:
            assert any(line.split()[-1] == entry and " T " in line for line in out.splitlines()), (path, entry)


def test_null_handle_needs_no_device(pkg):
    lib = pkg._lib.load()
    E = pkg._lib.ERR_INVALID
    assert lib.cgamd_solver_set_preconditioner_multigrid(None, 4, 4, 4, 0, 0.0, 0) == E
    assert b"set_preconditioner_multigrid" in lib.cgamd_last_error()
    assert lib.cgamd_solver_mg_levels(None) < 0
    info = (ctypes.c_longlong * 6)()
    assert lib.cgamd_solver_mg_level(None, 0, info) == E
    assert lib.cgamd_solver_mg_level_matrix(None, 0, None, None, None) == E
    assert lib.cgamd_solver_mg_apply(None, None, None) == E
