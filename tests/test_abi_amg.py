"""The algebraic multigrid entry through the layers that need no GPU: the header, the ctypes table, the exported symbols, the
command-line option and the refusals a call makes before it touches a device.  Mirrors test_abi_multigrid.py."""
import inspect
import os
import re
import subprocess

from conftest import PKG_NAME, ROOT

ENTRIES = {
    "cgamd_solver_set_preconditioner_amg": ["cgamd_solver *s", "int passes", "double strength", "int smooth_steps",
                                            "double over_correction", "int min_rows"],
    "cgamd_solver_mg_aggregates": ["cgamd_solver *s", "int level", "int *agg_host", "int *n_coarse"],
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
    for phrase in ("s_ij = -Re(b_ij)", "s_ij >= theta smax_i", "a NaN is never strong", "at most 32",
                   "pick[i] == j and pick[j] == i", "0x9E3779B1", "0x85EBCA6B", "0xC2B2AE35", "h ^= h >> 13",
                   "the larger s_ij, then the larger h(i, j), then the smaller j", "the ranks of the roots in ascending order",
                   "more than 64 distinct columns is dropped together with the passes after it", "5 rows(l + 1) > 4 rows(l)",
                   "passes 0 ... 3 (0 = 3)", "(0 = 0.25)", "aggregates included", "nx = rows, ny = nz = 0",
                   "CGAMD_ERR_INVALID on the coarsest level"):
        assert phrase in text, phrase


def test_ctypes_table_and_python_interface(pkg):
    src = inspect.getsource(pkg._lib)
    assert re.search(r'"cgamd_solver_set_preconditioner_amg":\s*\(ci,\s*\[vp,\s*ci,\s*ctypes\.c_double,\s*ci,\s*ctypes\.c_double,\s*ci\]\)', src)
    assert re.search(r'"cgamd_solver_mg_aggregates":\s*\(ci,\s*\[vp,\s*ci,\s*vp,\s*ctypes\.POINTER\(ci\)\]\)', src)
    assert '"amg"' in inspect.getsource(pkg.Solver.set_preconditioner)
    assert callable(pkg.Solver.mg_aggregates)


def test_makefile_builds_the_file_and_the_cli_knows_the_option():
    mk = open(os.path.join(ROOT, PKG_NAME, "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    assert "amg.hip" in srcs and os.path.exists(os.path.join(ROOT, PKG_NAME, "csrc", "amg.hip"))
    cli = open(os.path.join(ROOT, PKG_NAME, "csrc", "cli_main.cpp")).read()
    assert '"--amg"' in cli and "cgamd_solver_set_preconditioner_amg" in cli


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
    assert lib.cgamd_solver_set_preconditioner_amg(None, 0, 0.0, 0, 0.0, 0) == E
    assert b"set_preconditioner_amg" in lib.cgamd_last_error()
    assert lib.cgamd_solver_mg_aggregates(None, 0, None, None) == E
    assert b"mg_aggregates" in lib.cgamd_last_error()
