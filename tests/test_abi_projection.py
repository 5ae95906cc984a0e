"""The solution-projection entries through the layers that need no GPU: the header, the ctypes table, the Makefile, the exported
symbols and the refusals a call makes before it touches a device.  Mirrors test_abi_amg.py."""
import inspect
import os
import re
import subprocess

from conftest import PKG_NAME, ROOT

ENTRIES = {
    "cgamd_solver_projection_enable": ["cgamd_solver *s", "int capacity", "double drop_tol"],
    "cgamd_solver_projection_count": ["cgamd_solver *s"],
    "cgamd_solver_projection_clear": ["cgamd_solver *s"],
    "cgamd_solver_set_rhs_projected": ["cgamd_solver *s", "const void *b", "int on_device"],
    "cgamd_solver_projection_update": ["cgamd_solver *s", "int *added"],
    "cgamd_solver_projection_state": ["cgamd_solver *s", "int which", "int slot", "void *out_host"],
    "cgamd_projection_dots": ["cgamd_ctx *ctx", "int dtype", "int size", "long long ld", "int slots", "unsigned live_mask", "const void *W",
                              "long long slot_pitch", "const void *v", "int nRHS", "void *out"],
    "cgamd_projection_combine": ["cgamd_ctx *ctx", "int dtype", "int size", "long long ld", "int slots", "unsigned live_mask", "const void *W",
                                 "long long slot_pitch", "const void *v", "const void *c", "int sign", "void *y", "int nRHS"],
    "cgamd_projection_dots_grid": ["int dtype", "int size"],
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
    for phrase in ("<w_i, A w_j> = delta_ij", "<a, b> = sum a_i b_i", "alpha_j = <w_j, b>", "x0 = sum_j alpha_j w_j, slots ascending",
                   "e = x - x0", "q = A e", "c_j = <w_j, q>", "e' = e - sum_j c_j w_j", "one classical Gram-Schmidt pass",
                   "q' = A e', nu = <e', q'>", "not <e, q> - sum c_j^2, which cancels", "s = sum alpha_j^2 + 2 sum alpha_j c_j + <e, q>",
                   "|nu| > drop_tol^2 |s|", "for the real types also nu > 0", "w_new = e' (1 / sqrt nu)", "the principal square root",
                   "a refused column stores a column of zeros", "If every column is refused, nothing is retired and nothing is stored",
                   "the oldest slot is retired before the update", "its c_j is not formed", "e = (x - x0) + alpha_ret w_ret",
                   "Padding rows (cgamd_solver_ld) of every stored vector are 0", "two calls return the same bits",
                   "packs g 256 + t + k G 256", "v[l] += v[l + off], off = 32 ... 1", "the 16 wave sums in order",
                   "(m + ceil(m / 8) + 1) n V nRHS", "two SpMVs, then", "capacity 1 ... 32", "capacity 0 disables the feature",
                   "cgamd_solver_refresh_values and cgamd_solver_reload_matrix clear the basis",
                   "changing or removing a preconditioner does not", "cgamd_solver_layout() == 0", "the conjugated form is a later change",
                   "while the stream is being captured", "the entry of a masked slot is untouched"):
        assert phrase in text, phrase


def test_ctypes_table_and_python_interface(pkg):
    src = inspect.getsource(pkg._lib)
    assert re.search(r'"cgamd_solver_projection_enable":\s*\(ci,\s*\[vp,\s*ci,\s*ctypes\.c_double\]\)', src)
    assert re.search(r'"cgamd_solver_projection_count":\s*\(ci,\s*\[vp\]\)', src)
    assert re.search(r'"cgamd_solver_projection_clear":\s*\(ci,\s*\[vp\]\)', src)
    assert re.search(r'"cgamd_solver_set_rhs_projected":\s*\(ci,\s*\[vp,\s*vp,\s*ci\]\)', src)
    assert re.search(r'"cgamd_solver_projection_update":\s*\(ci,\s*\[vp,\s*ctypes\.POINTER\(ci\)\]\)', src)
    assert re.search(r'"cgamd_solver_projection_state":\s*\(ci,\s*\[vp,\s*ci,\s*ci,\s*vp\]\)', src)
    assert re.search(r'"cgamd_projection_dots":\s*\(ci,\s*\[vp,\s*ci,\s*ci,\s*ll,\s*ci,\s*ctypes\.c_uint,\s*vp,\s*ll,\s*vp,\s*ci,\s*vp\]\)', src)
    assert re.search(r'"cgamd_projection_combine":\s*\(ci,\s*\[vp,\s*ci,\s*ci,\s*ll,\s*ci,\s*ctypes\.c_uint,\s*vp,\s*ll,\s*vp,\s*vp,\s*ci,\s*vp,\s*ci\]\)', src)
    assert re.search(r'"cgamd_projection_dots_grid":\s*\(ci,\s*\[ci,\s*ci\]\)', src)
    for name in ("enable_projection", "projection_count", "projection_clear", "set_rhs_projected", "projection_update", "projection_state"):
        assert callable(getattr(pkg.Solver, name)), name
    assert inspect.signature(pkg.Solver.enable_projection).parameters["drop_tol"].default == 0.0
    assert inspect.signature(pkg.Solver.set_rhs_projected).parameters["on_device"].default is False
    assert inspect.signature(pkg.Solver.projection_state).parameters["slot"].default == 0
    for fn in (pkg.Solver.solve_until, pkg.Solver.pcg, pkg.solve_subdomains):
        assert inspect.signature(fn).parameters["project"].default is False


def test_makefile_builds_the_file():
    mk = open(os.path.join(ROOT, PKG_NAME, "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    assert "projection.hip" in srcs and os.path.exists(os.path.join(ROOT, PKG_NAME, "csrc", "projection.hip"))


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
    assert lib.cgamd_solver_projection_enable(None, 4, 0.0) == E
    assert b"projection_enable" in lib.cgamd_last_error()
    assert lib.cgamd_solver_projection_count(None) == -E
    assert lib.cgamd_solver_projection_clear(None) == E
    assert b"projection_clear" in lib.cgamd_last_error()
    assert lib.cgamd_solver_set_rhs_projected(None, None, 0) == E
    assert b"set_rhs_projected" in lib.cgamd_last_error()
    assert lib.cgamd_solver_projection_update(None, None) == E
    assert b"projection_update" in lib.cgamd_last_error()
    assert lib.cgamd_solver_projection_state(None, 0, 0, None) == E
    assert b"projection_state" in lib.cgamd_last_error()
    assert lib.cgamd_projection_dots(None, 1, 4, 4, 1, 1, None, 4, None, 1, None) == E
    assert b"projection_dots" in lib.cgamd_last_error()
    assert lib.cgamd_projection_combine(None, 1, 4, 4, 1, 1, None, 4, None, None, 1, None, 1) == E
    assert b"projection_combine" in lib.cgamd_last_error()
    assert lib.cgamd_projection_dots_grid(7, 4) == -E
    # the grid rule, restated in tests/projection_ref.py
    import numpy as np
    import projection_ref as PR
    for code, dt in enumerate((np.float32, np.float64, np.complex64, np.complex128)):
        for n in (0, 1, 37, 957, 2 * 1024 + 37, 65536, 65537, 524289, 10_000_000):
            assert lib.cgamd_projection_dots_grid(code, n) == PR.dots_grid(dt, n), (dt, n)
