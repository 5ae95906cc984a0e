"""The development entries of the multigrid kernels (cgamd_mg_smooth_step / _restrict / _prolong / _scan) and of a hierarchy's levels
(cgamd_solver_mg_level_state / _mg_level_spmv) through the layers that need no GPU: header, ctypes table, exported symbols of both
libraries, and the refusals that are made with ctx == NULL or a NULL handle -- before a device could have been touched."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

from conftest import ROOT

D = "double"
# entry: (C arguments, the table's arguments); every entry returns int / ci
ENTRIES = {
    "cgamd_mg_smooth_step": (["cgamd_ctx *ctx", "int dtype", "int mode", "int size", "long long ld", "int nRHS", "const void *dinv", "const void *b",
                              "const void *w", "void *d", "void *x", "double c0", "double c1", "int store_d"],
                             ["vp", "ci", "ci", "ci", "ll", "ci", "vp", "vp", "vp", "vp", "vp", D, D, "ci"]),
    "cgamd_mg_restrict": (["cgamd_ctx *ctx", "int dtype", "int nx", "int ny", "int nz", "const int *members", "int n_coarse", "long long ld_f",
                           "long long ld_c", "int nRHS", "const void *b", "const void *w", "void *bc", "const void *dinv_c", "void *xc", "void *dc",
                           "double c1", "int store_d"],
                          ["vp", "ci", "ci", "ci", "ci", "vp", "ci", "ll", "ll", "ci", "vp", "vp", "vp", "vp", "vp", "vp", D, "ci"]),
    "cgamd_mg_prolong": (["cgamd_ctx *ctx", "int dtype", "int nx", "int ny", "int nz", "const int *agg", "int n_fine", "long long ld_f",
                          "long long ld_c", "int nRHS", "const void *e", "void *x", "double omega"],
                         ["vp", "ci", "ci", "ci", "ci", "vp", "ci", "ll", "ll", "ci", "vp", "vp", D]),
    "cgamd_mg_scan": (["cgamd_ctx *ctx", "int n", "int *counts_to_ptr", "int *overflow"], ["vp", "ci", "vp", "vp"]),
    "cgamd_solver_mg_level_state": (["cgamd_solver *s", "int level", "int which", "void *out_host", "long long cap_values", "long long *count"],
                                    ["vp", "ci", "ci", "vp", "ll", "ctypes.POINTER(ll)"]),
    "cgamd_solver_mg_level_spmv": (["cgamd_solver *s", "int level", "const void *x_dev", "void *w_dev"], ["vp", "ci", "vp", "vp"]),
}


def _header():
    src = open(os.path.join(ROOT, "include", "cgamd.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_header_declares_the_entry(entry):
    c_args, _ = ENTRIES[entry]
    m = re.search(r"\bint\s+" + entry + r"\s*\(([^;{]*)\)\s*;", _header())
    assert m, f"cgamd.h does not declare {entry}"
    assert [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")] == c_args


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_ctypes_table_lists_the_entry(pkg, entry):
    _, py_args = ENTRIES[entry]
    m = re.search(r'"' + entry + r'":\s*\((\w+),\s*\[(.*?)\]\),\n', inspect.getsource(pkg._lib), flags=re.S)
    assert m, f"_lib.py does not list {entry}"
    assert m.group(1) == "ci"
    assert [a.strip().replace("ctypes.c_double", D) for a in m.group(2).split(",")] == py_args
    fn = getattr(pkg._lib.load(), entry)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(py_args)


def test_built_libraries_export_the_entries(pkg):
    for path in (pkg.LIB_PATH, pkg.LEGACY_LIB_PATH):
        assert os.path.exists(path), "run __graft_entry__.build() first"
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
        assert set(ENTRIES) <= exported, (path, sorted(set(ENTRIES) - exported))


def test_header_states_the_kernel_contracts():
    """the promises the device tests check are written where a caller reads them"""
    src = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "cgamd.h")).read()).replace(" * ", " ")
    for phrase in ("ONE IEEE operation in the value type", "ROUNDED TO THE REAL TYPE", "NO LANE AT OR BEYOND `size`", "w is NOT READ",
                   "d is NOT READ in modes 0 and 1", "d is NOT WRITTEN", "the scaled d is the LEFT operand", "dinv is shared by the columns",
                   "ASCENDING", "-1 behind the last", "a list of exactly 8 has no -1", "nothing at or beyond n_fine",
                   "every prefix is clamped to 2^31 - 1", "*overflow is NOT WRITTEN", "as the doubles the launches are given",
                   "exactly as the cycle launches it", "The launch chain of one cycle"):
        assert phrase in src, phrase


def test_refusals_are_made_before_the_context_is_looked_at(pkg):
    """ctx is NULL in every call; the message names what was judged.  The order of the header: mode, pointers, size / nRHS, leading
    dimensions, dtype, then the context"""
    lib, L = pkg._lib.load(), pkg._lib
    junk = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))

    def refused(rc, word):
        assert rc == L.ERR_INVALID
        assert word in lib.cgamd_last_error(), (word, lib.cgamd_last_error())

    def sm(dt=L.F64, mode=2, n=4, ld=4, nr=1, dinv=junk, b=junk, w=junk, d=junk, x=junk, store=1):
        return lib.cgamd_mg_smooth_step(None, dt, mode, n, ld, nr, dinv, b, w, d, x, 0.5, 0.5, store)

    def rs(dt=L.F64, dims=(3, 2, 1), mem=None, nc=2, ldf=6, ldc=2, nr=1, b=junk, w=junk, bc=junk, dinv=junk, xc=junk, dc=junk, store=1):
        return lib.cgamd_mg_restrict(None, dt, dims[0], dims[1], dims[2], mem, nc, ldf, ldc, nr, b, w, bc, dinv, xc, dc, 0.5, store)

    def pr(dt=L.F64, dims=(3, 2, 1), agg=None, nf=6, ldf=6, ldc=2, nr=1, e=junk, x=junk):
        return lib.cgamd_mg_prolong(None, dt, dims[0], dims[1], dims[2], agg, nf, ldf, ldc, nr, e, x, 1.6)

    def sc(n=4, a=junk, flag=junk):
        return lib.cgamd_mg_scan(None, n, a, flag)

    for mode in (-1, 3):
        refused(sm(mode=mode), b"mode is 0, 1 or 2")
    for kw in ({"dinv": None}, {"b": None}, {"x": None}, {"w": None}, {"d": None}, {"d": None, "mode": 1}, {"d": None, "store": 0}, {"w": None, "mode": 1}):
        refused(sm(**kw), b"mg_smooth_step: null")
    refused(sm(mode=0, w=None, d=None, store=0), b"ctx is NULL")                # what mode 0 does not touch may be NULL
    refused(sm(mode=1, d=None, store=0), b"ctx is NULL")
    for kw in ({"b": None}, {"w": None}, {"bc": None}, {"dinv": None}, {"xc": None}, {"dc": None}):
        refused(rs(**kw), b"mg_restrict: null")
    refused(rs(dc=None, store=0), b"ctx is NULL")
    for kw in ({"e": None}, {"x": None}):
        refused(pr(**kw), b"mg_prolong: null")
    for kw in ({"a": None}, {"flag": None}):
        refused(sc(**kw), b"mg_scan: null")
    for f, kws in ((sm, ({"n": -1}, {"nr": 0})), (rs, ({"nc": -1}, {"nr": 0}, {"dims": (0, 2, 1)}, {"dims": (3, 2, -1)}, {"mem": junk, "dims": (0, 0, 0)})),
                   (pr, ({"nf": -1}, {"nr": 0}, {"dims": (3, 0, 1)}, {"nf": 7, "ldf": 7})), (sc, ({"n": -1},))):
        for kw in kws:
            refused(f(**kw), b"bad size")
    refused(rs(nc=3, ldc=3), b"number of boxes")
    for f, kws in ((sm, ({"ld": 3},)), (rs, ({"ldf": 5}, {"ldc": 1}, {"mem": junk, "dims": (9, 0, 0), "ldf": 8})), (pr, ({"ldf": 5}, {"ldc": 1}, {"agg": junk, "ldc": 0}))):
        for kw in kws:
            refused(f(**kw), b"leading dimension")
    for f in (sm, rs, pr):
        for dt in (-1, 4):
            refused(f(dt=dt), b"dtype")
        for dt in (L.F32, L.F64, L.C64, L.C128):
            refused(f(dt=dt), b"ctx is NULL")
    refused(rs(mem=junk, dims=(9, 0, 0), ldf=9), b"ctx is NULL")                # a stored map: ny and nz are not looked at
    refused(pr(agg=junk, dims=(0, 0, 0), ldc=1), b"ctx is NULL")
    refused(sc(), b"ctx is NULL")
    refused(sc(n=0), b"ctx is NULL")


def test_handle_entries_reject_null(pkg):
    lib, L = pkg._lib.load(), pkg._lib
    junk = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    count = ctypes.c_longlong(0)
    assert lib.cgamd_solver_mg_level_state(None, 0, 0, junk, 8, ctypes.byref(count)) == L.ERR_INVALID
    assert b"mg_level_state: null" in lib.cgamd_last_error()
    assert lib.cgamd_solver_mg_level_spmv(None, 0, junk, junk) == L.ERR_INVALID
    assert b"mg_level_spmv: null" in lib.cgamd_last_error()
