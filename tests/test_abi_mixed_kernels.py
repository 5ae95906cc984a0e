"""The stateless entries of the mixed-precision kernels (cgamd_mixed_accumulate / _round_down / _norm2 / _norm2_grid / _round_values)
through the layers that need no GPU: header, ctypes table, exported symbols of both libraries, and the refusals, every one of which
is made with ctx == NULL -- before a device could have been touched."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

from conftest import ROOT
import mixed_kernel_ref as K

# entry: (C arguments, the table's arguments); every entry returns int / ci
ENTRIES = {
    "cgamd_mixed_accumulate": (["cgamd_ctx *ctx", "int dtype_hi", "int size", "void *x_hi", "long long ld_hi", "const void *x_lo", "long long ld_lo",
                                "const double *scale", "const int *mask", "int nRHS"], ["vp", "ci", "ci", "vp", "ll", "vp", "ll", "vp", "vp", "ci"]),
    "cgamd_mixed_round_down": (["cgamd_ctx *ctx", "int dtype_hi", "int size", "const void *r_hi", "long long ld_hi", "void *r_lo", "long long ld_lo",
                                "const double *inv_scale", "int nRHS"], ["vp", "ci", "ci", "vp", "ll", "vp", "ll", "vp", "ci"]),
    "cgamd_mixed_norm2_grid": (["int dtype_hi", "int size"], ["ci", "ci"]),
    "cgamd_mixed_norm2": (["cgamd_ctx *ctx", "int dtype_hi", "int size", "const void *v", "long long ld", "int nRHS", "double *partials",
                           "double *out"], ["vp", "ci", "ci", "vp", "ll", "ci", "vp", "vp"]),
    "cgamd_mixed_round_values": (["cgamd_ctx *ctx", "int dtype_hi", "long long count", "const void *hi", "void *lo"], ["vp", "ci", "ll", "vp", "vp"]),
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
    m = re.search(r'"' + entry + r'":\s*\((\w+),\s*\[(.*?)\]\)', inspect.getsource(pkg._lib), flags=re.S)
    assert m, f"_lib.py does not list {entry}"
    assert m.group(1) == "ci"
    assert [a.strip() for a in m.group(2).split(",")] == py_args
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
    src = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "cgamd.h")).read())
    for phrase in ("NEITHER READ NOR WRITTEN", "is written as +0", "in index order", "16-byte form", "scalar form", "gradual underflow",
                   "nearest-even"):
        assert phrase in src, phrase


def test_norm2_grid_without_a_device(pkg):
    lib, L = pkg._lib.load(), pkg._lib
    for m in (1, 2, 4095, 4096, 4097, 8193, 1024 * 4096, K.BIG, 2 ** 31 - 1):
        assert lib.cgamd_mixed_norm2_grid(L.F64, m) == K.grid(m), m
        if m % 2 == 0:
            assert lib.cgamd_mixed_norm2_grid(L.C128, m // 2) == K.grid(m), m
    assert lib.cgamd_mixed_norm2_grid(L.C128, 2 ** 31 - 1) == 1024          # 2^32 - 2 lanes: counted in 64 bits
    for dt, size in ((L.F32, 8), (L.C64, 8), (-1, 8), (4, 8), (L.F64, 0), (L.C128, -3)):
        assert lib.cgamd_mixed_norm2_grid(dt, size) == 0


def test_refusals_are_made_before_the_context_is_looked_at(pkg):
    """ctx is NULL in every call; the message names what was judged.  The order of the header: pointers, leading dimensions, dtype,
    size / nRHS, then the context"""
    lib, L = pkg._lib.load(), pkg._lib
    junk = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))

    def refused(rc, word):
        assert rc == L.ERR_INVALID
        assert word in lib.cgamd_last_error(), (word, lib.cgamd_last_error())

    acc = lambda dt=L.F64, n=4, xh=junk, lh=4, xl=junk, ll=4, sc=junk, mk=junk, nr=1: lib.cgamd_mixed_accumulate(None, dt, n, xh, lh, xl, ll, sc, mk, nr)
    rd = lambda dt=L.F64, n=4, rh=junk, lh=4, rl=junk, ll=4, sc=junk, nr=1: lib.cgamd_mixed_round_down(None, dt, n, rh, lh, rl, ll, sc, nr)
    n2 = lambda dt=L.F64, n=4, v=junk, ld=4, nr=1, p=junk, o=junk: lib.cgamd_mixed_norm2(None, dt, n, v, ld, nr, p, o)
    rv = lambda dt=L.F64, n=4, hi=junk, lo=junk: lib.cgamd_mixed_round_values(None, dt, n, hi, lo)
    for kw in ({"xh": None}, {"xl": None}, {"sc": None}, {"mk": None}):
        refused(acc(**kw), b"mixed_accumulate: null")
    for kw in ({"rh": None}, {"rl": None}, {"sc": None}):
        refused(rd(**kw), b"mixed_round_down: null")
    for kw in ({"v": None}, {"p": None}, {"o": None}):
        refused(n2(**kw), b"mixed_norm2: null")
    for kw in ({"hi": None}, {"lo": None}):
        refused(rv(**kw), b"mixed_round_values: null")
    for f, kws in ((acc, ({"lh": 3}, {"ll": 3})), (rd, ({"lh": 3}, {"ll": 3})), (n2, ({"ld": 3},))):
        for kw in kws:
            refused(f(**kw), b"leading dimension")
            refused(f(dt=L.C128, **kw), b"leading dimension")
    for f in (acc, rd, n2, rv):
        for dt in (L.F32, L.C64, -1, 4):
            refused(f(dt=dt), b"dtype_hi")
        refused(f(n=-1), b"bad size")
        for dt in (L.F64, L.C128):
            refused(f(dt=dt), b"ctx is NULL")
            refused(f(dt=dt, n=0), b"ctx is NULL")
    for f in (acc, rd, n2):
        refused(f(nr=0), b"bad size/nRHS")
