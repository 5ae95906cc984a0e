#!/usr/bin/env python3
"""Records tests/golden/spmv_form_parent.json, the table tests/test_spmv_form.py feeds the stand-alone build of csrc/spmv_form.cpp.

    python scripts/record_spmv_form.py --parent PARENT_ROOT [--out tests/golden/spmv_form_parent.json]

PARENT_ROOT is a built checkout of the commit BEFORE the decision had one home.  Every case runs twice, each time in a process of
its own: the parent build creates the handle under the case's tuning keys, launches one Solver.spmv and its cgamd_last_spmv_form
record is stored as the expected answer; this build does the same and supplies the decision's inputs (cgamd_solver_spmv_form, with
the call's own n, fused flag and vector alignments written over the loop's).  The script stops where this build's own launch record
differs from the parent's.  Cases no small matrix reaches are written by hand below (DERIVED), their form read off the parent's
condition, and marked "derived" in the table.  Needs a GPU; matrices come from tests/spmv_ref.py and the other tests' builders."""
import argparse
import ctypes
import importlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_NAME = "conjugate-gradient-pyopencl_amd"
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

DT = {"f32": np.float32, "f64": np.float64, "c64": np.complex64, "c128": np.complex128}
BASE = {"resident": 0, "index_codes_min_mb": 0}
ROWS = {"dev.row_codes_min_mb": 0, "dev.row_pairs": 0}                      # the row-coded form
PAIRS = {"dev.row_codes_min_mb": 0, "dev.row_pairs": 1, "dev.row_pairs_min_mb": 0}
STENCILS = {4: (-1, 0, 1), 5: (-37, -1, 0, 1, 37), 7: (-300, -20, -1, 0, 1, 20, 300)}
P7 = (-64, -8, -1, 0, 1, 8, 64)


def palette7(dtype, n=2301):
    import spmv_ref as R
    return R.toeplitz_matrix(np.random.default_rng(n), n, P7, dtype, R.palette_values(np.random.default_rng(5), 5, dtype))


def stencil(U, dtype, n=765, palette=True):
    import spmv_ref as R
    return R.toeplitz_matrix(np.random.default_rng(U), n, STENCILS[U], dtype, R.palette_values(np.random.default_rng(5), 5, dtype) if palette else None)


def rows_up_to(max_row, dtype, n=509, every=50):
    """test_gpu_spmv_forms._rows_up_to; every: for 9, which rows keep the +-2 entries (1: all of them, the slice exceeds 2048 entries)"""
    import spmv_ref as R
    offs = sorted((-64, -8, -2, -1, 0, 1, 2, 8, 64)[:max_row])
    ip, ix, da = R.toeplitz_matrix(np.random.default_rng(max_row), n, offs, dtype, R.palette_values(np.random.default_rng(6), 5, dtype))
    if max_row < 9:
        return ip, ix, da
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ip))
    keep = (np.abs(ix - rows) != 2) | (rows % every == every // 2)
    ip2 = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows[keep], minlength=n), out=ip2[1:])
    return ip2, ix[keep], da[keep]


def ragged(dtype, enc, n=1287):
    import spmv_ref as R
    rng = np.random.default_rng(300)
    L = R.ragged_lengths(rng, n, R.length_set(4 if np.dtype(dtype).itemsize > 8 else 8), 3)
    return R.banded_matrix(rng, L, R.offsets16(rng) if enc == 16 else R.offsets8(rng), dtype)


def chunked(dtype, lpr, enc):
    import spmv_ref as R
    U = 4 if np.dtype(dtype).itemsize > 8 else 8
    n = 256 + 256 // lpr + 1
    rng = np.random.default_rng(1000 + lpr)
    L = R.ragged_lengths(rng, n, R.length_set(U, lpr), steer=False)
    return R.banded_matrix(rng, L, R.offsets16(rng) if enc == 16 else R.offsets8(rng), dtype)


def chunked_tune(ip, dtype, lpr):
    import spmv_ref as R
    spans, _ = R.plan_spans(ip)
    eb = np.dtype(dtype).itemsize + 4
    return {"dev.spmv_slice_kb": 1, "dev.spmv_chunk_kb": int(-(-spans[{2: 1, 4: 2, 8: 3, 16: 4, 32: 5}[lpr]] * eb // 1024))}


def const7(dtype, n=2301):
    """constant coefficients: 27 row patterns (the palette matrices above have more than 256, and get no row codes)"""
    import test_gpu_row_codes as RC
    return RC.stencil_matrix(n, P7, (-1.25, -0.75, -1.5, 6.5, -1.125, -0.875, -1.375), dtype)


def const5(dtype, n=1021):
    import test_gpu_row_codes as RC
    return RC.stencil_matrix(n, STENCILS[5], (-1.25, -1.5, 6.5, -1.125, -1.375), dtype)


def order8(dtype, n=1021):
    import test_gpu_row_codes as RC
    vals = (-1.25, -0.75, -1.5, 6.5, -1.125, -0.875, -1.375)
    return RC.stencil_matrix(n, P7, vals, dtype, order=lambda i: range(7) if i % 2 == 0 else (0, 1, 2, 3, 4, 6, 5))


def split_small(dtype):
    import long_rows_ref as LR
    return LR.small_case(0, dtype)


def split_dense(dtype):
    import long_rows_ref as LR
    return LR.dense_body_case(dtype)


def case(label, dt, build, tune=None, nrhs=1, fused=1, x_off=0, y_off=0, long_rows=False, misalign=False, tune_from=None):
    return dict(label=label, dt=dt, build=build, tune=dict(tune or {}), nrhs=nrhs, fused=fused, x_off=x_off, y_off=y_off, long_rows=long_rows,
                misalign=misalign, tune_from=tune_from)


def cases():
    c = []
    f64, f32 = "f64", "f32"
    novc = {"dev.value_codes": 0}
    # stream
    c += [case("stream vec", f64, lambda d: ragged(d, 8), {"dev.generic_spmv": 1}, fused=0),
          case("stream vec fused", f32, lambda d: ragged(d, 8), {"dev.generic_spmv": 1}),
          case("stream scalar", f32, lambda d: ragged(d, 8), misalign=True),
          case("stream x3 fused", "c64", lambda d: ragged(d, 8), {"dev.generic_spmv": 1}, nrhs=3)]
    # row-block: three encodings, four batch lengths, both cache policies, a cycle of 1, the wide form
    for dt, encs in ((f64, (0, 8, 16)), (f32, (8,)), ("c64", (16,)), ("c128", (0,))):
        for enc in encs:
            c.append(case(f"rowblock enc{enc}", dt, lambda d, e=enc: ragged(d, e), dict(novc, **({"index_codes": 0} if enc == 0 else {})), fused=enc != 8))
    for U in (4, 5, 7):
        c.append(case(f"rowblock batch{U}", f64, lambda d, u=U: stencil(u, d, palette=False), novc))
    c += [case("rowblock rows9", f64, lambda d: rows_up_to(9, d), novc),
          case("rowblock unroll5 forced", f32, lambda d: ragged(d, 8), dict(novc, **{"dev.spmv_unroll": 5})),
          case("rowblock nt1", f64, lambda d: ragged(d, 8), dict(novc, spmv_nt=1)),
          case("rowblock nt0 cycle1", f64, lambda d: ragged(d, 8), dict(novc, spmv_nt=0, spmv_cycle=1)),
          case("rowblock no index codes key", f64, lambda d: palette7(d), {"index_codes": 0}),
          case("wide x2", f64, lambda d: ragged(d, 8), nrhs=2), case("wide x9 c128", "c128", lambda d: ragged(d, 8), nrhs=9, fused=0)]
    # value codes: vc, vcp, joint; short batches; the knobs that leave the default (the states of DESIGN.md section 1)
    c += [case("joint", f64, palette7), case("joint f32 plain", f32, palette7, fused=0), case("joint c64", "c64", palette7),
          case("vcp", f64, palette7, {"dev.joint_codes": 0}), case("vc", f64, palette7, {"dev.vc_pipe": 0}),
          case("codes8 of a palette", f64, palette7, novc),
          case("joint batch4", f64, lambda d: stencil(4, d)), case("joint batch5", f32, lambda d: stencil(5, d)),
          case("unroll 4 below the longest row", f64, palette7, {"dev.spmv_unroll": 4}),
          case("unroll 4 below the longest row, row codes", f64, const7, dict(ROWS, **{"dev.spmv_unroll": 4})),
          case("vc_pipe 0 with row codes", f64, const7, dict(ROWS, **{"dev.vc_pipe": 0})),
          case("rows4 joint", f64, lambda d: rows_up_to(4, d)), case("rows8 vcp", f64, lambda d: rows_up_to(8, d)), case("rows9 vc", f64, lambda d: rows_up_to(9, d)),
          case("rows9 dense: slice beyond the staging", f64, lambda d: rows_up_to(9, d, every=1)),
          case("joint cycle 1", f64, palette7, {"spmv_cycle": 1}), case("joint nt1", f64, palette7, {"spmv_nt": 1})]
    # row codes at three depths, row pairs at two, 7 and 8 slots, the table, unaligned vectors
    for depth in (1, 2, 4):
        c.append(case(f"rowcode depth{depth}", f64, const7, dict(ROWS, **{"dev.row_pipe": depth}), fused=depth != 2))
    c += [case("rowcode f32 default depth", f32, const7, ROWS), case("rowcode key off", f64, const7, dict(ROWS, **{"dev.row_codes": 0})),
          case("rowpair", f64, const7, PAIRS), case("rowpair plain", f64, const7, PAIRS, fused=0),
          case("rowpair f32 depth 4 -> 2", f32, const7, dict(PAIRS, **{"dev.row_pipe": 4})),
          case("rowpair depth1", f64, const7, dict(PAIRS, **{"dev.row_pipe": 1})),
          case("rowpair 8 slots", f64, order8, PAIRS),
          case("rowpair unaligned x", f64, const7, PAIRS, x_off=8),
          case("rowpair unaligned y", f64, const7, PAIRS, y_off=8),
          case("rowpair unaligned x, plain", f64, const7, PAIRS, x_off=8, fused=0),
          case("rowpair default rule f32: rows", f32, const7, dict(PAIRS, **{"dev.row_pairs": -1})),
          case("rowpair table", f64, const7, dict(PAIRS, **{"dev.spmv_plane": 1})),
          case("rowcode table", f32, const7, dict(ROWS, **{"dev.spmv_plane": 1})),
          case("rowpair nt1 batch5", f64, const5, dict(PAIRS, spmv_nt=1))]
    # chunked
    for dt, lpr, enc in ((f64, 2, 8), (f32, 4, 0), ("c64", 8, 16), ("c128", 16, 8), (f64, 32, 0)):
        c.append(case(f"chunked lpr{lpr} enc{enc}", dt, lambda d, l=lpr, e=enc: chunked(d, l, e), {"index_codes": 0} if enc == 0 else {},
                      fused=lpr != 4, tune_from=lambda ip, d, l=lpr: chunked_tune(ip, d, l)))
    # grouped SpMM
    for dt, nrhs in ((f64, 2), (f64, 3), (f32, 4), (f64, 5), ("c64", 6), (f64, 7), (f64, 9), ("c128", 5), ("c128", 9)):
        c.append(case(f"spmm x{nrhs}", dt, lambda d: ragged(d, 8), {"dev.spmm_wide_max": 0}, nrhs=nrhs, fused=nrhs != 3))
    c += [case("spmm x9 group 3", f64, lambda d: ragged(d, 8), {"dev.spmm_wide_max": 0, "dev.spmm_group": 3}, nrhs=9),
          case("spmm x9 in launches of 4", f64, lambda d: ragged(d, 8), {"dev.spmm_wide_max": 0, "dev.spmm_rb": 4}, nrhs=9)]
    # split long rows: a row-block body (on aCols and on codes), a chunked one
    import long_rows_ref as LR
    c += [case("split rowblock body", f32, split_small, {"spmv_nt": 1}, long_rows=True, tune_from=lambda ip, d: LR.small_tune(d)),
          case("split rowblock body plain", f64, split_small, {"index_codes": 0}, long_rows=True, fused=0, tune_from=lambda ip, d: LR.small_tune(d)),
          case("split chunked body", f64, split_dense, long_rows=True, tune_from=lambda ip, d: LR.dense_body_tune(ip, d))]
    return c


# ---- cases written by hand: (label, the recorded case whose inputs they start from, inputs written over, the form) ----------------------
# The parent's conditions (spmv.hip spmv_impl before this change): vcoded needs a.cap <= 8 * kBlock and n * sizeof(T) < 2^30 -- without
# it the launch is the row-block kernel on the 8-bit codes, batch length as before, grid = rowblock_grid(row_blocks, cycle); a
# row-block list of rb_count blocks makes the grid rb_count and rules the value codes out; an empty list launches nothing
def derived(recorded):
    by = {r["label"]: r for r in recorded}

    def rb_grid(row_blocks, cycle=64):
        return 8 * ((cycle + 7) // 8) * ((row_blocks + cycle - 1) // cycle)

    out = []
    j = by["joint"]
    big = 1 << 27                         # fp64 rows at the 2^30-byte gate
    blocks = (big + 255) // 256
    for label, n in (("joint at 2^27 fp64 rows: the row-block kernel", big), ("joint one pack below 2^27 rows", big - 2)):
        rb = (n + 255) // 256
        over = {"c.n": n, "plan.row_blocks": rb}
        if n * 8 < 1 << 30:
            form = dict(j["form"], grid=rb_grid((rb + 3) // 4, 16), partials=rb)
        else:
            form = dict(j["form"], family=1, value_codes=0, grid=rb_grid(rb), partials=rb)
        out.append((label, "joint", over, form))
    assert blocks == 524288
    out.append(("row-block list of 5 blocks on a joint-coded plan", "joint", {"c.rb_list": 1, "c.rb_count": 5},
                dict(j["form"], family=1, value_codes=0, grid=5)))
    out.append(("empty row-block list", "joint", {"c.rb_list": 1, "c.rb_count": 0}, None))
    ch = by["chunked lpr2 enc8"]
    out.append(("row-block list of 1 block, chunked", "chunked lpr2 enc8", {"c.rb_list": 1, "c.rb_count": 1}, dict(ch["form"], grid=1)))
    # the pair form needs 16-byte accesses to x, y and -- only where the dot is fused -- to dvec: (!fuse || aligned16(a.dvec)); else the row form
    out.append(("fused, only dvec unaligned: the row form", "rowpair", {"c.d16": 0}, dict(by["rowpair"]["form"], family=7)))
    out.append(("plain, dvec unaligned: still the pair form", "rowpair plain", {"c.d16": 0}, dict(by["rowpair plain"]["form"])))
    return out


FORM_FIELDS = ("family", "vec", "width", "index_bits", "value_codes", "nt", "fused", "wide", "grid", "partials")


def child(root, index):
    """one case on the package at `root`: prints {"form": [10 ints], "inputs": [...] or None}"""
    sys.path.insert(0, root)
    pkg = importlib.import_module(PKG_NAME)
    lib = pkg._lib.load()
    cs = cases()[index]
    dtype = DT[cs["dt"]]
    ip, ix, da = cs["build"](dtype)
    ip, ix, da = np.asarray(ip, np.int32), np.asarray(ix, np.int32), np.asarray(da).astype(dtype)
    n, nrhs = len(ip) - 1, cs["nrhs"]
    tune = dict(BASE, **cs["tune"])
    if cs["tune_from"]:
        tune.update(cs["tune_from"](ip, dtype))
    for k, v in tune.items():
        pkg._lib.check(lib.cgamd_tune(k.encode(), int(v)))
    ctx, _ = pkg.initialize_cl_environment()
    keep = []

    def off8(a):        # device copy starting 8 bytes off a 16-byte boundary
        raw = np.concatenate([np.zeros(8, np.uint8), np.ascontiguousarray(a).view(np.uint8).reshape(-1), np.zeros(64, np.uint8)])
        keep.append(pkg.DeviceBuffer(ctx, hostbuf=raw))
        return keep[-1].ptr + 8
    if cs["misalign"]:
        keep.append(pkg.DeviceBuffer(ctx, hostbuf=ip))
        s = pkg.Solver(ctx, n, len(ix), off8(da), keep[0].ptr, off8(ix), nrhs, flags=pkg._lib.MATRIX_ON_DEVICE, dtype=dtype)
    else:
        s = pkg.Solver(ctx, n, len(ix), da, ip, ix, nrhs, dtype=dtype, **({"long_rows": True} if cs["long_rows"] else {}))
    nbytes = n * nrhs * np.dtype(dtype).itemsize + 64
    xb, yb = pkg.DeviceBuffer(ctx, hostbuf=np.zeros(nbytes, np.uint8)), pkg.DeviceBuffer(ctx, hostbuf=np.zeros(nbytes, np.uint8))
    assert xb.ptr % 16 == 0 and yb.ptr % 16 == 0
    x, y = xb.ptr + cs["x_off"], yb.ptr + cs["y_off"]
    s.spmv(x, y, fused_dot=bool(cs["fused"]))
    form = (ctypes.c_int * 10)()
    assert lib.cgamd_last_spmv_form(form, 10) == 10
    ctx.synchronize()
    inputs = None
    if hasattr(lib, "cgamd_solver_spmv_form"):
        buf, out = (ctypes.c_int * 62)(), (ctypes.c_int * 10)()
        assert lib.cgamd_solver_spmv_form(s.handle, int(cs["fused"]), buf, 62, out, 10) == 10
        inputs = [int(v) for v in buf]
        # the call Solver.spmv made, not the loop's: the caller's n and vectors (fused: the dot is taken against x)
        inputs[2] = n
        inputs[11], inputs[12], inputs[13] = int(x % 16 == 0), int(y % 16 == 0), int(x % 16 == 0 or not cs["fused"])
        if not cs["fused"]:
            inputs[13] = 1          # (no dvec: a null pointer counts as aligned)
    s.close()
    print("RESULT " + json.dumps({"form": [int(v) for v in form], "inputs": inputs}))


def run_child(root, index):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, str(index)], capture_output=True, text=True, timeout=120)
    if r.returncode != 0:
        raise SystemExit(f"case {index} on {root} ended with {r.returncode}; nothing more is started\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    line = next(l for l in r.stdout.splitlines() if l.startswith("RESULT "))
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "spmv_form_parent.json"))
    ap.add_argument("--reuse", help="a table recorded earlier: its cases are kept ...")
    ap.add_argument("--redo", default="", help="... except those whose label contains one of these comma-separated words")
    ap.add_argument("--child", nargs=2)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], int(a.child[1]))
    assert a.parent, "--parent PARENT_ROOT"
    exe = os.path.join(tempfile.mkdtemp(), "spmv_form_main")
    csrc = os.path.join(ROOT, PKG_NAME, "csrc")
    subprocess.check_call(["c++", "-std=c++17", "-O1", "-I", csrc, os.path.join(ROOT, "tests", "spmv_form_main.cpp"), os.path.join(csrc, "spmv_form.cpp"), "-o", exe])
    names = subprocess.run([exe, "names"], capture_output=True, text=True, check=True).stdout.split()
    assert len(names) == 62, names
    recorded = []
    kept = {c["label"]: c for c in json.load(open(a.reuse))["cases"] if not c.get("derived")} if a.reuse else {}
    for i, cs in enumerate(cases()):
        label = f"{cs['label']} ({cs['dt']})"
        if label in kept and not any(w and w in label for w in a.redo.split(",")):
            recorded.append(kept[label])
            continue
        old, new = run_child(os.path.abspath(a.parent), i), run_child(ROOT, i)
        assert old["inputs"] is None and new["inputs"] is not None, cs["label"]
        if old["form"] != new["form"]:
            raise SystemExit(f"{cs['label']}: this build launched {new['form']}, the parent {old['form']}")
        print(f"{i:3d} {cs['label']} ({cs['dt']} x{cs['nrhs']}): {old['form']}", flush=True)
        recorded.append({"label": label, "inputs": new["inputs"], "form": dict(zip(FORM_FIELDS, old["form"]))})
    by_short = [dict(r, label=r["label"].rsplit(" (", 1)[0]) for r in recorded]
    for label, start, over, form in derived(by_short):
        base = next(r for r in by_short if r["label"] == start)
        inputs = list(base["inputs"])
        for k, v in over.items():
            inputs[names.index(k)] = v
        recorded.append({"label": label, "inputs": inputs, "form": form, "derived": True})
    with open(a.out, "w") as f:
        json.dump({"names": names, "cases": recorded}, f, indent=0)
        f.write("\n")
    print(f"{len(recorded)} cases -> {a.out}")


if __name__ == "__main__":
    main()
