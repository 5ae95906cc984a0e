#!/usr/bin/env python3
"""Setup time of the line preconditioner: built from the handle's matrix on the device (cgamd_solver_set_preconditioner_line)
against the route through the caller's arrays (three device arrays into cgamd_solver_set_preconditioner_tridiag_strided with
on_device = 1: download, serial host factorisation and plan, upload).  One JSON line per case, written to --out (default
profiles/line_setup/) as <group>.log and echoed.

Without --case this is the driver: every case runs in a child process of its own under a time limit (--limit seconds), one after
the other, and the driver stops at the first child that fails or runs out of time.
  grids    aniso (250 x 200 x 40 fp64, z-coupling 100x, stride 50 000) and lap10m (250 x 200 x 200) at strides 1, 250 and 50 000.
           extract_ms: cutting the three arrays out of the CSR matrix with torch on the device (what the array route needs first,
           stated apart); arrays_ms / line_ms: the two setup calls, synchronised, median of 5 after one warm-up with the spread;
           iter_ms_*: one iterate_timed pair per route (same kernel, same plan); aniso also setup + solve to 1e-6 ||b||.
  chains   1-D chains at stride 2 (two segments of n / 2 rows), n = 2^16 .. 2^23, fp64: the device factorisation (one thread per
           segment, dev.line_host_route = -1) against the host route of the same call (dev.line_host_route = 1).  The default
           host-route limit (kLineHostRouteRows, solver.cpp) is the largest segment length at which the device is no slower.
usage: line_setup_ab.py [--groups grids,chains] [--out DIR] [--limit 240] [--reps 5]"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRID_CASES = [("aniso", 50_000), ("lap10m", 1), ("lap10m", 250), ("lap10m", 50_000)]
CHAIN_CASES = [1 << k for k in range(16, 24)]

ap = argparse.ArgumentParser()
ap.add_argument("--groups", default="grids,chains")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "line_setup"))
ap.add_argument("--limit", type=int, default=240, help="seconds a case may take")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--case", default=None, help="(child) grid:<system>:<stride> or chain:<rows>")
args = ap.parse_args()


def driver():
    os.makedirs(args.out, exist_ok=True)
    for group in args.groups.split(","):
        cases = [f"grid:{s}:{st}" for s, st in GRID_CASES] if group == "grids" else [f"chain:{n}" for n in CHAIN_CASES]
        log = os.path.join(args.out, "long_segments.log" if group == "chains" else "grids.log")
        with open(log, "w") as f:
            for case in cases:
                try:
                    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--reps", str(args.reps)],
                                       stdout=subprocess.PIPE, text=True, timeout=args.limit)
                except subprocess.TimeoutExpired:
                    raise SystemExit(f"{case}: no result within {args.limit} s; stopping")
                if p.returncode != 0:
                    raise SystemExit(f"{case}: exit status {p.returncode}; stopping")
                f.write(p.stdout)
                f.flush()
                print(p.stdout, end="", flush=True)


def timed(fn, sync, reps):
    """median and spread in ms of `reps` synchronised calls after one warm-up"""
    ts = []
    for k in range(reps + 1):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts = ts[1:]
    return {"ms": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}


def child():
    import torch
    pkg = importlib.import_module("conjugate-gradient-pyopencl_amd")
    lib = pkg._lib.load()
    ctx = pkg.Context(0)
    dev = torch.device("cuda", 0)
    kind, *rest = args.case.split(":")
    dt = np.float64
    if kind == "grid":
        name, stride = rest[0], int(rest[1])
        grid = (250, 200, 200) if name == "lap10m" else (250, 200, 40)
        ip, ix, da = pkg.generators.laplace3d(ctx, *grid, dtype=dt)
        n = int(ip.numel()) - 1
        if name == "aniso":          # z-coupling 100x: those off-diagonals times 100, the diagonal 2 x 99 larger
            rows = torch.repeat_interleave(torch.arange(n, device=dev, dtype=torch.int32), (ip[1:] - ip[:-1]).long())
            off = ix - rows
            da = torch.where(off.abs() == grid[0] * grid[1], da * 100.0, torch.where(off == 0, da + 198.0, da)).contiguous()
    else:
        import scipy.sparse as sp
        name, stride, n = "chain", 2, int(rest[0])
        rng = np.random.default_rng(1)
        offd = -rng.uniform(0.2, 1.0, n - 2)
        A = sp.diags([offd, 2.5 + rng.uniform(0.0, 1.0, n), offd], [-2, 0, 2], format="csr")
        ip, ix, da = (torch.from_numpy(a).to(dev) for a in (A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data))
    nnz = int(ix.numel())
    b = torch.full((n,), 5.0, dtype=torch.float64, device=dev)
    sync = torch.cuda.synchronize
    sync()

    def extract():
        rows = torch.repeat_interleave(torch.arange(n, device=dev), (ip[1:] - ip[:-1]).long())
        off = ix.long() - rows
        out = [torch.zeros(n, dtype=da.dtype, device=dev) for _ in range(3)]
        for k, o in enumerate((-stride, 0, stride)):
            sel = off == o
            out[k][rows[sel]] = da[sel]
        return out

    def handle(route=0):
        pkg._lib.check(lib.cgamd_tune(b"dev.line_host_route", route))     # a handle keeps the configuration it was created under
        try:
            return pkg.Solver(ctx, n, nnz, da, ip, ix, 1, flags=pkg._lib.MATRIX_ON_DEVICE, dtype=dt)
        finally:
            pkg._lib.check(lib.cgamd_tune(b"dev.line_host_route", 0))

    def line(s):
        pkg._lib.check(lib.cgamd_solver_set_preconditioner_line(s.handle, stride))

    rec = {"system": name, "n": n, "dtype": "float64", "stride": stride}
    if kind == "chain":
        rec["segment_rows"] = n // 2
        for label, route in (("device", -1), ("host_route", 1)):
            s = handle(route)
            t = timed(lambda: line(s), sync, args.reps)
            rec[label + "_ms"], rec[label + "_spread"], rec[label + "_source"] = t["ms"], [t["min"], t["max"]], s.preconditioner_source
            s.close()
        rec["device_no_slower"] = rec["device_ms"] <= rec["host_route_ms"]
        print(json.dumps(rec), flush=True)
        ctx.close()
        return
    t = timed(extract, sync, args.reps)
    rec["extract_ms"], rec["extract_spread"] = t["ms"], [t["min"], t["max"]]
    tri = extract()
    sync()
    s1, s2 = handle(), handle()

    def arrays(s):
        pkg._lib.check(lib.cgamd_solver_set_preconditioner_tridiag_strided(s.handle, stride, *(pkg._lib.ptr(v) for v in tri), 1))

    for label, s, fn in (("arrays", s1, arrays), ("line", s2, line)):
        t = timed(lambda: fn(s), sync, args.reps)
        rec[label + "_ms"], rec[label + "_spread"], rec[label + "_source"] = t["ms"], [t["min"], t["max"]], s.preconditioner_source
        rec[label + "_launches"] = lib.cgamd_solver_loop_launches(s.handle)
        s.set_rhs(b, None, on_device=True)
        s.iterate(20)
        rec["iter_ms_" + label] = [round(v, 4) for v in s.iterate_timed(50)]      # (SpMV, whole iteration)
    rec["device_faster"] = rec["line_ms"] < rec["arrays_ms"]
    if name == "aniso":              # setup + solve to 1e-6 ||b||, both routes, on a handle that has no preconditioner yet
        tol = 1e-6 * float(torch.linalg.vector_norm(b).item())
        for label, fn in (("arrays", arrays), ("line", line)):
            s = handle()
            s.set_rhs = lambda b_, x0_, s_=s: pkg.Solver.set_rhs(s_, b_, x0_, on_device=True)
            sync()
            t0 = time.perf_counter()
            fn(s)
            t1 = time.perf_counter()
            its = s._run_to_tol(b, None, tol, 20000, 8)
            sync()
            t2 = time.perf_counter()
            rec["setup_solve_" + label] = {"setup_ms": round((t1 - t0) * 1e3, 3), "solve_ms": round((t2 - t1) * 1e3, 3), "iters": its,
                                           "total_ms": round((t2 - t0) * 1e3, 3)}
            s.close()
    s1.close()
    s2.close()
    print(json.dumps(rec), flush=True)
    ctx.close()


if args.case is None:
    driver()
else:
    child()
