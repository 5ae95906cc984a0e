#!/usr/bin/env python3
"""Mixed-precision CG (MixedSolver / cgamd_mixed_solve: fp32 loop, fp64 x and residual replacement) against the fp64 handle's
solve_until -- the path an fp64 answer takes without it -- in ONE process on ONE GPU.

Workload: the headline system, the 7-point Laplacian on 250 x 200 x 200 (10M rows) in fp64, b[i] = 5, x0 = 0, to 1e-6 ||b|| and to
1e-10 ||b||, without a preconditioner and with Jacobi (on the fp64 handle; on the inner handle of the mixed solve).  Matrix, b and x
stay on the device (cgamd_mixed_solve with on_device = 1; set_rhs / iterate_until / get_x on device arrays), so that no solve pays
for a PCIe copy of 80 MB vectors.
Forms, alternating inside every one of --reps repeats after one untimed round (medians with the extremes; the window is the whole
solve on the host clock, the stream drained on both sides):
  fp64   Solver(fp64): set_rhs(b), iterate_until(tol, maxit, check_every 8), x
  mixed  MixedSolver: solve(b, x0 = 0, tol, maxit, delta) for every --deltas value
Recorded per form: ms per solve, iterations, replacements, and the TRUE residual sqrt|r.r| / ||b|| of the x returned, r = b - A x
evaluated by the fp64 handle's SpMV.

The driver opens no GPU: the measurement is a child process under its own time limit.  Lines are appended to --out and echoed.
usage: mixed_ab.py [--grid 250x200x200] [--reps 7] [--tols 1e-6,1e-10] [--deltas 0.1,0.25,0.01] [--out profiles/mixed/ab.log]"""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--grid", default="250x200x200")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--tols", default="1e-6,1e-10")
ap.add_argument("--deltas", default="0.1,0.25,0.01")
ap.add_argument("--maxit", type=int, default=6000)
ap.add_argument("--step-timeout", type=int, default=420, help="time limit of the measurement, in seconds")
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "mixed", "ab.log"))
ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
args = ap.parse_args()

if not args.child:                      # the driver
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--grid", args.grid, "--reps", str(args.reps), "--tols", args.tols,
           "--deltas", args.deltas, "--maxit", str(args.maxit)]
    lines = [f"# scripts/mixed_ab.py --grid {args.grid} --reps {args.reps} --tols {args.tols} --deltas {args.deltas}"]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
        lines += [l for l in p.stdout.splitlines() if l.startswith("{")]
        if p.returncode != 0:
            lines.append(f"# the measurement failed (exit status {p.returncode}); stopped here\n" + p.stderr[-2000:])
    except subprocess.TimeoutExpired:
        lines.append(f"# the measurement ran into its time limit of {args.step_timeout} s; stopped here")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    sys.exit(1 if lines[-1].startswith("# the measurement") else 0)

# ---- the measurement
sys.path.insert(0, HERE)
import torch  # noqa: E402

pkg = importlib.import_module("conjugate-gradient-pyopencl_amd")
L = pkg._lib
lib = L.load()
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
ctx = pkg.Context(0)
nx, ny, nz = (int(v) for v in args.grid.split("x"))
n = nx * ny * nz
indptr, cols, data = pkg.generators.laplace3d(ctx, nx, ny, nz, dtype=np.float64)
nnz = int(data.numel())
b = torch.full((n,), 5.0, dtype=torch.float64, device=dev)
x = torch.zeros_like(b)
y = torch.zeros_like(b)
torch.cuda.synchronize()
bnorm = 5.0 * np.sqrt(n)
pd, pi = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)


def drain():
    ctx.synchronize()
    torch.cuda.synchronize()


def timed(fn):
    drain()
    t0 = time.perf_counter()
    out = fn()
    drain()
    return (time.perf_counter() - t0) * 1e3, out


def true_residual(s64):
    """sqrt|r.r| / ||b|| of the x in `x`, by the fp64 handle's SpMV"""
    s64.spmv(x, y)
    drain()
    return float(torch.linalg.vector_norm(b - y)) / bnorm


def summary(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


say = lambda d: print(json.dumps(d), flush=True)      # noqa: E731
deltas = [float(v) for v in args.deltas.split(",")]
for pre in (None, "jacobi"):
    s64 = pkg.Solver(ctx, n, nnz, data, indptr, cols, 1, flags=L.MATRIX_ON_DEVICE, dtype=np.float64)
    ref = pkg.Solver(ctx, n, nnz, data, indptr, cols, 1, flags=L.MATRIX_ON_DEVICE, dtype=np.float64)      # the residual's SpMV only
    mx = pkg.MixedSolver(ctx, n, nnz, data, indptr, cols, 1, flags=L.MATRIX_ON_DEVICE, dtype=np.float64)
    if pre:
        s64.set_preconditioner(pre)
        mx.inner.set_preconditioner(pre)
    say({"rows": n, "preconditioner": pre or "none", "fp64_loop_launches": lib.cgamd_solver_loop_launches(s64.handle),
         "inner_loop_launches": lib.cgamd_solver_loop_launches(mx.inner.handle), "inner_row_codes": mx.inner.row_codes,
         "fp64_row_codes": s64.row_codes})
    for rel in (float(v) for v in args.tols.split(",")):
        tol = rel * bnorm

        def fp64():
            s64.set_rhs(b, None, on_device=True)
            its = s64.iterate_until(tol, args.maxit, 8)
            s64.x(x)
            return {"iterations": int(its[0]), "replacements": 0}

        def mixed(delta):
            x.zero_()
            torch.cuda.synchronize()
            its, st, res, repl = np.zeros(1, np.intc), np.zeros(1, np.intc), np.zeros(1), ctypes.c_int(0)
            t = np.array([tol])
            L.check(lib.cgamd_mixed_solve(mx.handle, L.ptr(b), L.ptr(x), 1, t.ctypes.data_as(pd), 1, args.maxit, delta, 0, 8, its.ctypes.data_as(pi),
                                          res.ctypes.data_as(pd), st.ctypes.data_as(pi), ctypes.byref(repl)))
            return {"iterations": int(its[0]), "replacements": int(repl.value), "status": int(st[0]), "resnorm_over_b": float(res[0]) / bnorm}

        forms = [("fp64", fp64)] + [(f"mixed delta={d:g}", (lambda d=d: mixed(d))) for d in deltas]
        got, last, resid = {k: [] for k, _ in forms}, {}, {}
        for rep in range(args.reps + 1):
            for name, fn in forms:
                ms, out = timed(fn)
                if rep:
                    got[name].append(ms)
                else:
                    last[name], resid[name] = out, true_residual(ref)
        for name, _ in forms:
            say({"preconditioner": pre or "none", "rel_tol": rel, "form": name, **last[name], "true_residual_over_b": resid[name],
                 "ms_per_solve": summary(got[name]), "reps": args.reps,
                 "speedup_over_fp64": round(statistics.median(got["fp64"]) / statistics.median(got[name]), 3)})
    mx.close()
    s64.close()
    ref.close()
ctx.close()
