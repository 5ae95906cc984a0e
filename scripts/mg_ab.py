#!/usr/bin/env python3
"""Multigrid PCG (Solver.set_preconditioner(("multigrid", dims)) / cgamd_solver_set_preconditioner_multigrid) against the same
handle's plain solve_until and against Jacobi, in ONE process on ONE GPU, at one commit.

Workloads: the headline system, the 7-point Laplacian on 250 x 200 x 200 (10M rows) in fp64, b[i] = 5, x0 = 0, to 1e-6 ||b|| and to
1e-10 ||b||; and config 2, the 2-D 5-point Laplacian on 1000 x 1000 (--grid 1000x1000).  Matrix, b and x stay on the device.
Forms, alternating inside every one of --reps repeats after one untimed round (medians with the extremes; the window is the whole
solve on the host clock, the stream drained on both sides): none, jacobi, multigrid -- each set_preconditioner once, then
set_rhs(b), iterate_until(tol, maxit, check_every 8), x.
Recorded: the setup time of the hierarchy (set_preconditioner, median of 3), the level table, the launches per iteration, ms per
solve and iterations per form, the TRUE residual of the x returned, and us per iteration of the multigrid loop (a window of
--window fixed-count iterations) split into the fine level and the rest.  The split: the coarse part is measured on a second handle
that holds the LEVEL-1 matrix of the hierarchy with the same options -- its multigrid iteration minus its plain iteration is one
cycle over the levels 1 ... L - 1 (smoothing on level 1 included) plus one r.z launch; the fine part is the remainder.

The driver opens no GPU: the measurement is a child process under its own time limit.  Lines are appended to --out and echoed.
usage: mg_ab.py [--grid 250x200x200] [--reps 7] [--tols 1e-6,1e-10] [--out profiles/multigrid/ab.log]"""
import argparse
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
ap.add_argument("--maxit", type=int, default=6000)
ap.add_argument("--window", type=int, default=64)
ap.add_argument("--step-timeout", type=int, default=420, help="time limit of the measurement, in seconds")
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "multigrid", "ab.log"))
ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
args = ap.parse_args()

if not args.child:                      # the driver
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--grid", args.grid, "--reps", str(args.reps), "--tols", args.tols,
           "--maxit", str(args.maxit), "--window", str(args.window)]
    lines = [f"# scripts/mg_ab.py --grid {args.grid} --reps {args.reps} --tols {args.tols}"]
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
dims = tuple(int(v) for v in args.grid.split("x"))
dims = dims + (1,) * (3 - len(dims))
n = int(np.prod(dims))
if dims[2] == 1 and dims[0] == dims[1]:
    indptr, cols, data = pkg.generators.poisson2d(ctx, dims[0], dtype=np.float64)
else:
    indptr, cols, data = pkg.generators.laplace3d(ctx, *dims, dtype=np.float64)
nnz = int(data.numel())
b = torch.full((n,), 5.0, dtype=torch.float64, device=dev)
x = torch.zeros_like(b)
y = torch.zeros_like(b)
torch.cuda.synchronize()
bnorm = 5.0 * np.sqrt(n)


def drain():
    ctx.synchronize()
    torch.cuda.synchronize()


def timed(fn):
    drain()
    t0 = time.perf_counter()
    out = fn()
    drain()
    return (time.perf_counter() - t0) * 1e3, out


def summary(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def window_us(s, rhs):
    """us per iteration of a window of fixed-count iterations, median of 5"""
    out = []
    for _ in range(6):
        s.set_rhs(rhs, None, on_device=True)
        s.iterate(8)
        out.append(timed(lambda: s.iterate(args.window))[0] * 1e3 / args.window)
    return statistics.median(out[1:])


say = lambda d: print(json.dumps(d), flush=True)      # noqa: E731
M = ("multigrid", dims)
handles = {name: pkg.Solver(ctx, n, nnz, data, indptr, cols, 1, flags=L.MATRIX_ON_DEVICE, dtype=np.float64)
           for name in ("none", "jacobi", "multigrid")}
ref = pkg.Solver(ctx, n, nnz, data, indptr, cols, 1, flags=L.MATRIX_ON_DEVICE, dtype=np.float64)      # the residual's SpMV only
handles["jacobi"].set_preconditioner("jacobi")
setup = [timed(lambda: handles["multigrid"].set_preconditioner(M))[0] for _ in range(4)][1:]
mg = handles["multigrid"]
levels = mg.mg_levels()
say({"rows": n, "grid": list(dims), "setup_ms": summary(setup), "levels": levels,
     "launches_per_iteration": {k: lib.cgamd_solver_loop_launches(s.handle) for k, s in handles.items()},
     "iter_moved_bytes": {k: lib.cgamd_solver_iter_moved_bytes(s.handle) for k, s in handles.items()}})

for rel in (float(v) for v in args.tols.split(",")):
    tol = rel * bnorm
    got, last, resid = {k: [] for k in handles}, {}, {}
    for rep in range(args.reps + 1):
        for name, s in handles.items():
            def solve(s=s):
                s.set_rhs(b, None, on_device=True)
                its = s.iterate_until(tol, args.maxit, 8)
                s.x(x)
                return int(its[0])
            ms, its = timed(solve)
            if rep:
                got[name].append(ms)
            else:
                ref.spmv(x, y)
                drain()
                last[name], resid[name] = its, float(torch.linalg.vector_norm(b - y)) / bnorm
    for name in handles:
        say({"preconditioner": name, "rel_tol": rel, "iterations": last[name], "true_residual_over_b": resid[name],
             "ms_per_solve": summary(got[name]), "reps": args.reps,
             "speedup_over_none": round(statistics.median(got["none"]) / statistics.median(got[name]), 3),
             "speedup_over_jacobi": round(statistics.median(got["jacobi"]) / statistics.median(got[name]), 3)})

# us per iteration, and the split of the multigrid iteration
us = {name: window_us(s, b) for name, s in handles.items()}
split = {}
if len(levels) > 1:
    ip1, ix1, da1 = mg.mg_level_matrix(1)
    d1 = (levels[1]["nx"], levels[1]["ny"], levels[1]["nz"])
    L.check(lib.cgamd_tune(b"resident", 0))       # the plain window on the launched loop too, like the multigrid one
    try:
        c = pkg.Solver(ctx, levels[1]["rows"], len(ix1), da1, ip1, ix1, 1, dtype=np.float64)
    finally:
        L.check(lib.cgamd_tune(b"resident", 1))
    b1 = torch.full((levels[1]["rows"],), 5.0, dtype=torch.float64, device=dev)
    plain1 = window_us(c, b1)
    c.set_preconditioner(("multigrid", d1))
    mg1 = window_us(c, b1)
    c.close()
    split = {"level1_plain_us": round(plain1, 2), "level1_multigrid_us": round(mg1, 2), "coarse_part_us": round(mg1 - plain1, 2),
             "fine_part_us": round(us["multigrid"] - (mg1 - plain1), 2)}
say({"us_per_iteration": {k: round(v, 2) for k, v in us.items()}, "window": args.window, **split})
for s in list(handles.values()) + [ref]:
    s.close()
ctx.close()
