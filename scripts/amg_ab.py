#!/usr/bin/env python3
"""Algebraic multigrid PCG (Solver.set_preconditioner("amg") / cgamd_solver_set_preconditioner_amg) against the preconditioners a
caller had before it, in ONE process per system on ONE GPU, at one commit, in the style of scripts/mg_ab.py.

Systems, fp64, b[i] = 5, x0 = 0, to 1e-6 ||b|| and to 1e-10 ||b||, matrix, b and x on the device:
  headline   the 7-point Laplacian on 250 x 200 x 200 (10M rows): amg against the grid multigrid and Jacobi
  zaniso     250 x 200 x 40 with 100 x z-coupling: amg against the z-line preconditioner and the grid multigrid
  permuted   the 7-point Laplacian on 100^3 (1M rows) under a seeded random permutation: amg against Jacobi (nothing else applies)
Forms alternate inside every one of --reps repeats after one untimed round (medians with the extremes; the window is the whole solve
on the host clock, the stream drained on both sides): set_preconditioner once, then set_rhs(b), iterate_until(tol, maxit, check_every
8), x.  Recorded per system: the setup time of every form (set_preconditioner, median of 3), the level table of amg, the launches per
iteration, ms per solve and iterations per form, the TRUE residual of the x returned, us per iteration (a window of --window
fixed-count iterations).

The driver opens no GPU: every system is a child process under its own time limit, and the first that fails ends the run.  Lines are
appended to --out and echoed.
usage: amg_ab.py [--systems headline,zaniso,permuted] [--reps 7] [--tols 1e-6,1e-10] [--out profiles/amg/ab.log]"""
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
ap.add_argument("--systems", default="headline,zaniso,permuted")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--tols", default="1e-6,1e-10")
ap.add_argument("--maxit", type=int, default=6000)
ap.add_argument("--window", type=int, default=64)
ap.add_argument("--step-timeout", type=int, default=300, help="time limit of one system's measurement, in seconds")
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "amg", "ab.log"))
ap.add_argument("--child", default="", help=argparse.SUPPRESS)
args = ap.parse_args()

if not args.child:                      # the driver
    os.makedirs(os.path.dirname(args.out), exist_ok=True)

    def record(lines):                  # after every system, so that a long run shows its progress
        if not lines:
            return
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
        print("\n".join(lines), flush=True)

    record([f"# scripts/amg_ab.py --systems {args.systems} --reps {args.reps} --tols {args.tols}"])
    for system in args.systems.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", system, "--reps", str(args.reps), "--tols", args.tols,
               "--maxit", str(args.maxit), "--window", str(args.window)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            record([f"# the measurement of {system} ran into its time limit of {args.step_timeout} s; stopped here"])
            sys.exit(1)
        record([l for l in p.stdout.splitlines() if l.startswith("{")])
        if p.returncode != 0:
            record([f"# the measurement of {system} failed (exit status {p.returncode}); stopped here\n" + p.stderr[-2000:]])
            sys.exit(1)
    sys.exit(0)

# ---- the measurement of one system
sys.path.insert(0, HERE)
import torch  # noqa: E402

pkg = importlib.import_module("conjugate-gradient-pyopencl_amd")
L = pkg._lib
lib = L.load()
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
ctx = pkg.Context(0)

if args.child == "headline":
    dims = (250, 200, 200)
    indptr, cols, data = pkg.generators.laplace3d(ctx, *dims, dtype=np.float64)
    forms = {"amg": "amg", "multigrid": ("multigrid", dims), "jacobi": "jacobi"}
elif args.child == "zaniso":
    dims = (250, 200, 40)
    indptr, cols, data = pkg.generators.laplace3d(ctx, *dims, dtype=np.float64)
    rows = torch.repeat_interleave(torch.arange(indptr.numel() - 1, device=dev), (indptr[1:] - indptr[:-1]).long())
    dist = (cols.long() - rows).abs()
    data[dist == dims[0] * dims[1]] *= 100.0          # the z-couplings, and the diagonal that goes with them: 2 + 2 + 200
    data[dist == 0] = 204.0
    del rows, dist
    forms = {"amg": "amg", "line_z": ("line", dims[0] * dims[1]), "multigrid": ("multigrid", dims)}
elif args.child == "permuted":
    import scipy.sparse as sp
    dims = (100, 100, 100)
    indptr, cols, data = pkg.generators.laplace3d(ctx, *dims, dtype=np.float64)
    A = sp.csr_matrix((data.cpu().numpy(), cols.cpu().numpy(), indptr.cpu().numpy()), shape=(10 ** 6,) * 2)
    perm = np.random.default_rng(5).permutation(A.shape[0])
    A = sp.csr_matrix(A[perm][:, perm])
    A.sort_indices()
    indptr, cols, data = (torch.from_numpy(a).to(dev) for a in (A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data))
    forms = {"amg": "amg", "jacobi": "jacobi"}
else:
    raise SystemExit(f"unknown system {args.child}")
n = int(indptr.numel()) - 1
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
handles = {name: pkg.Solver(ctx, n, nnz, data, indptr, cols, 1, flags=L.MATRIX_ON_DEVICE, dtype=np.float64) for name in forms}
ref = pkg.Solver(ctx, n, nnz, data, indptr, cols, 1, flags=L.MATRIX_ON_DEVICE, dtype=np.float64)      # the residual's SpMV only
setup = {name: summary([timed(lambda: handles[name].set_preconditioner(m))[0] for _ in range(4)][1:]) for name, m in forms.items()}
levels = handles["amg"].mg_levels()
say({"system": args.child, "rows": n, "nnz": nnz, "setup_ms": setup,
     "amg_levels": [{"rows": v["rows"], "nnz": v["nnz"], "lmax": round(v["lmax"], 4)} for v in levels],
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
        say({"system": args.child, "preconditioner": name, "rel_tol": rel, "iterations": last[name], "true_residual_over_b": resid[name],
             "ms_per_solve": summary(got[name]), "reps": args.reps,
             "amg_speedup_over_this": round(statistics.median(got[name]) / statistics.median(got["amg"]), 3)})

say({"system": args.child, "us_per_iteration": {name: round(window_us(s, b), 2) for name, s in handles.items()}, "window": args.window})
for s in list(handles.values()) + [ref]:
    s.close()
ctx.close()
