#!/usr/bin/env python3
"""Preconditioned block CG (cgamd_solver_set_block_pcg) against the SAME handle's per-column PCG.

Per case, solves to 1e-8 |b_j| in float64 for every column of ONE handle with its preconditioner in force, independent random
right-hand sides made on the device:
  (a) block     set_block_pcg(True); set_rhs; iterate_until -- all columns stop together
  (b) columns   set_block_pcg(False); set_rhs; iterate_until -- the scalar PCG loop: every column on its own recurrence and stop
Cases: the 5-point Poisson matrix on 1000^2 rows with 4 and 16 right-hand sides, with the grid multigrid and with Jacobi, and the
7-point Laplacian on 250 x 200 x 200 (the 10M-row system of bench.py) with 8 and the grid multigrid.
Method (scripts/block_ab.py's): both forms are warmed up by one solve each, then alternate inside every one of --reps repeats; a solve
is timed on the host clock from before set_rhs (b already on the device) to a synchronise behind iterate_until.  Logged per case and
form: the iterations, the median ms per solve with the extremes (the spread), and us per iteration.  Then the two vector kernels of
block_pcg.hip alone beside the three of block_cg.hip, through the development entries on device arrays of the case's shape,
--kernel-reps launches between two synchronises: us and TB/s on the bytes each must move (Gram 2, x / w update 6, q / p update 4,
weighted Gram 1 and m, q / p update with Z 5, with m 4 and m: passes of s n values).
The driver opens no GPU: one child process per case under --step-timeout, chained; a case that fails or runs out of time ends the run.
Lines are appended to --out (profiles/block_pcg/ab.log) and echoed.
usage: block_pcg_ab.py [--reps 7] [--cases 2d4mg,2d16mg,2d4jac,2d16jac,3d8mg]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"2d4mg": ("poisson2d 1000^2", 4, "multigrid"), "2d16mg": ("poisson2d 1000^2", 16, "multigrid"),
         "2d4jac": ("poisson2d 1000^2", 4, "jacobi"), "2d16jac": ("poisson2d 1000^2", 16, "jacobi"),
         "3d8mg": ("laplace3d 250x200x200", 8, "multigrid")}
TOL = 1e-8

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--cases", default="2d4mg,2d16mg,2d4jac,2d16jac,3d8mg")
ap.add_argument("--maxit", type=int, default=20000)
ap.add_argument("--kernel-reps", type=int, default=20)
ap.add_argument("--step-timeout", type=int, default=240, help="time limit of one case, in seconds")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "block_pcg", "ab.log"))
ap.add_argument("--child", default="", help=argparse.SUPPRESS)
args = ap.parse_args()

if not args.child:          # the driver
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(f"# scripts/block_pcg_ab.py --reps {args.reps} --cases {args.cases}\n")
    for case in args.cases.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", case, "--reps", str(args.reps), "--maxit", str(args.maxit),
               "--kernel-reps", str(args.kernel_reps), "--out", args.out]
        try:
            rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(f"block_pcg_ab: case {case} ended with status {rc}; nothing more is started", file=sys.stderr)
            sys.exit(rc)
    sys.exit(0)

import importlib  # noqa: E402

import torch  # noqa: E402

pkg = importlib.import_module("conjugate-gradient-pyopencl_amd")
L = pkg._lib
lib = L.load()
case = args.child
what, s, kind = CASES[case]
dtype = np.dtype(np.float64)
ctx = pkg.Context(0)
dev = torch.device("cuda", ctx.device)
if case.startswith("2d"):
    indptr, indices, data = pkg.generators.poisson2d(ctx, 1000, dtype=dtype)
    dims = (1000, 1000, 1)
else:
    indptr, indices, data = pkg.generators.laplace3d(ctx, 250, 200, 200, dtype=dtype)
    dims = (250, 200, 200)
n, nnz = int(indptr.numel()) - 1, int(indices.numel())
tdt = pkg.generators.torch_dtype(dtype)
gen = torch.Generator(device=dev)
gen.manual_seed(11)
b = torch.randn((s, n), dtype=tdt, device=dev, generator=gen)
tol_abs = (TOL * torch.linalg.vector_norm(b.double(), dim=1)).cpu().numpy()
torch.cuda.synchronize()
sv = pkg.Solver(ctx, n, nnz, data, indptr, indices, s, flags=L.MATRIX_ON_DEVICE, dtype=dtype)
sv.set_preconditioner("jacobi" if kind == "jacobi" else ("multigrid", dims))


def solve(block):
    sv.set_block_pcg(block)
    ctx.synchronize()
    t0 = time.perf_counter()
    sv.set_rhs(b, None, on_device=True)
    its = sv.iterate_until(tol_abs, args.maxit, 8)
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3, its


def true_residual():
    """max_j |b_j - A x_j| / (tol |b_j|), float64 on the device through the handle's own SpMV of the solution"""
    x = torch.empty((s, n), dtype=tdt, device=dev)
    y = torch.empty_like(x)
    sv.x(out=x)
    sv.spmv(x, y)
    ctx.synchronize()
    r = torch.linalg.vector_norm(b.double() - y.double(), dim=1).cpu().numpy()
    return float(np.max(r / tol_abs))


out = []
times = {True: [], False: []}
its, res, launches = {}, {}, {}
for block in (True, False):             # warm-up: graphs captured, the iteration counts and the true residual of each form
    _, its[block] = solve(block)
    res[block] = true_residual()
    launches[block] = lib.cgamd_solver_loop_launches(sv.handle)
status = None
for _ in range(args.reps):
    for block in (True, False):
        ms, got = solve(block)
        assert np.array_equal(got, its[block]), "a repeat took other iteration counts"
        times[block].append(ms)
        if block:
            status = sv.block_status()
for block in (True, False):
    med = statistics.median(times[block])
    out.append({"case": what, "M": kind, "nrhs": s, "tol": TOL, "form": "block pcg" if block else "columns pcg",
                "iterations": [int(its[block].min()), int(its[block].max())], "ms_per_solve": round(med, 3),
                "ms_min_max": [round(min(times[block]), 3), round(max(times[block]), 3)],
                "us_per_iteration": round(1e3 * med / max(int(its[block].max()), 1), 2), "loop_launches": launches[block],
                "residual_over_tol": round(res[block], 3),
                **({"status": status["status"], "min_pivot_ratio": round(status["min_pivot_ratio"], 4)} if block else {})})
out.append({"case": what, "M": kind, "nrhs": s, "block_over_columns_time": round(out[0]["ms_per_solve"] / out[1]["ms_per_solve"], 3),
            "iterations_ratio": round(out[0]["iterations"][1] / out[1]["iterations"][1], 3)})
sv.close()

# the vector kernels alone: the two of block_pcg.hip beside the three of block_cg.hip
code, V = L.DTYPE_CODE[dtype], dtype.itemsize
P, AP, X, Q = (torch.randn((s, n), dtype=tdt, device=dev, generator=gen) for _ in range(4))
m = torch.rand(n, dtype=tdt, device=dev, generator=gen) + 0.5
eye = torch.eye(s, dtype=tdt, device=dev).contiguous()
small = (0.01 * torch.randn((s, s), dtype=tdt, device=dev, generator=gen)).contiguous()
tri = small.triu().contiguous()
grid = lib.cgamd_block_gram_grid(n)
part = torch.empty(s * (s + 1) // 2 * grid, dtype=torch.float64, device=dev)
torch.cuda.synchronize()
p = L.ptr
kernels = {
    "gram": (2 * s, lambda: lib.cgamd_block_gram(ctx.handle, code, n, n, s, p(P), p(AP), p(part))),
    "update_xw": (6 * s, lambda: lib.cgamd_block_update_xw(ctx.handle, code, n, n, s, p(P), p(AP), p(X), p(Q), p(small), p(small), p(part))),
    "update_qp": (4 * s, lambda: lib.cgamd_block_update_qp(ctx.handle, code, n, n, s, p(Q), p(P), p(eye), p(tri), 0)),
    "gram_weighted": (s + 1, lambda: lib.cgamd_block_gram_weighted(ctx.handle, code, n, n, s, p(Q), p(m), p(part))),
    "update_qp_z (Z)": (5 * s, lambda: lib.cgamd_block_update_qp_z(ctx.handle, code, n, n, s, p(Q), p(P), p(AP), None, p(eye), p(tri), 0)),
    "update_qp_z (m)": (4 * s + 1, lambda: lib.cgamd_block_update_qp_z(ctx.handle, code, n, n, s, p(Q), p(P), None, p(m), p(eye), p(tri), 0)),
}
for name, (vectors, call) in kernels.items():
    L.check(call())
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.kernel_reps):
        L.check(call())
    ctx.synchronize()
    us = (time.perf_counter() - t0) * 1e6 / args.kernel_reps
    out.append({"case": what, "nrhs": s, "kernel": name, "us": round(us, 1), "TB_per_s": round(vectors * n * V / us / 1e6, 3)})
with open(args.out, "a") as f:
    for line in out:
        text = json.dumps(line)
        f.write(text + "\n")
        print(text)
