#!/usr/bin/env python3
"""Tridiagonal (line) preconditioner against Jacobi and plain CG: per-iteration time and time to tolerance, one JSON line per
(system, M).  Systems, all built on the device:
  helm500   helmFE_var(500) complex64 (config 3, b = rhsA(500, 12)), M = the driver's Htrid (entries with |i - j| < 10)
  lap10m    the 10M 7-point fp64 headline system (250 x 200 x 200, b = 5), M = its x-line (tridiagonal) part
  aniso     250 x 200 x 40 fp64 7-point, x-coupling 100x, b = 5, M = its x-line part
M = none / jacobi (1/diag) / tri (cgamd_solver_set_preconditioner_tridiag with device inputs) / triy, triz (the grid systems:
the y-line / z-line part, stride nx / nx ny, through cgamd_solver_set_preconditioner_tridiag_strided).  --axis y or z puts the
100x coupling of `aniso` on that axis instead of x.  us_per_iter: `--iters` iterations of the handle's own loop (resident for
plain / Jacobi where one applies, launched for the line forms), synchronised; to_tol: iterations and wall time until
||r|| < 1e-6 ||b|| (device stop where the loop has one, else the host-driven check).
usage: pcg_tridiag_ab.py [--systems helm500,lap10m,aniso] [--precs none,jacobi,tri,triy,triz] [--axis x] [--iters 200]"""
import argparse
import ctypes
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--systems", default="helm500,lap10m,aniso")
ap.add_argument("--precs", default="none,jacobi,tri")
ap.add_argument("--axis", default="x", choices=["x", "y", "z"], help="axis of the 100x coupling of `aniso`")
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--maxit", type=int, default=20000)
ap.add_argument("--no-tol", action="store_true", help="per-iteration time only (profiling runs)")
args = ap.parse_args()
pkg = importlib.import_module("conjugate-gradient-pyopencl_amd")
lib = pkg._lib.load()
ctx = pkg.Context(0)
dev = torch.device("cuda", 0)


def system(name):
    if name == "helm500":
        dt = np.complex64
        strides = {"tri": 1}
        ip, ix, da = pkg.generators.helm_fe_var(ctx, 500, 12.0, None, 0.15, dtype=dt)
        b = pkg.generators.rhsA(ctx, 500, 12.0, dtype=dt).reshape(-1)
        width = 10                      # the driver's rule (helmFE_var.py:660-673)
    else:
        dt = np.float64
        grid = (250, 200, 200) if name == "lap10m" else (250, 200, 40)
        ip, ix, da = pkg.generators.laplace3d(ctx, *grid, dtype=dt)
        strides = {"tri": 1, "triy": grid[0], "triz": grid[0] * grid[1]}
        if name == "aniso":             # coupling 100x along --axis: those off-diagonals times 100, the diagonal 2 x 99 larger
            far = strides[{"x": "tri", "y": "triy", "z": "triz"}[args.axis]]
            n = int(ip.numel()) - 1
            rows = torch.repeat_interleave(torch.arange(n, device=dev, dtype=torch.int32), (ip[1:] - ip[:-1]).long())
            off = ix - rows
            da = torch.where(off.abs() == far, da * 100.0, torch.where(off == 0, da + 198.0, da))
        b = torch.full((int(ip.numel()) - 1,), 5.0, dtype=torch.float64, device=dev)
        width = 2
    n = int(ip.numel()) - 1
    rows = torch.repeat_interleave(torch.arange(n, device=dev), (ip[1:] - ip[:-1]).long())
    off = ix.long() - rows
    keep = off.abs() < width
    assert not bool((keep & (off.abs() > 1) & (da != 0)).any()), "M is not tridiagonal"
    tri = {}
    for prec, st in strides.items():     # lower, diag, upper of the line part at distance st
        tri[prec] = [torch.zeros(n, dtype=da.dtype, device=dev) for _ in range(3)]
        for k, o in enumerate((-st, 0, st)):
            sel = off == o
            tri[prec][k][rows[sel]] = da[sel]
    return dt, ip, ix, da.contiguous(), b.contiguous(), tri, strides


def make(name, prec, dt, ip, ix, da, tri, strides):
    n, nnz = int(ip.numel()) - 1, int(ix.numel())
    s = pkg.Solver(ctx, n, nnz, da, ip, ix, 1, flags=pkg._lib.MATRIX_ON_DEVICE, dtype=dt)
    if prec == "jacobi":
        m = (1.0 / tri["tri"][1]).contiguous()
        pkg._lib.check(lib.cgamd_solver_set_preconditioner(s.handle, pkg._lib.ptr(m), 1))
        s._m = m
    elif prec == "tri":
        pkg._lib.check(lib.cgamd_solver_set_preconditioner_tridiag(s.handle, *(pkg._lib.ptr(t) for t in tri["tri"]), 1))
    elif prec in strides:
        pkg._lib.check(lib.cgamd_solver_set_preconditioner_tridiag_strided(s.handle, strides[prec],
                                                                          *(pkg._lib.ptr(t) for t in tri[prec]), 1))
    elif prec != "none":
        raise SystemExit(f"{name} has no preconditioner {prec!r}")
    return s


for name in args.systems.split(","):
    dt, ip, ix, da, b, tri, strides = system(name)
    torch.cuda.synchronize()
    bnorm = float(torch.linalg.vector_norm(b).item())
    for prec in args.precs.split(","):
        s = make(name, prec, dt, ip, ix, da, tri, strides)
        rec = {"system": name, "n": int(ip.numel()) - 1, "dtype": np.dtype(dt).name, "M": prec, "stride": strides.get(prec, 0),
               "launches": lib.cgamd_solver_loop_launches(s.handle), "iter_moved_bytes": s.iter_moved_bytes}
        s.set_rhs(b, None, on_device=True)
        s.iterate(20)
        ctx.synchronize()
        t0 = time.perf_counter()
        s.iterate(args.iters)
        ctx.synchronize()
        rec["us_per_iter"] = round((time.perf_counter() - t0) / args.iters * 1e6, 2)
        if not args.no_tol:
            tol = 1e-6 * bnorm
            ctx.synchronize()
            t0 = time.perf_counter()
            its = None
            if rec["launches"] < 2:
                s.set_rhs(b, None, on_device=True)
                run_ = ctypes.c_int(0)
                st = lib.cgamd_solver_iterate_tol(s.handle, args.maxit, tol, ctypes.byref(run_))
                if st == 0:
                    its = int(run_.value)
            if its is None:         # (the host-driven stop of Solver.pcg, with b already on the device)
                s.set_rhs = lambda b_, x0_, s_=s: pkg.Solver.set_rhs(s_, b_, x0_, on_device=True)
                its = s._run_to_tol(b, None, tol, args.maxit, 8)
            ctx.synchronize()
            rec["to_tol_iters"] = its
            rec["to_tol_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
            rec["final_rel_res"] = float(np.sqrt(abs(s.history()[-1, 0])) / bnorm)
        print(json.dumps(rec), flush=True)
        s.close()
ctx.close()
