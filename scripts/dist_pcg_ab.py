#!/usr/bin/env python3
"""What preconditioned CG costs on one rank of a row-partitioned run, measured on ONE GPU, next to the single-GPU handle.

Setup: one process, a one-rank peer-to-peer handle that is its own halo peer (the self-peer slab of scripts/dist_slab_probe.py:
the plane below is routed through halo slots the rank fills from its own first plane, so pushes, waits and the scalar rounds all
run -- only the wire is missing), on the 1/8 slab (250 x 200 x 5) of the anisotropic 250 x 200 x 40 system with 100x z-coupling.
Preconditioners: none, Jacobi, lines at stride 1 and nx * ny.  Per preconditioner: us per iteration and iterations to
sqrt|r.r| < 1e-6 ||b||, for the dist handle and for the plain Solver on the same slab with the same preconditioner, in the same run.
(The routed links are halo columns to the dist handle: its z-lines are cut there, the Solver's are not.)

Every GPU step is a child process of its own under its own time limit; the steps are chained: the first that fails ends the run.
usage: python scripts/dist_pcg_ab.py --commit HASH [--out profiles/dist_pcg/slab_ab.log] [--grid 250x200x5] [--iters 200]
"""
import argparse
import importlib
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = ("none", "jacobi", "line1", "linez")


def step(args):
    import torch
    pkg = importlib.import_module("conjugate-gradient-pyopencl_amd")
    dmod = importlib.import_module("conjugate-gradient-pyopencl_amd.dist")
    L = pkg._lib
    lib = L.load()
    nx, ny, nz = (int(v) for v in args.grid.split("x"))
    n, h = nx * ny * nz, nx * ny
    pre = {"none": None, "jacobi": "jacobi", "line1": ("line", 1), "linez": ("line", h)}[args.step]
    ctx = pkg.Context(0)
    dev = torch.device("cuda", 0)
    indptr, indices, data = pkg.generators.laplace3d(ctx, nx, ny, nz, dtype=np.float64)
    rows = torch.repeat_interleave(torch.arange(n, device=dev), (indptr[1:] - indptr[:-1]).long())
    off = indices.long() - rows
    data = torch.where(off == 0, torch.full_like(data, 204.0), torch.where(off.abs() == h, torch.full_like(data, -100.0), -torch.ones_like(data)))
    b = torch.full((n,), 5.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    bnorm = 5.0 * np.sqrt(n)

    def run(obj, single):
        sync = ctx.synchronize if single else obj.synchronize
        best = []
        for _ in range(3):
            obj.set_rhs(b, None, on_device=True) if single else obj.set_rhs(b, None)
            obj.iterate(20)
            sync()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            obj.iterate(args.iters)
            sync()
            torch.cuda.synchronize()
            best.append((time.perf_counter() - t0) / args.iters * 1e6)
        obj.set_rhs(b, None, on_device=True) if single else obj.set_rhs(b, None)
        obj.iterate(args.maxit)
        hist = obj.history()
        hist = np.abs(hist[:, 0] if hist.ndim == 2 else hist)
        at = np.flatnonzero(np.sqrt(hist) < 1e-6 * bnorm)
        return min(best), float(np.median(best)), (str(int(at[0])) if at.size else f">{args.maxit}")

    s = pkg.Solver(ctx, n, int(indices.numel()), data, indptr, indices, 1, flags=L.MATRIX_ON_DEVICE | L.NO_GRAPH, dtype=np.float64)
    s.set_preconditioner(pre)
    lo, med, k = run(s, True)
    print(f"{args.grid} rows={n} {args.step:7s} plain Solver (launched loop, {lib.cgamd_solver_loop_launches(s.handle)} launches): "
          f"{lo:7.2f} us/iter (median {med:7.2f}), {k} iterations to 1e-6 ||b||", flush=True)
    s.close()
    route = (indices < h) & (rows >= h)
    cols_local = torch.where(route, indices + n, indices).to(torch.int32)
    plan = dmod.HaloPlan(0, 1, 0, n, n, h, cols_local, torch.arange(h), [0], [h], [h], torch.arange(h, dtype=torch.int32, device=dev))
    d = dmod.DistSolver(ctx, plan, indptr, data, np.float64, comm="p2p")
    d.set_preconditioner(pre)
    lo, med, k = run(d, False)
    assert d.p2p_error() == 0
    print(f"{args.grid} rows={n} {args.step:7s} dist p2p self-peer ({d.loop_launches()} launches):                 "
          f"{lo:7.2f} us/iter (median {med:7.2f}), {k} iterations to 1e-6 ||b||", flush=True)
    d.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="250x200x5")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--maxit", type=int, default=400)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dist_pcg", "slab_ab.log"))
    ap.add_argument("--step", default="", choices=("",) + STEPS)
    ap.add_argument("--step-timeout", type=int, default=120)
    args = ap.parse_args()
    if args.step:
        return step(args)
    lines = [f"# scripts/dist_pcg_ab.py --grid {args.grid} --iters {args.iters}; commit {args.commit}"]
    for name in STEPS:          # chained: a step that fails or runs out of time ends the run
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--grid", args.grid, "--iters", str(args.iters),
                                "--maxit", str(args.maxit)], capture_output=True, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            lines.append(f"# step {name} ran into its time limit of {args.step_timeout} s; stopped here")
            break
        lines += [l for l in r.stdout.splitlines() if l.startswith(args.grid)]
        if r.returncode != 0:
            lines.append(f"# step {name} failed with exit status {r.returncode}; stopped here\n" + r.stderr[-2000:])
            break
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 1 if lines[-1].startswith("# step") else 0


if __name__ == "__main__":
    sys.exit(main())
