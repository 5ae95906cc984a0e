#!/usr/bin/env python3
"""Multigrid PCG on the row-partitioned solver, one hierarchy per rank on its cut matrix (DistSolver.set_preconditioner(("multigrid",
local_dims)), cgamd_dist_set_preconditioner_multigrid), against Jacobi and against no preconditioner, measured on ONE GPU.

Workload: the isotropic 7-point Laplacian of the headline system, fp64, b = 5, solved to sqrt|r.r| < 1e-6 ||b|| through
solve_until (cgamd_dist_iterate_until, check_every = 8).
  self   one process, a one-rank peer-to-peer handle that is its own halo peer on a 250 x 200 x 25 slab: 1.25M rows, one rank's share
         of the headline system.  The couplings between the first two planes are routed through halo slots the rank fills from its
         own rows, in BOTH directions, so pushes, waits and the scalar rounds all run (only the wire is missing) and the cut matrix
         stays symmetric: it is the slab with one cut face (plane 0 on its own, planes 1 ... 24 together)
  two    2 ranks as processes that share cuda:0 (gloo bootstrap, peer-to-peer mailboxes), the 250 x 200 x 40 system: 1M rows each
Per preconditioner, after one untimed solve: iterations, ms per solve (median and extremes of --reps solves, the window is the whole
solve on the host clock, x on the host side of the stream included, between barriers in the `two` leg), the launches per iteration
and the setup time of the preconditioner.  Also recorded: us per iteration of cgamd_dist_iterate WITHOUT a preconditioner on the same
handle (200 iterations after 20, best and median of 3) -- with --iterate-only, and --root pointing at another checkout's tree, the
same figure for that checkout (this script only needs what that tree has when it is run so).

What the figures cannot say: two ranks that share one GPU also share its compute units and memory -- every launch of a V-cycle on one
rank queues beside the other's -- and a mailbox in the same HBM says little about xGMI.  They price the cycle beside the exchange and
reduction launches of this loop, on this machine, and nothing else.

The driver opens no GPU: every leg is a child process (the `two` leg: one per rank) under its own time limit, chained; a leg that
fails or runs out of time ends the run.  Lines are appended to --out and echoed.
usage: dist_mg_ab.py [--legs self,two] [--reps 7] [--out profiles/dist_mg/ab.log] [--iterate-only] [--root DIR] [--tag TEXT]"""
import argparse
import importlib
import json
import os
import socket
import statistics
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--legs", default="self,two")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--maxit", type=int, default=1000)
ap.add_argument("--grid-self", default="250x200x25")
ap.add_argument("--grid-two", default="250x200x40")
ap.add_argument("--iterate-only", action="store_true", help="only the per-iteration time of cgamd_dist_iterate without a preconditioner")
ap.add_argument("--root", default=HERE, help="the tree whose package is measured")
ap.add_argument("--tag", default="this tree")
ap.add_argument("--step-timeout", type=int, default=240, help="time limit of one leg, in seconds")
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "dist_mg", "ab.log"))
ap.add_argument("--child", default="", help=argparse.SUPPRESS)       # leg:rank:world:port
args = ap.parse_args()


def children(leg):
    world = 2 if leg == "two" else 1
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    base = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--maxit", str(args.maxit), "--root", args.root, "--tag", args.tag,
            "--grid-self", args.grid_self, "--grid-two", args.grid_two] + (["--iterate-only"] if args.iterate_only else [])
    return [subprocess.Popen(base + ["--child", f"{leg}:{r}:{world}:{port}"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            for r in range(world)]


if not args.child:                      # the driver
    lines = [f"# scripts/dist_mg_ab.py --reps {args.reps}{' --iterate-only' if args.iterate_only else ''}; {args.tag}"]
    for leg in args.legs.split(","):
        procs = children(leg)
        deadline, failed = time.monotonic() + args.step_timeout, None
        outs = []
        for p in procs:
            try:
                outs.append(p.communicate(timeout=max(1.0, deadline - time.monotonic())))
            except subprocess.TimeoutExpired:
                failed = f"# leg {leg} ran into its time limit of {args.step_timeout} s; stopped here"
                break
        for p in procs:
            if p.poll() is None:
                p.kill()
        if failed is None:
            lines += [l for l in outs[0][0].splitlines() if l.startswith("{")]
            bad = [(r, p.returncode) for r, p in enumerate(procs) if p.returncode != 0]
            if bad:
                failed = f"# leg {leg} failed (rank, exit status) {bad}; stopped here\n" + outs[bad[0][0]][1][-2000:]
        if failed:
            lines.append(failed)
            break
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    sys.exit(1 if lines[-1].startswith("# leg") else 0)

# ---- one rank of one leg
leg, rank, world, port = args.child.split(":")
rank, world = int(rank), int(world)
sys.path.insert(0, args.root)
import torch  # noqa: E402

pkg = importlib.import_module("conjugate-gradient-pyopencl_amd")
dmod = importlib.import_module("conjugate-gradient-pyopencl_amd.dist")
dist = None
if world > 1:
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(rank), WORLD_SIZE=str(world), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
ctx = pkg.Context(0)
nx, ny, nz = (int(v) for v in (args.grid_two if leg == "two" else args.grid_self).split("x"))
n, h = nx * ny * nz, nx * ny
ranges = dmod.row_ranges(n, world)
rb, re = ranges[rank]
indptr, cols, data = pkg.generators.laplace3d(ctx, nx, ny, nz, dtype=np.float64, row_begin=rb, row_end=re)
if world == 1:      # the rank is its own halo peer: the links between planes 0 and 1 go through 2 h halo slots it fills from its own rows
    rows = torch.repeat_interleave(torch.arange(n, device=dev), (indptr[1:] - indptr[:-1]).long())
    c = cols.long()
    route = ((c < h) & (rows >= h)) | ((c >= h) & (c < 2 * h) & (rows < h))
    plan = dmod.HaloPlan(0, 1, 0, n, n, 2 * h, torch.where(route, c + n, c).to(torch.int32), torch.arange(2 * h), [0], [2 * h], [2 * h],
                         torch.arange(2 * h, dtype=torch.int32, device=dev))
else:
    plan = dmod.build_halo_plan(cols.cpu(), ranges, rank)
    plan.cols_local = plan.cols_local.to(dev)
    plan.send_index = plan.send_index.to(dev)
b = torch.full((re - rb,), 5.0, dtype=torch.float64, device=dev)
xbuf = torch.empty_like(b)
torch.cuda.synchronize()
tol = 1e-6 * 5.0 * np.sqrt(n)
s = dmod.DistSolver(ctx, plan, indptr, data, np.float64, comm="p2p")


def barrier():
    s.synchronize()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()


def timed(fn):
    barrier()
    t0 = time.perf_counter()
    out = fn()
    barrier()
    return (time.perf_counter() - t0) * 1e3, out


def summary(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


say = (lambda d: print(json.dumps(d), flush=True)) if rank == 0 else (lambda d: None)
common = {"leg": leg, "ranks": world, "rows_per_rank": re - rb, "tag": args.tag}
per_iter = []
for _ in range(3):
    s.set_rhs(b, None)
    s.iterate(20)
    ms, _ = timed(lambda: s.iterate(200))
    per_iter.append(ms * 1e3 / 200)
say({**common, "form": "iterate", "preconditioner": "none", "loop_launches": s.loop_launches(),
     "us_per_iteration": {"min": round(min(per_iter), 2), "median": round(statistics.median(per_iter), 2)}})
if not args.iterate_only:
    local = (nx, ny, nz) if world == 1 else dmod.local_grid_dims((nx, ny, nz), ranges, rank)
    medians = {}
    for name, pre in (("none", None), ("jacobi", "jacobi"), ("multigrid", ("multigrid", local))):
        setup_ms, _ = timed(lambda: s.set_preconditioner(pre))
        got, its = [], 0
        for rep in range(args.reps + 1):
            ms, its = timed(lambda: (s.solve_until(b, None, tol, args.maxit, check_every=8), s.x(xbuf))[0])
            if rep:
                got.append(ms)
        medians[name] = statistics.median(got)
        line = {**common, "form": "solve_until", "preconditioner": name, "tol": tol, "iterations": int(its), "ms_per_solve": summary(got),
                "reps": args.reps, "loop_launches": s.loop_launches(), "setup_ms": round(setup_ms, 3),
                "ms_per_iteration": round(medians[name] / max(1, int(its)), 4)}
        if name == "multigrid":
            line["levels"] = [L["rows"] for L in s.mg_levels()]
            line["speedup_over_none"] = round(medians["none"] / medians[name], 3)
            line["speedup_over_jacobi"] = round(medians["jacobi"] / medians[name], 3)
        say(line)
assert s.p2p_error() == 0
s.close()
ctx.close()
if dist is not None:
    dist.barrier()
    dist.destroy_process_group()
