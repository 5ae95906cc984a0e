#!/usr/bin/env python3
"""The tolerance stop on the device of the row-partitioned solver (DistSolver.solve_until / cgamd_dist_iterate_until) against the
host scheme it replaces, measured on ONE GPU.

Workload: line-z PCG (("line", nx * ny), cut at the rank boundaries) on the anisotropic 7-point system with 100x z-coupling, fp64,
b = 5, to sqrt|r.r| < 1e-6 ||b||.
  self   one process, a one-rank peer-to-peer handle that is its own halo peer (the self-peer slab of scripts/dist_pcg_ab.py: pushes,
         waits and the scalar rounds all run, only the wire is missing) on a 250 x 200 x 25 slab: 1.25M rows, one rank's share of
         the headline system
  two    2 ranks as processes that share cuda:0 (gloo bootstrap, peer-to-peer mailboxes), the 250 x 200 x 40 system: 1M rows each
Forms, alternating inside every one of --reps repeats after one untimed round (medians with the extremes; the window is the whole
solve on the host clock, x on the host side of the stream included, between barriers in the `two` leg):
  until  solve_until(b, tol, maxit, check_every=8), x
  host   set_rhs; then iterate(8), synchronize, history() per chunk until the norm is below the tolerance; a re-run set_rhs;
         iterate(k) to the exact iteration when the chunk overshot it; x
Also recorded: us per iteration of cgamd_dist_iterate on the same handle (200 iterations after 20, best and median of 3) -- with
--iterate-only, and --root pointing at another checkout's tree, the same figure for that checkout, to be read against the ~10 %
spread between machines.

The driver opens no GPU: every leg is a child process (the `two` leg: one per rank) under its own time limit, chained; a leg that
fails or runs out of time ends the run.  Lines are appended to --out and echoed.
usage: dist_until_ab.py [--legs self,two] [--reps 7] [--out profiles/dist_until/ab.log] [--iterate-only] [--root DIR] [--tag TEXT]"""
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
ap.add_argument("--maxit", type=int, default=400)
ap.add_argument("--grid-self", default="250x200x25")
ap.add_argument("--grid-two", default="250x200x40")
ap.add_argument("--iterate-only", action="store_true", help="only the per-iteration time of cgamd_dist_iterate")
ap.add_argument("--root", default=HERE, help="the tree whose package is measured")
ap.add_argument("--tag", default="this tree")
ap.add_argument("--step-timeout", type=int, default=240, help="time limit of one leg, in seconds")
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "dist_until", "ab.log"))
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
    lines = [f"# scripts/dist_until_ab.py --reps {args.reps}{' --iterate-only' if args.iterate_only else ''}; {args.tag}"]
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
rb, re = dmod.row_ranges(n, world)[rank]
indptr, cols, data = pkg.generators.laplace3d(ctx, nx, ny, nz, dtype=np.float64, row_begin=rb, row_end=re)
rows = rb + torch.repeat_interleave(torch.arange(re - rb, device=dev), (indptr[1:] - indptr[:-1]).long())
off = cols.long() - rows
data = torch.where(off == 0, torch.full_like(data, 204.0), torch.where(off.abs() == h, torch.full_like(data, -100.0), -torch.ones_like(data)))
if world == 1:      # the rank is its own halo peer: the plane below is routed through halo slots it fills from its own first plane
    route = (cols < h) & (rows >= h)
    plan = dmod.HaloPlan(0, 1, 0, n, n, h, torch.where(route, cols + n, cols).to(torch.int32), torch.arange(h), [0], [h], [h],
                         torch.arange(h, dtype=torch.int32, device=dev))
else:
    plan = dmod.build_halo_plan(cols.cpu(), dmod.row_ranges(n, world), rank)
    plan.cols_local = plan.cols_local.to(dev)
    plan.send_index = plan.send_index.to(dev)
b = torch.full((re - rb,), 5.0, dtype=torch.float64, device=dev)
xbuf = torch.empty_like(b)
torch.cuda.synchronize()
tol = 1e-6 * 5.0 * np.sqrt(n)
s = dmod.DistSolver(ctx, plan, indptr, data, np.float64, comm="p2p")
s.set_preconditioner(("line", h))


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


def until():
    its = s.solve_until(b, None, tol, args.maxit, check_every=8)
    return its, s.x(xbuf)


def host():
    s.set_rhs(b, None)
    k, syncs = None, 0
    while s.iterations < args.maxit and k is None:
        s.iterate(min(8, args.maxit - s.iterations))
        s.synchronize()
        syncs += 1
        hist = s.history()
        below = np.flatnonzero(~(np.sqrt(np.abs(hist[-8:])) >= tol))
        if below.size:
            k = max(1, len(hist) - len(hist[-8:]) + int(below[0]))
    if k is not None and k != s.iterations:         # the chunk overshot: the x of the stopping iteration needs a second solve
        s.set_rhs(b, None)
        s.iterate(k)
    return (k if k is not None else s.iterations), s.x(xbuf)


def summary(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


per_iter = []
for _ in range(3):
    s.set_rhs(b, None)
    s.iterate(20)
    ms, _ = timed(lambda: s.iterate(200))
    per_iter.append(ms * 1e3 / 200)
say = (lambda d: print(json.dumps(d), flush=True)) if rank == 0 else (lambda d: None)
common = {"leg": leg, "ranks": world, "rows_per_rank": re - rb, "tag": args.tag}
say({**common, "form": "iterate", "loop_launches": s.loop_launches(), "us_per_iteration": {"min": round(min(per_iter), 2), "median": round(statistics.median(per_iter), 2)}})
if not args.iterate_only:
    got = {"until": [], "host": []}
    last = {}
    for rep in range(args.reps + 1):
        for name, fn in (("until", until), ("host", host)):
            ms, out = timed(fn)
            last[name] = (out[0], out[1].cpu().numpy().copy())
            if rep:
                got[name].append(ms)
    same_x = bool(np.array_equal(last["until"][1].view(np.uint8), last["host"][1].view(np.uint8)))
    for name in ("until", "host"):
        say({**common, "form": name, "tol": tol, "iterations": int(last[name][0]), "ms_per_solve": summary(got[name]), "reps": args.reps})
    say({**common, "same_iterations": last["until"][0] == last["host"][0], "same_x_bits": same_x,
         "until_over_host_speedup": round(statistics.median(got["host"]) / statistics.median(got["until"]), 3)})
assert s.p2p_error() == 0
s.close()
ctx.close()
if dist is not None:
    dist.barrier()
    dist.destroy_process_group()
