#!/usr/bin/env python3
"""CGAMD_SPLIT_LONG_ROWS against the unflagged handle (DESIGN.md sections 4 and 7): SpMV time and CG iterations/s on matrices with hub rows.

Matrices (fp64, built in numpy):
  lap        the 100^3 7-point Laplacian + 0.1 I (no hub: what the body can reach at best)
  hub1       the same with one hub row coupled to every 8th row (weight -1/64, diagonals raised: symmetric positive definite)
  hub16      the same with 16 hubs
  pa         the Laplacian + 0.1 I of a preferential-attachment graph of 1M vertices (vertex i attaches to 3 earlier vertices
             floor(i u^2), u uniform: degrees fall off as a power law, the first vertices are hubs)
Configurations: the unflagged handle, and the flagged handle at segment lengths 1024, 2048, 4096 and 8192 entries.  ONE PROCESS PER
CONFIGURATION, each under its own time limit, chained: a configuration that fails or runs out of time ends the run.
Reported per configuration, medians of --reps windows: SpMV us (event pairs around the SpMV launches of cgamd_solver_iterate_timed:
for the split form the pair brackets the chain of its three launches), CG iterations/s over --iters captured iterations, the form that
ran and cgamd_solver_long_rows.  The three launches' separate shares are not measured here.
usage: long_rows_ab.py [--matrices lap,hub1,hub16,pa] [--segments 1024,2048,4096,8192] [--iters 200] [--reps 7]"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--matrices", default="lap,hub1,hub16,pa")
ap.add_argument("--segments", default="1024,2048,4096,8192")
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--step-timeout", type=int, default=150, help="time limit of one configuration, in seconds")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "long_rows", "ab.log"))
ap.add_argument("--child", default="", help=argparse.SUPPRESS)
args = ap.parse_args()

if not args.child:          # the driver: opens no GPU itself
    lines = [f"# scripts/long_rows_ab.py --matrices {args.matrices} --segments {args.segments} --iters {args.iters} --reps {args.reps}"]
    failed = False
    for m in args.matrices.split(","):
        cfgs = ["off"] + ([] if m == "lap" else [f"seg{s}" for s in args.segments.split(",")])
        for cfg in cfgs:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", f"{m}:{cfg}", "--iters", str(args.iters), "--reps", str(args.reps)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
            except subprocess.TimeoutExpired:
                lines.append(f"# {m}:{cfg} ran into its time limit of {args.step_timeout} s; stopped here")
                failed = True
                break
            lines += [l for l in r.stdout.splitlines() if l.startswith("{")]
            if r.returncode != 0:
                lines.append(f"# {m}:{cfg} failed with exit status {r.returncode}; stopped here\n" + r.stderr[-2000:])
                failed = True
                break
        if failed:
            break
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    sys.exit(1 if failed else 0)


def csr_from_coo(n, rows, cols, vals):
    """duplicates summed, columns sorted"""
    key = rows.astype(np.int64) * n + cols
    uk, inv = np.unique(key, return_inverse=True)
    v = np.zeros(uk.size)
    np.add.at(v, inv, vals)
    r = (uk // n).astype(np.int64)
    ip = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(r, minlength=n), out=ip[1:])
    return ip, (uk % n).astype(np.int32), v


def laplacian3d(nx, hubs):
    n = nx ** 3
    idx = np.arange(n, dtype=np.int64)
    i, j, k = idx % nx, (idx // nx) % nx, idx // (nx * nx)
    rows, cols, vals = [idx], [idx], [np.full(n, 6.1)]
    for ok, off in ((i > 0, -1), (i < nx - 1, 1), (j > 0, -nx), (j < nx - 1, nx), (k > 0, -nx * nx), (k < nx - 1, nx * nx)):
        rows.append(idx[ok]); cols.append(idx[ok] + off); vals.append(np.full(int(ok.sum()), -1.0))
    w = 1.0 / 64
    hub_rows = [(2 * h + 1) * n // (2 * hubs) + 3 for h in range(hubs)]          # (not multiples of 8: a hub is not coupled to itself)
    for h in hub_rows:
        t = np.arange(0, n, 8, dtype=np.int64)
        hh = np.full(t.size, h, dtype=np.int64)
        rows += [hh, t, t, hh]; cols += [t, hh, t, hh]; vals += [np.full(t.size, -w), np.full(t.size, -w), np.full(t.size, w), np.full(t.size, w)]
    return csr_from_coo(n, np.concatenate(rows), np.concatenate(cols), np.concatenate(vals))


def pa_laplacian(n, m=3):
    rng = np.random.default_rng(11)
    src = np.repeat(np.arange(1, n, dtype=np.int64), m)
    dst = np.floor(src * rng.random(src.size) ** 2).astype(np.int64)
    keep = src != dst
    src, dst = src[keep], dst[keep]
    pair = np.unique(np.minimum(src, dst) * n + np.maximum(src, dst))
    a, b = pair // n, pair % n
    deg = np.bincount(np.concatenate([a, b]), minlength=n).astype(np.float64)
    idx = np.arange(n, dtype=np.int64)
    return csr_from_coo(n, np.concatenate([a, b, idx]), np.concatenate([b, a, idx]), np.concatenate([-np.ones(a.size), -np.ones(a.size), deg + 0.1]))


import torch  # noqa: E402

name, cfg = args.child.split(":")
dtype = np.float64
if name == "pa":
    ip, ix, da = pa_laplacian(1 << 20)
else:
    ip, ix, da = laplacian3d(100, {"lap": 0, "hub1": 1, "hub16": 16}[name])
n = len(ip) - 1
pkg = importlib.import_module("conjugate-gradient-pyopencl_amd")
lib = pkg._lib.load()
ctx = pkg.Context(0)
dev = torch.device("cuda", 0)
stream = torch.cuda.ExternalStream(ctx.stream, device=dev)
flagged = cfg != "off"
if flagged:
    pkg._lib.check(lib.cgamd_tune(b"dev.long_row_segment", int(cfg[3:])))
s = pkg.Solver(ctx, n, len(ix), da, ip, ix, 1, dtype=dtype, long_rows=flagged)
q = s.long_rows
b = np.random.default_rng(5).standard_normal(n)
spmv_us, rates = [], []
for rep in range(args.reps):
    s.set_rhs(b)
    s.iterate(16)
    ctx.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    s.iterate(args.iters)
    e1.record(stream)
    ctx.synchronize()
    rates.append(args.iters / (e0.elapsed_time(e1) * 1e-3))
    s.set_rhs(b)
    spmv_ms, _ = s.iterate_timed(20)
    spmv_us.append(spmv_ms * 1e3)
form = s.last_spmv_form()
h = s.history()
assert np.all(np.isfinite(h))
moved = lib.cgamd_solver_spmv_moved_bytes(s.handle)
med = statistics.median(spmv_us)
print(json.dumps({"matrix": name, "rows": n, "nnz": int(ip[-1]), "longest_row": int(np.diff(ip).max()), "config": cfg, "family": form["family"],
                  "body_width": form["width"], "long_rows": q, "reps": args.reps, "iters_per_window": args.iters,
                  "spmv_us": {"median": round(med, 1), "min": round(min(spmv_us), 1), "max": round(max(spmv_us), 1)},
                  "spmv_moved_GBps": round(moved / med * 1e-3, 1),
                  "cg_it_per_s": {"median": round(statistics.median(rates), 1), "min": round(min(rates), 1), "max": round(max(rates), 1)}}), flush=True)
s.close()
ctx.close()
