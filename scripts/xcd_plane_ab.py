#!/usr/bin/env python3
"""The plane-matched XCD schedule of the row- and pair-coded SpMV (dev.spmv_plane, cgamd_solver_spmv_schedule)
against the block-cyclic schedule, A/B in one process.

Forms: two handles on ONE device matrix, created under dev.spmv_plane = 0 (the cycle) and 1 (the table).  First both run --check
iterations from the same right-hand side and x and the whole history are compared with np.array_equal (full size).  Then --reps
repeats; inside every repeat the forms alternate, each one set_rhs, 16 iterations (two graphs) and a timed window of --iters iterations
between two events on the handles' stream.  One JSON line per form: iterations/s, median and min / max over the repeats, and the gain
over the cycle set against the cycle's own spread.  Legs: the headline (3-D 7-point Laplacian 250x200x200, fp64), fp32 on the same
grid, 100M rows (464^3, fp64) and the 2-D 5-point system of 5M rows (2236 x 2236, fp64; its stride is 2.2 super blocks); the driver
starts one child process per leg, each under its own time limit, chained: a leg that fails or runs out of time ends the run.  The
lines are appended to --out and echoed.
usage: xcd_plane_ab.py [--legs 250x200x200:f64,250x200x200:f32,464x464x464:f64,2236x2236:f64] [--iters 400] [--reps 7] [--check 200]"""
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
ap.add_argument("--legs", default="250x200x200:f64,250x200x200:f32,464x464x464:f64,2236x2236:f64")
ap.add_argument("--iters", type=int, default=400)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--check", type=int, default=200, help="iterations of the equality check (x and history across the handles)")
ap.add_argument("--step-timeout", type=int, default=240, help="time limit of one leg, in seconds")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xcd_plane", "ab.log"))
ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
args = ap.parse_args()

if not args.child:          # the driver: opens no GPU itself
    lines = [f"# scripts/xcd_plane_ab.py --iters {args.iters} --reps {args.reps} --check {args.check}"]
    for leg in args.legs.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--legs", leg, "--iters", str(args.iters), "--reps", str(args.reps),
               "--check", str(args.check)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            lines.append(f"# leg {leg} ran into its time limit of {args.step_timeout} s; stopped here")
            break
        lines += [l for l in r.stdout.splitlines() if l.startswith("{")]
        if r.returncode != 0:
            lines.append(f"# leg {leg} failed with exit status {r.returncode}; stopped here\n" + r.stderr[-2000:])
            break
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    sys.exit(1 if lines[-1].startswith("# leg") else 0)

import torch  # noqa: E402

NP = {"f32": np.float32, "f64": np.float64}
grid, dt_name = args.legs.split(":")
dims = [int(v) for v in grid.split("x")]
dtype = NP[dt_name]
pkg = importlib.import_module("conjugate-gradient-pyopencl_amd")
lib = pkg._lib.load()
ctx = pkg.Context(0)
dev = torch.device("cuda", 0)
stream = torch.cuda.ExternalStream(ctx.stream, device=dev)
if len(dims) == 3:
    ip, ix, da = pkg.generators.laplace3d(ctx, *dims, dtype=dtype)
    n = dims[0] * dims[1] * dims[2]
else:
    assert dims[0] == dims[1], "2-D legs are N x N"
    ip, ix, da = pkg.generators.poisson2d(ctx, dims[0], dtype=dtype)
    n = dims[0] * dims[0]
nnz = int(ix.numel())
b = torch.full((n,), 5.0, dtype=pkg.generators.torch_dtype(dtype), device=dev)
torch.cuda.synchronize()

# one handle per value of the key, each created under its own setting
KEY, DEFAULT = "dev.spmv_plane", -1
handles = {}
for value in (0, 1):
    pkg._lib.check(lib.cgamd_tune(KEY.encode(), value))
    try:
        s = handles[value] = pkg.Solver(ctx, n, nnz, da, ip, ix, 1, flags=pkg._lib.MATRIX_ON_DEVICE, dtype=dtype)
    finally:
        pkg._lib.check(lib.cgamd_tune(KEY.encode(), DEFAULT))
    assert s.row_codes > 0, f"{KEY} = {value}: the handle does not run a row-coded form"
    assert s.spmv_schedule["kind"] == ("plane" if value == 1 else "cycle"), s.spmv_schedule

# the same bits, at full size
ref, family = None, {}
for value, s in handles.items():
    s.set_rhs(b, None, on_device=True)
    s.iterate(args.check)
    x, h = s.x(), s.history()
    assert np.all(np.isfinite(h)), value
    assert s.last_spmv_form()["grid"] == s.spmv_schedule["grid"], (s.last_spmv_form(), s.spmv_schedule)
    family[value] = s.last_spmv_form()["family"]
    if ref is None:
        ref = (x, h)
    else:
        assert np.array_equal(h, ref[1]), f"{KEY} = {value}: history differs from the first handle's"
        assert np.array_equal(x, ref[0]), f"{KEY} = {value}: x differs from the first handle's"
del ref

rates = {value: [] for value in handles}
for rep in range(args.reps):
    for value, s in handles.items():
        s.set_rhs(b, None, on_device=True)
        s.iterate(16)
        ctx.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        s.iterate(args.iters)
        e1.record(stream)
        ctx.synchronize()
        rates[value].append(args.iters / (e0.elapsed_time(e1) * 1e-3))

base = rates[0]
base_med, base_spread = statistics.median(base), max(base) - min(base)
for value, s in handles.items():
    med = statistics.median(rates[value])
    print(json.dumps({"grid": grid, "dtype": dt_name, "rows": n, "schedule": s.spmv_schedule, "form": family[value],
                      "iters_per_window": args.iters, "reps": args.reps, "x_and_history_equal_after": args.check,
                      "it_per_s": {"median": round(med, 1), "min": round(min(rates[value]), 1), "max": round(max(rates[value]), 1)},
                      "us_per_iteration_median": round(1e6 / med, 2), "gain_over_cycle": round(med / base_med, 4),
                      "gain_in_cycle_spreads": round((med - base_med) / base_spread, 1) if base_spread > 0 else None}), flush=True)
    s.close()
ctx.close()
