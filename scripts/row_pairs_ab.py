#!/usr/bin/env python3
"""The row-pair form of the row-coded SpMV (dev.row_pairs, cgamd_solver_row_pairs): two rows per lane and one
16-byte gather per slot against one row per lane and 8-byte gathers, A/B in one process.

Forms: two handles on ONE device matrix, created under dev.row_pairs = 0 (the row form) and 1 (the pair form).  First both run --check
iterations from the same right-hand side and x and the whole history are compared with np.array_equal (full size).  Then --reps
repeats; inside every repeat the forms alternate, each one set_rhs, 16 iterations (two graphs) and a timed window of --iters iterations
between two events on the handles' stream.  One JSON line per form: iterations/s, median and min / max over the repeats, and the gain
over the row form set against the row form's own spread.  Legs: the headline (3-D 7-point Laplacian 250x200x200, fp64), fp32 on the
same grid, the 2-D 5-point system of 5M rows (2236 x 2236, fp64) and 100M rows (464^3, fp64); the driver starts one child process per
leg, each under its own time limit, chained: a leg that fails or runs out of time ends the run.  The lines are appended to --out and
echoed.
usage: row_pairs_ab.py [--legs 250x200x200:f64,250x200x200:f32,2236x2236:f64,464x464x464:f64] [--iters 400] [--reps 7] [--check 200]"""
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
ap.add_argument("--legs", default="250x200x200:f64,250x200x200:f32,2236x2236:f64,464x464x464:f64")
ap.add_argument("--iters", type=int, default=400)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--check", type=int, default=200, help="iterations of the equality check (x and history across the handles)")
ap.add_argument("--step-timeout", type=int, default=240, help="time limit of one leg, in seconds")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "row_pairs", "ab.log"))
ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
args = ap.parse_args()

if not args.child:          # the driver: opens no GPU itself
    lines = [f"# scripts/row_pairs_ab.py --iters {args.iters} --reps {args.reps} --check {args.check}"]
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

# (key, value, the value to put back): one handle per entry, each created under its own setting
forms = [("dev.row_pairs", v, -1) for v in (0, 1)]
handles = {}
for key, value, default in forms:
    pkg._lib.check(lib.cgamd_tune(key.encode(), value))
    try:
        s = handles[value] = pkg.Solver(ctx, n, nnz, da, ip, ix, 1, flags=pkg._lib.MATRIX_ON_DEVICE, dtype=dtype)
    finally:
        pkg._lib.check(lib.cgamd_tune(key.encode(), default))
    assert s.row_codes > 0, f"{key} = {value}: the handle does not run the row-coded form"
    assert (s.row_pairs > 0) == (value == 1), f"{key} = {value}: the handle reports {s.row_pairs} pair patterns"

# the same bits, at full size
ref = None
for value, s in handles.items():
    s.set_rhs(b, None, on_device=True)
    s.iterate(args.check)
    x, h = s.x(), s.history()
    assert np.all(np.isfinite(h)), value
    assert s.last_spmv_form()["family"] == ("rowpair" if value == 1 else "rowcode"), s.last_spmv_form()
    if ref is None:
        ref = (x, h)
    else:
        assert np.array_equal(h, ref[1]), f"{forms[0][0]} = {value}: history differs from the first handle's"
        assert np.array_equal(x, ref[0]), f"{forms[0][0]} = {value}: x differs from the first handle's"
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

first = forms[0][1]
base = rates[first]
base_med, base_spread = statistics.median(base), max(base) - min(base)
for value, s in handles.items():
    med = statistics.median(rates[value])
    print(json.dumps({"grid": grid, "dtype": dt_name, "rows": n, "form": "rowpair" if value == 1 else "rowcode", "row_pipe": s.row_pipe, "row_patterns": s.row_codes, "pair_patterns": s.row_pairs,
                      "iters_per_window": args.iters, "reps": args.reps, "x_and_history_equal_after": args.check,
                      "it_per_s": {"median": round(med, 1), "min": round(min(rates[value]), 1), "max": round(max(rates[value]), 1)},
                      "us_per_iteration_median": round(1e6 / med, 2), "gain_over_rowcode": round(med / base_med, 4),
                      "gain_in_rowcode_spreads": round((med - base_med) / base_spread, 1) if base_spread > 0 else None}), flush=True)
    s.close()
ctx.close()
