#!/usr/bin/env python3
"""The deferred x update (cgamd_solver_x_lag) against the loop that updates x in every iteration, A/B in one
process on the headline system of bench.py (3-D 7-point Laplacian 250x200x200, fp64, one right-hand side, b = 5, x0 = 0).

Forms: handles created under dev.x_lag = 1, 2, 4, 8 on ONE device matrix, and 4 / 8 again with the direction buffers of the group's
last step loaded non-temporally (dev.x_lag_dnt = 1).  First every handle runs --check iterations from the same right-hand side and x
and the whole history are compared with np.array_equal across the forms (full size).  Then --reps repeats; inside every repeat the
forms alternate, each one set_rhs, 16 iterations (two graphs) and a timed window of --iters iterations between two events on the
handles' stream.  One JSON line per form: iterations/s, median and min / max over the repeats, and the gain over lag 1 set against
lag 1's own spread.  Legs: the headline, then fp32 on the same grid, then 464^3 fp64 (what one GPU holds of the largest
configuration); the driver starts one child process per leg, each under its own time limit, chained: a leg that fails or runs out of
time ends the run.  The lines are appended to --out and echoed.
usage: x_lag_ab.py [--legs 250x200x200:f64,250x200x200:f32,464x464x464:f64] [--iters 400] [--reps 7] [--check 200]"""
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
ap.add_argument("--legs", default="250x200x200:f64,250x200x200:f32,464x464x464:f64")
ap.add_argument("--iters", type=int, default=400)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--check", type=int, default=200, help="iterations of the equality check (x and history across the forms)")
ap.add_argument("--step-timeout", type=int, default=240, help="time limit of one leg, in seconds")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "x_lag", "ab.log"))
ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
args = ap.parse_args()

if not args.child:          # the driver: opens no GPU itself
    lines = [f"# scripts/x_lag_ab.py --iters {args.iters} --reps {args.reps} --check {args.check}"]
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
nx, ny, nz = (int(v) for v in grid.split("x"))
dtype = NP[dt_name]
pkg = importlib.import_module("conjugate-gradient-pyopencl_amd")
lib = pkg._lib.load()
ctx = pkg.Context(0)
dev = torch.device("cuda", 0)
stream = torch.cuda.ExternalStream(ctx.stream, device=dev)
n = nx * ny * nz
ip, ix, da = pkg.generators.laplace3d(ctx, nx, ny, nz, dtype=dtype)
nnz = int(ix.numel())
b = torch.full((n,), 5.0, dtype=pkg.generators.torch_dtype(dtype), device=dev)
torch.cuda.synchronize()

FORMS = {"lag1": (1, 0), "lag2": (2, 0), "lag4": (4, 0), "lag8": (8, 0), "lag4+dnt": (4, 1), "lag8+dnt": (8, 1)}
handles = {}
for name, (lag, dnt) in FORMS.items():
    pkg._lib.check(lib.cgamd_tune(b"dev.x_lag", lag))
    pkg._lib.check(lib.cgamd_tune(b"dev.x_lag_dnt", dnt))
    try:
        handles[name] = pkg.Solver(ctx, n, nnz, da, ip, ix, 1, flags=pkg._lib.MATRIX_ON_DEVICE, dtype=dtype)
    finally:
        pkg._lib.check(lib.cgamd_tune(b"dev.x_lag", -1))
        pkg._lib.check(lib.cgamd_tune(b"dev.x_lag_dnt", 0))
    got = lib.cgamd_solver_x_lag(handles[name].handle)
    assert got == lag, f"{name}: the handle reports lag {got}"

# the same bits, at full size
ref = None
for name, s in handles.items():
    s.set_rhs(b, None, on_device=True)
    s.iterate(args.check)
    x, h = s.x(), s.history()
    assert np.all(np.isfinite(h)), name
    if ref is None:
        ref = (x, h)
    else:
        assert np.array_equal(h, ref[1]), f"{name}: history differs from lag1"
        assert np.array_equal(x, ref[0]), f"{name}: x differs from lag1"
del ref

rates = {name: [] for name in handles}
for rep in range(args.reps):
    for name, s in handles.items():
        s.set_rhs(b, None, on_device=True)
        s.iterate(16)
        ctx.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        s.iterate(args.iters)
        e1.record(stream)
        ctx.synchronize()
        rates[name].append(args.iters / (e0.elapsed_time(e1) * 1e-3))

base = rates["lag1"]
base_med, base_spread = statistics.median(base), max(base) - min(base)
for name, s in handles.items():
    med = statistics.median(rates[name])
    print(json.dumps({"grid": grid, "dtype": dt_name, "rows": n, "form": name, "x_lag": lib.cgamd_solver_x_lag(s.handle),
                      "iters_per_window": args.iters, "reps": args.reps, "x_and_history_equal_lag1_after": args.check,
                      "it_per_s": {"median": round(med, 1), "min": round(min(rates[name]), 1), "max": round(max(rates[name]), 1)},
                      "us_per_iteration_median": round(1e6 / med, 2), "iter_moved_bytes": s.iter_moved_bytes,
                      "gain_over_lag1": round(med / base_med, 4),
                      "gain_in_lag1_spreads": round((med - base_med) / base_spread, 1) if base_spread > 0 else None}), flush=True)
    s.close()
ctx.close()
