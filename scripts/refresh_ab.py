#!/usr/bin/env python3
"""cgamd_solver_refresh_values ("Values that change in place") against destroy + create, in one process.

One borrowed fp64 handle on the headline system (3-D 7-point Laplacian 250x200x200) whose value tensor is rewritten in place.  Three
ways to bring a handle up to date with new values are timed on the host clock, from the call to the point where the handle's stream
has drained, as medians of --reps calls:
  fast      the stencil rescaled (I + tau L with a new tau per call): the classes of equal values are intact, one pass over the values
            and the dictionaries rewritten in place (last_refresh == 1);
  rebuild   the same with ONE entry perturbed (and restored for the next call): the value, joint and row codes are built again (2);
  recreate  the handle destroyed and created again on the rescaled values.
After each way the handle runs set_rhs, 16 iterations and a window of --iters iterations between two events on its stream; the three
rates must agree (the same kernels on the same bytes), and the histories of the window after `fast` and after `recreate` on the same
values are compared with np.array_equal.  The driver starts one child process under its own time limit; the JSON lines are appended
to --out and echoed.
usage: refresh_ab.py [--grid 250x200x200] [--iters 400] [--reps 7]"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--grid", default="250x200x200")
ap.add_argument("--iters", type=int, default=400)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--step-timeout", type=int, default=300, help="time limit of the measuring process, in seconds")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refresh", "ab.log"))
ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
args = ap.parse_args()

if not args.child:          # the driver: opens no GPU itself
    lines = [f"# scripts/refresh_ab.py --grid {args.grid} --iters {args.iters} --reps {args.reps}"]
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--grid", args.grid, "--iters", str(args.iters), "--reps", str(args.reps)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
        lines += [l for l in r.stdout.splitlines() if l.startswith("{")]
        if r.returncode != 0:
            lines.append(f"# failed with exit status {r.returncode}\n" + r.stderr[-2000:])
    except subprocess.TimeoutExpired:
        lines.append(f"# ran into its time limit of {args.step_timeout} s")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    sys.exit(1 if lines[-1].startswith("#") else 0)

import torch  # noqa: E402

dims = [int(v) for v in args.grid.split("x")]
dtype = np.float64
pkg = importlib.import_module("conjugate-gradient-pyopencl_amd")
ctx = pkg.Context(0)
dev = torch.device("cuda", 0)
stream = torch.cuda.ExternalStream(ctx.stream, device=dev)
ip, ix, da = pkg.generators.laplace3d(ctx, *dims, dtype=dtype)
n = dims[0] * dims[1] * dims[2]
nnz = int(ix.numel())
b = torch.full((n,), 5.0, dtype=torch.float64, device=dev)
is_diag = da > 0                     # diag 6 / off -1 as generated
torch.cuda.synchronize()


def rescale(tau):
    """I + tau L, written into the borrowed tensor in place"""
    da.copy_(torch.where(is_diag, torch.full_like(da, 1.0 + 6.0 * tau), torch.full_like(da, -tau)))
    torch.cuda.synchronize()


def create():
    return pkg.Solver(ctx, n, nnz, da, ip, ix, 1, flags=pkg._lib.MATRIX_ON_DEVICE, dtype=dtype)


def window(s):
    s.set_rhs(b, None, on_device=True)
    s.iterate(16)
    ctx.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    s.iterate(args.iters)
    e1.record(stream)
    ctx.synchronize()
    return args.iters / (e0.elapsed_time(e1) * 1e-3)


s = create()
assert s.row_codes > 0 and s.value_codes == 2, (s.value_codes, s.row_codes)
window(s)                           # graphs captured
ms = {"fast": [], "rebuild": [], "recreate": []}
rates = {k: [] for k in ms}
outcomes = {k: set() for k in ms}
hist = {}
for rep in range(args.reps):
    tau = 0.25 + rep / 64.0
    for way in ms:
        rescale(tau)
        if way == "rebuild":
            da[nnz // 2] *= 1.5
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        if way == "recreate":
            s.close()
            s = create()
        else:
            s.refresh_values()
        ctx.synchronize()
        ms[way].append((time.perf_counter() - t0) * 1e3)
        outcomes[way].add(s.last_refresh)
        rates[way].append(window(s))
        if rep == 0 and way != "rebuild":
            hist[way] = s.history().copy()
        assert np.all(np.isfinite(s.history())), way
assert outcomes == {"fast": {1}, "rebuild": {2}, "recreate": {0}}, outcomes
assert np.array_equal(hist["fast"], hist["recreate"]), "history after the fast path differs from a fresh handle's"
med_rate = {k: statistics.median(v) for k, v in rates.items()}
for way in ms:
    print(json.dumps({"grid": args.grid, "dtype": "f64", "rows": n, "nnz": nnz, "way": way, "last_refresh": sorted(outcomes[way])[0],
                      "reps": args.reps, "ms_per_call": {"median": round(statistics.median(ms[way]), 3), "min": round(min(ms[way]), 3),
                                                         "max": round(max(ms[way]), 3)},
                      "it_per_s_after": {"median": round(med_rate[way], 1), "min": round(min(rates[way]), 1), "max": round(max(rates[way]), 1)},
                      "iters_per_window": args.iters, "rate_over_recreate": round(med_rate[way] / med_rate["recreate"], 4),
                      "history_equal_fresh_handle": bool(way == "fast")}), flush=True)
s.close()
ctx.close()
