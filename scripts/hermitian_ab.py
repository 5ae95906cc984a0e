#!/usr/bin/env python3
"""CGAMD_HERMITIAN handles (conjugated recurrence, csrc/hermitian.hip) against an unflagged handle on the same matrix.

The yardstick is the unflagged handle on its launched loop: the tune keys `resident` 0 and `two_launch` 0 are set for the run, so both
handles run three / four launches per iteration and differ in the vector and scalar steps only (the SpMV kernel is the same; the flagged
one reads conj(d) for its fused dot).  The expectation is the byte-model ratio iter_moved_bytes(flagged) / iter_moved_bytes(unflagged):
12 vector passes against 10 (9.25 where the unflagged handle defers its x update, cgamd_solver_x_lag).  The README's box-to-box spread
is 10 %, so a measured ratio above model x 1.10 wants an explanation (DESIGN.md "Hermitian systems").  This is a measurement, not a test.
Shapes: a 500 x 500 magnetic Laplacian (tests/herm_ref.magnetic, flux 0.1, shift 0.05) in complex64 and a 2000 x 2000 one in
complex128.
Method: both handles are created and warmed up first; a timed window is set_rhs (outside the window), then `--iters` iterations between
two device events on the handles' stream; flagged and unflagged alternate inside every one of `--reps` windows (7), medians reported
with the extremes.  The driver opens no GPU: it starts one child process per shape, each under its own time limit (--step-timeout),
chained -- a shape that fails or runs out of time ends the run -- and appends the JSON lines to --out (profiles/hermitian/ab.log).
usage: hermitian_ab.py [--shapes 500:c64,2000:c128] [--iters 48] [--warmup 16] [--reps 7]"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="500:c64,2000:c128", help="nodes per side : value type, comma separated")
ap.add_argument("--iters", type=int, default=48)
ap.add_argument("--warmup", type=int, default=16)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--step-timeout", type=int, default=240, help="time limit of one shape, in seconds")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hermitian", "ab.log"))
ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
args = ap.parse_args()
if not args.child:          # the driver: opens no GPU itself
    lines = [f"# scripts/hermitian_ab.py --shapes {args.shapes} --iters {args.iters} --warmup {args.warmup} --reps {args.reps}"]
    for shape in args.shapes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--shapes", shape, "--iters", str(args.iters), "--warmup",
               str(args.warmup), "--reps", str(args.reps)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            lines.append(f"# shape {shape} ran into its time limit of {args.step_timeout} s; stopped here")
            break
        lines += [l for l in r.stdout.splitlines() if l.startswith("{")]
        if r.returncode != 0:
            lines.append(f"# shape {shape} failed with exit status {r.returncode}; stopped here\n" + r.stderr[-2000:])
            break
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    sys.exit(1 if lines[-1].startswith("# shape") else 0)

import torch  # noqa: E402
import herm_ref  # noqa: E402

pkg = importlib.import_module("conjugate-gradient-pyopencl_amd")
lib = pkg._lib.load()
for key in ("resident", "two_launch"):      # before any handle exists: a handle keeps the configuration it was created under
    pkg._lib.check(lib.cgamd_tune(key.encode(), 0))
ctx = pkg.Context(0)
dev = torch.device("cuda", 0)
stream = torch.cuda.ExternalStream(ctx.stream, device=dev) if ctx.stream else None
DT = {"c64": np.complex64, "c128": np.complex128}


def window(fn):
    """fn() between two events on the handles' stream: milliseconds"""
    ctx.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    ctx.synchronize()
    return e0.elapsed_time(e1)


def summary(samples):
    return {"median": round(statistics.median(samples), 3), "min": round(min(samples), 3), "max": round(max(samples), 3)}


for shape in args.shapes.split(","):
    side, dt = shape.split(":")
    side, dtype = int(side), DT[dt]
    A = herm_ref.magnetic(side, side, 0.1, 0.05)
    n, nnz = A.shape[0], A.nnz
    rng = np.random.default_rng(1)
    b = torch.from_numpy((rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(dtype)).to(dev)
    ip, ix = torch.from_numpy(A.indptr.astype(np.int32)).to(dev), torch.from_numpy(A.indices.astype(np.int32)).to(dev)
    da = torch.from_numpy(A.data.astype(dtype)).to(dev)
    del A
    torch.cuda.synchronize()
    forms = {"hermitian": pkg.Solver(ctx, n, nnz, da, ip, ix, 1, flags=pkg._lib.MATRIX_ON_DEVICE, dtype=dtype, hermitian=True),
             "unflagged": pkg.Solver(ctx, n, nnz, da, ip, ix, 1, flags=pkg._lib.MATRIX_ON_DEVICE, dtype=dtype)}
    spmv_form = {}
    for name, h in forms.items():
        h.set_rhs(b, None, on_device=True)
        h.iterate(args.warmup + args.iters)         # captures both graphs
        spmv_form[name] = h.last_spmv_form()        # (this thread's last SpMV launch: read before the other handle runs)
    ctx.synchronize()
    times = {name: [] for name in forms}
    for rep in range(args.reps):
        for name, h in forms.items():
            h.set_rhs(b, None, on_device=True)
            times[name].append(window(lambda h=h: h.iterate(args.iters)) / args.iters * 1e3)
    res = {}
    for name, h in forms.items():
        hist = h.history()
        res[name] = float(np.sqrt(abs(hist[-1, 0]) / abs(hist[0, 0])))
        print(json.dumps({"rows": n, "nnz": nnz, "dtype": np.dtype(dtype).name, "form": name, "hermitian": h.hermitian,
                          "loop_launches": lib.cgamd_solver_loop_launches(h.handle), "x_lag": lib.cgamd_solver_x_lag(h.handle),
                          "index_codes": h.index_codes, "value_codes": h.value_codes, "spmv": spmv_form[name],
                          "iters_per_window": args.iters, "reps": args.reps, "us_per_iteration": summary(times[name]),
                          "iter_moved_bytes": h.iter_moved_bytes, "sqrt_delta_ratio_after_window": res[name]}), flush=True)
    model = forms["hermitian"].iter_moved_bytes / forms["unflagged"].iter_moved_bytes
    measured = statistics.median(times["hermitian"]) / statistics.median(times["unflagged"])
    print(json.dumps({"rows": n, "dtype": np.dtype(dtype).name, "hermitian_over_unflagged_time": round(measured, 3),
                      "byte_model_ratio": round(model, 3), "measured_over_model": round(measured / model, 3),
                      "within_model_x_1.10": bool(measured <= model * 1.10)}), flush=True)
    for h in forms.values():
        h.close()
    del forms, da, ip, ix, b
    torch.cuda.empty_cache()
ctx.close()
