#!/usr/bin/env python3
"""Batched CG (one pattern, a matrix of its own per right-hand side) against what a user runs without it.

The shape is the reference's additive-Schwarz step with variable coefficients (as_prec with VarCoeff, p_h-PY_C-CL.py:1970-1985):
complex64, 9 sub-domain matrices on the pattern of local_rect, a fixed number of CG iterations.  Per size (16 384 and 250 000 rows):
  (a) batched     ONE batched handle (cgamd_solver_create_batched) on the 9 matrices
  (b) sequence    what a UseCG == 4 user runs today: nine single-system handles, iterated one after another
  (c) shared      the shared-matrix handle of the same shape (one matrix, 9 right-hand sides): the floor that reads one matrix
The 9 matrices are symmetric scalings of local_rect's (a[j] * s[row] * s[col], s in [0.8, 1.25]): same pattern, different values.
Method: every handle is created and warmed up first (`--warmup` iterations each); a timed window is `--iters` iterations between two
device events on the handles' stream (and a host clock around the same window, ending in a synchronise); (a), (b), (c) alternate
inside every one of `--reps` repeats, and the median over the repeats is reported with the extremes.  One JSON line per (size, form).
The batched SpMV alone (Solver.spmv on device vectors, `--spmv-reps` launches per window) is priced on
cgamd_solver_spmv_moved_bytes against 8 TB/s.
--pcg {jacobi,line}: the preconditioned leg.  (a) the batched handle with one M per system (cgamd_solver_set_preconditioner_batched_jacobi
/ _batched_line at --stride) against (b) the nine single-system handles with the same preconditioner of their own matrix
(cgamd_solver_set_preconditioner_jacobi / _line), same method; (c) and the SpMV part are left out.  The driver starts one child
process per size, each under its own time limit (--step-timeout), chained: a size that fails or runs out of time ends the run.  The
lines are appended to --out (profiles/batched/pcg_ab.log: one log for both legs) and are echoed.
usage: batched_ab.py [--sizes 128,500] [--systems 9] [--iters 400] [--warmup 50] [--reps 7] [--pcg jacobi|line [--stride 1]]"""
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
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="128,500", help="nodes per side of the local_rect grid (128: 16 384 rows, 500: 250 000)")
ap.add_argument("--systems", type=int, default=9)
ap.add_argument("--iters", type=int, default=400)
ap.add_argument("--warmup", type=int, default=50)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--spmv-reps", type=int, default=200)
ap.add_argument("--pcg", default="", choices=("", "jacobi", "line"), help="preconditioned leg: batched PCG against single-system PCG handles")
ap.add_argument("--stride", type=int, default=1, help="--pcg line: distance of the coupled rows (1: the x-lines of the grid)")
ap.add_argument("--step-timeout", type=int, default=300, help="--pcg: time limit of one size, in seconds")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batched", "pcg_ab.log"))
ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
args = ap.parse_args()
if args.pcg and not args.child:         # the driver: opens no GPU itself
    head = f"# scripts/batched_ab.py --pcg {args.pcg}" + (f" --stride {args.stride}" if args.pcg == "line" else "")
    lines = [head + f" --systems {args.systems} --iters {args.iters} --warmup {args.warmup} --reps {args.reps}"]
    for side in args.sizes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--pcg", args.pcg, "--stride", str(args.stride), "--sizes", side,
               "--systems", str(args.systems), "--iters", str(args.iters), "--warmup", str(args.warmup), "--reps", str(args.reps)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            lines.append(f"# size {side} ran into its time limit of {args.step_timeout} s; stopped here")
            break
        lines += [l for l in r.stdout.splitlines() if l.startswith("{")]
        if r.returncode != 0:
            lines.append(f"# size {side} failed with exit status {r.returncode}; stopped here\n" + r.stderr[-2000:])
            break
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:          # one log for both legs: every run adds its header and lines
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    sys.exit(1 if lines[-1].startswith("# size") else 0)
M = None if not args.pcg else "jacobi" if args.pcg == "jacobi" else ("line", args.stride)
pkg = importlib.import_module("conjugate-gradient-pyopencl_amd")
lib = pkg._lib.load()
ctx = pkg.Context(0)
dev = torch.device("cuda", 0)
HBM = 8e12
DT = np.complex64
stream = torch.cuda.ExternalStream(ctx.stream, device=dev) if ctx.stream else None      # events go on the handles' own stream


def window(fn):
    """fn() between two events on the handles' stream, and on the host clock up to the synchronise: (event ms, wall ms)"""
    ctx.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    if stream is not None:
        e0.record(stream)
    fn()
    if stream is not None:
        e1.record(stream)
    ctx.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    return (e0.elapsed_time(e1) if stream is not None else float("nan")), wall


def summary(samples):
    return {"median": round(statistics.median(samples), 3), "min": round(min(samples), 3), "max": round(max(samples), 3)}


for side in (int(v) for v in args.sizes.split(",")):
    nsys = args.systems
    ip, ix, da = pkg.generators.local_rect(ctx, side, 10.0, 10.0, 10.0, 1.0, side, side, dtype=DT)
    n, nnz = int(ip.numel()) - 1, int(ix.numel())
    rows = torch.repeat_interleave(torch.arange(n, device=dev), (ip[1:] - ip[:-1]).long())
    gen = torch.Generator(device=dev)
    vals = []
    for r in range(nsys):
        gen.manual_seed(100 + r)
        s_ = (0.8 + 0.45 * torch.rand(n, device=dev, dtype=torch.float64, generator=gen)).to(torch.float32)
        vals.append((da * s_[rows] * s_[ix.long()]).contiguous())
    stack = torch.cat(vals).contiguous()
    b1 = torch.linspace(1.0, 2.0, n, device=dev, dtype=torch.float64).to(torch.complex64)
    b = b1.repeat(nsys).contiguous()
    torch.cuda.synchronize()
    flags = pkg._lib.MATRIX_ON_DEVICE
    forms = {
        "batched": [pkg.Solver(ctx, n, nnz, stack, ip, ix, nsys, flags=flags, dtype=DT, batched=True)],
        "sequence": [pkg.Solver(ctx, n, nnz, vals[r], ip, ix, 1, flags=flags, dtype=DT) for r in range(nsys)],
        "shared": [pkg.Solver(ctx, n, nnz, vals[0], ip, ix, nsys, flags=flags, dtype=DT)],
    }
    if M is not None:
        del forms["shared"]             # one matrix for all right-hand sides has no per-system M
    for name, hs in forms.items():
        for h in hs:
            if M is not None:
                h.set_preconditioner(M)
            h.set_rhs(b if h.n_rhs == nsys else b1, None, on_device=True)
            h.iterate(args.warmup)
    ctx.synchronize()
    # same iterates: the batched handle against the sequence, after the warm-up, on the history the handles keep
    hb = forms["batched"][0].history()[-1]
    hs_ = np.array([h.history()[-1, 0] for h in forms["sequence"]])
    agree = float(np.max(np.abs(hb - hs_) / np.abs(hs_)))
    times = {name: {"ev": [], "wall": []} for name in forms}
    for rep in range(args.reps):
        for name, hs in forms.items():
            ev, wall = window(lambda hs=hs: [h.iterate(args.iters) for h in hs])
            times[name]["ev"].append(ev / args.iters * 1e3)
            times[name]["wall"].append(wall / args.iters * 1e3)
    for name, hs in forms.items():
        rec = {"rows": n, "nnz": nnz, "systems": nsys, "dtype": "complex64", "form": name, "handles": len(hs),
               "loop_launches": lib.cgamd_solver_loop_launches(hs[0].handle), "iters_per_window": args.iters, "reps": args.reps,
               "us_per_iteration_all_systems_events": summary(times[name]["ev"]),
               "us_per_iteration_all_systems_wall": summary(times[name]["wall"]),
               "iter_moved_bytes": sum(h.iter_moved_bytes for h in hs)}
        if name == "batched":
            rec["delta_vs_sequence_after_warmup_max_rel"] = agree
        if M is not None:
            rec["pcg"] = args.pcg if args.pcg == "jacobi" else f"line, stride {args.stride}"
            rec["preconditioner_source"] = hs[0].preconditioner_source
        print(json.dumps(rec), flush=True)
    if M is not None:                   # the preconditioned leg ends here
        ma, mb = (statistics.median(times[k]["ev" if stream is not None else "wall"]) for k in ("batched", "sequence"))
        print(json.dumps({"rows": n, "systems": nsys, "pcg": args.pcg, "batched_over_sequence_speedup": round(mb / ma, 3)}), flush=True)
        for hs in forms.values():
            for h in hs:
                h.close()
        del forms, vals, stack
        torch.cuda.empty_cache()
        continue
    ma, mb, mc = (statistics.median(times[k]["ev" if stream is not None else "wall"]) for k in ("batched", "sequence", "shared"))
    print(json.dumps({"rows": n, "systems": nsys, "batched_over_sequence_speedup": round(mb / ma, 3),
                      "batched_over_shared_time_ratio": round(ma / mc, 3)}), flush=True)
    # the batched SpMV alone
    sb = forms["batched"][0]
    x = b.clone()
    y = torch.empty_like(x)
    torch.cuda.synchronize()
    for _ in range(20):
        sb.spmv(x, y)
    samples = []
    for rep in range(args.reps):
        ev, wall = window(lambda: [sb.spmv(x, y) for _ in range(args.spmv_reps)])
        samples.append((ev if stream is not None else wall) / args.spmv_reps * 1e3)
    us = statistics.median(samples)
    print(json.dumps({"rows": n, "systems": nsys, "form": "batched spmv", "launch": sb.last_spmv_form(), "us_per_spmv": summary(samples),
                      "spmv_moved_bytes": sb.spmv_moved_bytes, "floor_us_at_8TBps": round(sb.spmv_moved_bytes / HBM * 1e6, 3),
                      "fraction_of_8TBps": round(sb.spmv_moved_bytes / HBM / (us * 1e-6), 4)}), flush=True)
    for hs in forms.values():
        for h in hs:
            h.close()
    del forms, vals, stack
    torch.cuda.empty_cache()
ctx.close()
