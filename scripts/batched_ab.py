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
--mg: the multigrid leg (profiles/batched/mg_ab.log).  Per case, solves to 1e-6 ||b_r|| per system through iterate_until, medians of
--reps solves on the host clock (set_rhs from a device vector, iterate_until, synchronise): ONE batched handle with
cgamd_solver_set_preconditioner_batched_multigrid against (a) nine single-system multigrid handles one after another and (b) the
batched Jacobi handle.  Cases: 9 fp64 variable-coefficient 5-point systems (the 2-D form of the tests' variable7: D^(1/2) (Laplacian +
shift) D^(1/2), seeds 3 + r) at 128^2 and 500^2 rows, and the local_rect shape of the other legs at 16 384 rows in complex64.  Logged
per form: the iterations of every system, ms per solve (all systems), us per iteration (that time over the largest iteration count)
and the setup time of the preconditioner.  One child process per case under --step-timeout, chained.
usage: batched_ab.py [--sizes 128,500] [--systems 9] [--iters 400] [--warmup 50] [--reps 7] [--pcg jacobi|line [--stride 1]] [--mg]"""
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
ap.add_argument("--mg", action="store_true", help="multigrid leg: batched multigrid PCG against nine single handles and batched Jacobi")
ap.add_argument("--mg-case", default="", help=argparse.SUPPRESS)
ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
args = ap.parse_args()
MG_OUT = os.path.join(ROOT, "profiles", "batched", "mg_ab.log")
if args.mg and not args.child:          # the driver: opens no GPU itself
    lines = [f"# scripts/batched_ab.py --mg --systems {args.systems} --reps {args.reps}"]
    for case in ("var5:128", "var5:500", "local_rect:128"):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--mg", "--mg-case", case, "--systems", str(args.systems),
               "--reps", str(args.reps)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            lines.append(f"# case {case} ran into its time limit of {args.step_timeout} s; stopped here")
            break
        lines += [l for l in r.stdout.splitlines() if l.startswith("{")]
        if r.returncode != 0:
            lines.append(f"# case {case} failed with exit status {r.returncode}; stopped here\n" + r.stderr[-2000:])
            break
    out = MG_OUT if args.out == ap.get_default("out") else args.out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    sys.exit(1 if lines[-1].startswith("# case") else 0)
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


def mg_case(case):
    """one case of the multigrid leg: the three forms on the same systems, right-hand sides and tolerances"""
    import scipy.sparse as sp
    kind, side = case.split(":")
    side = int(side)
    nsys = args.systems
    dims = (side, side, 1)
    if kind == "var5":
        dt = np.float64
        t = sp.diags([-np.ones(side - 1), 2 * np.ones(side), -np.ones(side - 1)], [-1, 0, 1], format="csr")
        eye = sp.identity(side, format="csr")
        lap = sp.csr_matrix(sp.kron(eye, t) + sp.kron(t, eye))
        mats = []
        for r in range(nsys):
            rng = np.random.default_rng(3 + r)
            d = sp.diags(np.sqrt(rng.uniform(0.5, 2.0, side * side)))
            A = sp.csr_matrix(d @ (lap + sp.diags(rng.uniform(0.0, 0.5, side * side))) @ d)
            A.sort_indices()
            mats.append(A)
        ip, ix = mats[0].indptr.astype(np.int32), mats[0].indices.astype(np.int32)
        vals = [A.data.astype(dt) for A in mats]
    else:
        dt = np.complex64
        ipd, ixd, dad = pkg.generators.local_rect(ctx, side, 10.0, 10.0, 10.0, 1.0, side, side, dtype=dt)
        ip, ix, da = ipd.cpu().numpy().astype(np.int32), ixd.cpu().numpy().astype(np.int32), dad.cpu().numpy()
        rows = np.repeat(np.arange(len(ip) - 1), np.diff(ip))
        vals = []
        for r in range(nsys):
            s_ = np.random.default_rng(100 + r).uniform(0.8, 1.25, len(ip) - 1).astype(np.float32)
            vals.append((da * s_[rows] * s_[ix]).astype(dt))
    n, nnz = len(ip) - 1, len(ix)
    rng = np.random.default_rng(11)
    B = rng.standard_normal((nsys, n)).astype(dt)
    tol = 1e-6 * np.linalg.norm(B, axis=1)
    bd = torch.from_numpy(B.reshape(-1)).to(dev)
    b1 = [torch.from_numpy(B[r].copy()).to(dev) for r in range(nsys)]
    M = ("multigrid", dims)
    forms = {
        "batched multigrid": ([pkg.Solver(ctx, n, nnz, np.concatenate(vals), ip, ix, nsys, batched=True)], M),
        "nine multigrid handles": ([pkg.Solver(ctx, n, nnz, vals[r], ip, ix, 1) for r in range(nsys)], M),
        "batched jacobi": ([pkg.Solver(ctx, n, nnz, np.concatenate(vals), ip, ix, nsys, batched=True)], "jacobi"),
    }
    maxit = 4000

    def solve(hs):
        its = []
        for k, h in enumerate(hs):
            h.set_rhs(bd if h.n_rhs == nsys else b1[k], None, on_device=True)
            its += [int(v) for v in h.iterate_until(tol if h.n_rhs == nsys else tol[k:k + 1], maxit)]
        ctx.synchronize()
        return its

    results = {}
    for name, (hs, m) in forms.items():
        setup = []
        for _ in range(3):              # the setup: set_preconditioner on every handle of the form, synchronised
            ctx.synchronize()
            t0 = time.perf_counter()
            for h in hs:
                h.set_preconditioner(m)
            ctx.synchronize()
            setup.append((time.perf_counter() - t0) * 1e3)
        its = solve(hs)                 # warm-up: captures the graphs
        solve(hs)
        results[name] = {"its": its, "setup": setup, "ms": []}
    for rep_ in range(args.reps):       # the forms alternate inside every repeat
        for name, (hs, m) in forms.items():
            ctx.synchronize()
            t0 = time.perf_counter()
            solve(hs)
            results[name]["ms"].append((time.perf_counter() - t0) * 1e3)
    for name, (hs, m) in forms.items():
        r = results[name]
        med = statistics.median(r["ms"])
        print(json.dumps({"case": case, "rows": n, "nnz": nnz, "systems": nsys, "dtype": np.dtype(dt).name, "form": name, "handles": len(hs),
                          "levels": len(hs[0].mg_levels()), "loop_launches": lib.cgamd_solver_loop_launches(hs[0].handle),
                          "iterations": r["its"], "converged": bool(max(r["its"]) < maxit), "reps": args.reps,
                          "ms_per_solve_all_systems": summary(r["ms"]),
                          "us_per_iteration": round(med * 1e3 / max(1, max(r["its"])), 3),
                          "setup_ms": summary(r["setup"]), "iter_moved_bytes": sum(h.iter_moved_bytes for h in hs)}), flush=True)
    ma, mb, mc = (statistics.median(results[k]["ms"]) for k in forms)
    print(json.dumps({"case": case, "rows": n, "systems": nsys, "batched_multigrid_over_nine_handles_speedup": round(mb / ma, 3),
                      "batched_multigrid_over_batched_jacobi_speedup": round(mc / ma, 3)}), flush=True)
    for hs, _ in forms.values():
        for h in hs:
            h.close()


if args.mg:
    mg_case(args.mg_case)
    ctx.close()
    sys.exit(0)


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
