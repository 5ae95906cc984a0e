#!/usr/bin/env python3
"""The per-right-hand-side tolerance stop on the device (Solver.solve_until / cgamd_solver_iterate_until) against what a user runs
without it.

  (a) the reference's additive-Schwarz step solved to a tolerance (p_h-PY_C-CL.py:1916-1921): complex64, 9 systems on the pattern
      of local_rect (symmetric scalings of its matrix, as scripts/batched_ab.py makes them), right-hand side r = 10^(-r/2) b so that
      the stopping iterations differ, at 16 384 and 250 000 rows, plain and with the Jacobi preconditioner of every system.
        until      ONE batched handle, one solve_until for all nine
        sequence   nine single-system handles, nine solve_tol calls one after another (the device-side stop of the resident loop
                   where the handle has one, else the host scheme _run_to_tol)
  (b) the 10M-row 7-point fp64 system of bench.py, one right-hand side b = A u:
        until      solve_until on the handle
        host       solve_tol on the same handle: the host scheme (history read back per chunk, a re-run after an overshoot)
The tolerance of a leg comes from a fixed-count probe run of the `until` handle: the norm column 0 has after --probe iterations,
so the longest solve takes about that many.  Both forms of a leg get the same host right-hand sides and return x, the iteration
counts and the history to the host; a timed window is the whole call on the host clock (both synchronise before they return).  The
forms alternate inside every one of --reps repeats after one untimed round; medians with the extremes, one JSON line per (leg,
form), the iteration counts of both forms beside them.  The driver starts one child process per leg, each under its own time limit,
chained: a leg that fails or runs out of time ends the run.  Lines are appended to --out and echoed.
usage: until_ab.py [--sizes 128,500] [--systems 9] [--probe 300] [--reps 7] [--big 250,200,200] [--legs a,b]"""
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
ap.add_argument("--sizes", default="128,500", help="(a): nodes per side of the local_rect grid (128: 16 384 rows, 500: 250 000)")
ap.add_argument("--systems", type=int, default=9)
ap.add_argument("--probe", type=int, default=300, help="iterations of the probe run that sets the tolerance")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--big", default="250,200,200", help="(b): nx,ny,nz of the 7-point grid")
ap.add_argument("--legs", default="a,b")
ap.add_argument("--step-timeout", type=int, default=240, help="time limit of one leg, in seconds")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "until", "ab.log"))
ap.add_argument("--child", default="", help=argparse.SUPPRESS)
args = ap.parse_args()

if not args.child:                      # the driver: opens no GPU itself
    legs = []
    if "a" in args.legs.split(","):
        legs += [f"a:{side}:{pre}" for side in args.sizes.split(",") for pre in ("none", "jacobi")]
    if "b" in args.legs.split(","):
        legs.append("b:" + args.big)
    lines = [f"# scripts/until_ab.py --systems {args.systems} --probe {args.probe} --reps {args.reps}"]
    for leg in legs:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", leg, "--systems", str(args.systems), "--probe", str(args.probe),
               "--reps", str(args.reps)]
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

pkg = importlib.import_module("conjugate-gradient-pyopencl_amd")
lib = pkg._lib.load()
ctx = pkg.Context(0)
dev = torch.device("cuda", 0)


def summary(samples):
    return {"median": round(statistics.median(samples), 3), "min": round(min(samples), 3), "max": round(max(samples), 3)}


def timed(fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    out = fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def alternate(forms):
    """{name: fn} -> {name: ([ms per repeat], last result)}; one untimed round first"""
    got = {name: ([], None) for name in forms}
    for rep in range(args.reps + 1):
        for name, fn in forms.items():
            ms, out = timed(fn)
            if rep:
                got[name][0].append(ms)
            got[name] = (got[name][0], out)
    return got


kind, _, rest = args.child.partition(":")
if kind == "a":
    side, pre = rest.split(":")
    side, nsys, DT = int(side), args.systems, np.complex64
    M = None if pre == "none" else "jacobi"
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
    torch.cuda.synchronize()
    flags = pkg._lib.MATRIX_ON_DEVICE
    batched = pkg.Solver(ctx, n, nnz, stack, ip, ix, nsys, flags=flags, dtype=DT, batched=True)
    singles = [pkg.Solver(ctx, n, nnz, vals[r], ip, ix, 1, flags=flags, dtype=DT) for r in range(nsys)]
    for h in [batched] + singles:
        h.set_preconditioner(M)
    b1 = np.linspace(1.0, 2.0, n).astype(DT)
    B = np.stack([b1 * DT(10.0 ** (-r / 2.0)) for r in range(nsys)])
    batched.set_rhs(B.reshape(-1))
    batched.iterate(args.probe)
    norms = np.sqrt(np.abs(batched.history()[:, 0].astype(np.complex128)))
    tol = float(norms[-1]) * 1.0001
    maxit = 4 * args.probe
    got = alternate({
        "until": lambda: batched.solve_until(B.reshape(-1), tol=tol, maxit=maxit),
        "sequence": lambda: [h.solve_tol(B[r], tol=tol, maxit=maxit) for r, h in enumerate(singles)],
    })
    its_u = [int(v) for v in got["until"][1][1]]
    its_s = [int(o[1]) for o in got["sequence"][1]]
    xs = np.concatenate([o[0] for o in got["sequence"][1]])
    xdiff = float(np.linalg.norm(got["until"][1][0] - xs) / np.linalg.norm(xs))
    for name in ("until", "sequence"):
        print(json.dumps({"leg": "a", "rows": n, "nnz": nnz, "systems": nsys, "dtype": "complex64", "pcg": pre, "form": name,
                          "tol": tol, "maxit": maxit, "iterations": its_u if name == "until" else its_s,
                          "loop_launches": lib.cgamd_solver_loop_launches((batched if name == "until" else singles[0]).handle),
                          "ms_per_solve_of_all_systems": summary(got[name][0]), "reps": args.reps}), flush=True)
    print(json.dumps({"leg": "a", "rows": n, "pcg": pre, "same_iterations": its_u == its_s, "x_rel_diff_until_vs_sequence": xdiff,
                      "until_over_sequence_speedup": round(statistics.median(got["sequence"][0]) / statistics.median(got["until"][0]), 3)}),
          flush=True)
    for h in [batched] + singles:
        h.close()
else:
    nx, ny, nz = (int(v) for v in rest.split(","))
    ip, ix, da = pkg.generators.laplace3d(ctx, nx, ny, nz, dtype=np.float64)
    n, nnz = nx * ny * nz, int(ix.numel())
    s = pkg.Solver(ctx, n, nnz, da, ip, ix, 1, flags=pkg._lib.MATRIX_ON_DEVICE, dtype=np.float64)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    u = (0.5 + torch.rand(n, device=dev, dtype=torch.float64, generator=gen)).contiguous()
    bd = torch.empty_like(u)
    torch.cuda.synchronize()
    s.spmv(u, bd)                       # b = A u: the residual norm falls from the first iteration on
    ctx.synchronize()
    b = bd.cpu().numpy()
    s.set_rhs(b)
    s.iterate(args.probe)
    tol = float(np.sqrt(abs(s.history()[-1, 0]))) * 1.0001
    maxit = 4 * args.probe
    got = alternate({
        "until": lambda: s.solve_until(b, tol=tol, maxit=maxit),
        "host": lambda: s.solve_tol(b, tol=tol, maxit=maxit),
    })
    for name in ("until", "host"):
        print(json.dumps({"leg": "b", "rows": n, "nnz": nnz, "dtype": "float64", "form": name, "tol": tol, "maxit": maxit,
                          "iterations": int(np.asarray(got[name][1][1]).reshape(-1)[0]), "ms_per_solve": summary(got[name][0]),
                          "reps": args.reps}), flush=True)
    print(json.dumps({"leg": "b", "rows": n, "until_over_host_speedup":
                      round(statistics.median(got["host"][0]) / statistics.median(got["until"][0]), 3)}), flush=True)
    s.close()
ctx.close()
