#!/usr/bin/env python3
"""Solution projection (Solver.enable_projection / cgamd_solver_set_rhs_projected / cgamd_solver_projection_update) against the same
handle's solve from zero, in ONE process on ONE GPU, at one commit.

Workload: the headline system, the 7-point Laplacian on 250 x 200 x 200 (10M rows) in fp64, and the moving-source sequence of the
tests scaled to the grid: with xs = linspace(0, 1, rows), b_t = exp(-(xs - 0.2 - 0.02 t)^2 / 0.01) + 1, t = 0 ... 11, every solve to
1e-8 ||b_t||, capacity K = 8, drop_tol 0.  Matrix, b and x stay on the device.
Forms: plain CG and PCG with the grid multigrid, each from zero (set_rhs, iterate_until) and projected (set_rhs_projected,
iterate_until, projection_update -- the update is inside the window).  The four forms alternate inside every one of --reps repeats
after one untimed round; a window is one whole sequence of 12 solves on the host clock, the stream drained on both sides (medians
with the extremes).  Recorded per form: ms per sequence, ms and iterations of every solve (last repeat), the slots held.
The kernels: windows of --calls calls of cgamd_projection_dots and cgamd_projection_combine on 8 slots of random data of the same
size, GB/s by the byte model of include/cgamd.h ((8 + 1) n V and (8 + 2) n V) against 8 TB/s; the store pass has no entry of its
own: the guess and the update as a whole are timed on the handle (--calls each) and priced by the same byte model without the SpMVs.

The driver opens no GPU: the measurement is a child process under its own time limit.  Lines are appended to --out and echoed.
usage: projection_ab.py [--grid 250x200x200] [--reps 7] [--solves 12] [--capacity 8] [--out profiles/projection/ab.log]"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--grid", default="250x200x200")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--solves", type=int, default=12)
ap.add_argument("--capacity", type=int, default=8)
ap.add_argument("--rel-tol", type=float, default=1e-8)
ap.add_argument("--maxit", type=int, default=20000)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--forms", default="plain,multigrid")
ap.add_argument("--step-timeout", type=int, default=900, help="time limit of the measurement, in seconds")
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "projection", "ab.log"))
ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
args = ap.parse_args()

if not args.child:                      # the driver
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--grid", args.grid, "--reps", str(args.reps), "--solves", str(args.solves),
           "--capacity", str(args.capacity), "--rel-tol", str(args.rel_tol), "--maxit", str(args.maxit), "--calls", str(args.calls),
           "--forms", args.forms]
    lines = [f"# scripts/projection_ab.py --grid {args.grid} --reps {args.reps} --solves {args.solves} --capacity {args.capacity} "
             f"--rel-tol {args.rel_tol} --forms {args.forms}"]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
        lines += [l for l in p.stdout.splitlines() if l.startswith("{")]
        if p.returncode != 0:
            lines.append(f"# the measurement failed (exit status {p.returncode}); stopped here\n" + p.stderr[-2000:])
    except subprocess.TimeoutExpired:
        lines.append(f"# the measurement ran into its time limit of {args.step_timeout} s; stopped here")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    sys.exit(1 if lines[-1].startswith("# the measurement") else 0)

# ---- the measurement
sys.path.insert(0, HERE)
import torch  # noqa: E402

pkg = importlib.import_module("conjugate-gradient-pyopencl_amd")
L = pkg._lib
lib = L.load()
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
ctx = pkg.Context(0)
dims = tuple(int(v) for v in args.grid.split("x"))
dims = dims + (1,) * (3 - len(dims))
n = int(np.prod(dims))
indptr, cols, data = pkg.generators.laplace3d(ctx, *dims, dtype=np.float64)
nnz = int(data.numel())
xs = torch.linspace(0.0, 1.0, n, dtype=torch.float64, device=dev)
B = [torch.exp(-((xs - 0.2 - 0.02 * t) ** 2) / 0.01) + 1.0 for t in range(args.solves)]
TOL = [args.rel_tol * float(torch.linalg.vector_norm(b)) for b in B]
x = torch.zeros_like(B[0])
torch.cuda.synchronize()
K, V = args.capacity, 8


def drain():
    ctx.synchronize()
    torch.cuda.synchronize()


def timed(fn):
    drain()
    t0 = time.perf_counter()
    out = fn()
    drain()
    return (time.perf_counter() - t0) * 1e3, out


def summary(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


say = lambda d: print(json.dumps(d), flush=True)      # noqa: E731
handles = {}
for form in args.forms.split(","):
    for start in ("zero", "projected"):
        s = pkg.Solver(ctx, n, nnz, data, indptr, cols, 1, flags=L.MATRIX_ON_DEVICE, dtype=np.float64)
        if form == "multigrid":
            s.set_preconditioner(("multigrid", dims))
        if start == "projected":
            s.enable_projection(K, 0.0)
        handles[(form, start)] = s
say({"rows": n, "grid": list(dims), "solves": args.solves, "capacity": K, "rel_tol": args.rel_tol,
     "launches_per_iteration": {"/".join(k): lib.cgamd_solver_loop_launches(s.handle) for k, s in handles.items()},
     "dots_grid": lib.cgamd_projection_dots_grid(1, n)})


def sequence(key):
    """the 12 solves of one form; returns (ms, iterations) per solve"""
    s, projected = handles[key], key[1] == "projected"
    if projected:
        s.projection_clear()
    out = []
    for b, tol in zip(B, TOL):
        def solve():
            if projected:
                s.set_rhs_projected(b, on_device=True)
            else:
                s.set_rhs(b, None, on_device=True)
            its = s.iterate_until(tol, args.maxit, 8)
            s.x(x)
            if projected:
                s.projection_update()
            return int(its[0])
        out.append(timed(solve))
    return out


total, last = {k: [] for k in handles}, {}
for rep in range(args.reps + 1):
    for key in handles:
        ms, per = timed(lambda: sequence(key))
        if rep:
            total[key].append(ms)
        last[key] = per
for key, s in handles.items():
    zero = statistics.median(total[(key[0], "zero")])
    say({"form": key[0], "start": key[1], "ms_per_sequence": summary(total[key]), "reps": args.reps,
         "speedup_over_zero": round(zero / statistics.median(total[key]), 3),
         "iterations": [its for _, its in last[key]], "ms_per_solve": [round(ms, 2) for ms, _ in last[key]],
         "slots_held": s.projection_count()})

# ---- the kernels, on random data of the same size
gen = torch.Generator(device=dev)
gen.manual_seed(7)
W = torch.randn((K, n), dtype=torch.float64, device=dev, generator=gen)
v = torch.randn((n,), dtype=torch.float64, device=dev, generator=gen)
c = torch.randn((K,), dtype=torch.float64, device=dev, generator=gen)
out = torch.zeros((K,), dtype=torch.float64, device=dev)
y = torch.zeros_like(v)
mask = (1 << K) - 1
vp = lambda t: L.ptr(t)      # noqa: E731


def window(fn):
    fn()
    got = []
    for _ in range(args.reps):
        ms, _ = timed(lambda: [fn() for _ in range(args.calls)])
        got.append(ms / args.calls)
    return got


def gbs(bytes_, ms):
    return round(bytes_ / (statistics.median(ms) * 1e-3) / 1e9, 1)


dots = window(lambda: L.check(lib.cgamd_projection_dots(ctx.handle, 1, n, n, K, mask, vp(W), n, vp(v), 1, vp(out))))
comb = window(lambda: L.check(lib.cgamd_projection_combine(ctx.handle, 1, n, n, K, mask, vp(W), n, vp(v), vp(c), 1, vp(y), 1)))
groups = -(-K // 8)
say({"kernel": "dots", "slots": K, "ms": summary(dots), "bytes": (K + groups) * n * V, "GB_per_s": gbs((K + groups) * n * V, dots), "of_8_TB_per_s": round(gbs((K + groups) * n * V, dots) / 8000, 3)})
say({"kernel": "combine", "slots": K, "ms": summary(comb), "bytes": (K + 2) * n * V, "GB_per_s": gbs((K + 2) * n * V, comb), "of_8_TB_per_s": round(gbs((K + 2) * n * V, comb) / 8000, 3)})

# the guess and the update as a whole, on the plain projected handle with a full basis (the store pass is part of the update)
key = (args.forms.split(",")[0], "projected")
s = handles[key]
sequence(key)
m = s.projection_count()
plain = window(lambda: s.set_rhs(B[-1], None, on_device=True))
guess = window(lambda: s.set_rhs_projected(B[-1], on_device=True))


def update():
    s.set_rhs_projected(B[-1], on_device=True)
    s.iterate(8)
    drain()
    t0 = time.perf_counter()
    s.projection_update()
    drain()
    return (time.perf_counter() - t0) * 1e3


update()
upd = [update() for _ in range(args.reps)]
spmv_bytes = lib.cgamd_solver_spmv_moved_bytes(s.handle)
g_bytes = (m + -(-m // 8) + 1) * n * V
live = m - 1 if m == K else m
u_bytes = ((4 if m == K else 3) + live + -(-live // 8) + 4 + live + 2 + 2) * n * V
say({"step": "guess", "slots_held": m, "set_rhs_ms": summary(plain), "set_rhs_projected_ms": summary(guess),
     "guess_ms": round(statistics.median(guess) - statistics.median(plain), 3), "bytes": g_bytes,
     "GB_per_s": round(g_bytes / max(1e-9, (statistics.median(guess) - statistics.median(plain)) * 1e-3) / 1e9, 1)})
say({"step": "update", "slots_held": m, "ms": summary(upd), "bytes_without_spmv": u_bytes, "spmv_moved_bytes": int(spmv_bytes),
     "GB_per_s_with_two_spmv": round((u_bytes + 2 * spmv_bytes) / (statistics.median(upd) * 1e-3) / 1e9, 1)})
for s in handles.values():
    s.close()
ctx.close()
