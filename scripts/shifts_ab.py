#!/usr/bin/env python3
"""Multi-shift CG (Solver.set_shifts / cgamd_solver_set_shifts) against separate solves, in ONE process on ONE GPU, at one commit.

Workload: the headline system, the 7-point Laplacian on 250 x 200 x 200 (10M rows) in fp64, --iterations iterations (200) from a
random right-hand side; shifts sigma_j = the first S of linspace(0.05, 2, 16), S in --shifts (1, 4, 8, 16).  Matrix, b and x stay on
the device.
A/B: ONE handle with S shifts in force against S + 1 single handles -- the seed and one per A + sigma_j I (the diagonal value class
changed, so each keeps the codes of the seed's SpMV form) -- run one after another.  The two sides alternate inside every one of
--reps repeats after one untimed round; a window is iterate(iterations) on the host clock, the stream drained on both sides, set_rhs
outside it (medians with the extremes).  The comparison is against those handles, never against a byte model.
Seed: the it/s of the handle without shifts (S = 0), the same windows.
The vector launch: windows of --calls calls of cgamd_shift_update on random data of the same size for every S, plain and
non-temporal (what a handle of this size launches), us and TB/s by the byte model of include/cgamd.h ((4 S + 1) n V), beside the
project's streaming yardsticks from this very run: cgamd_projection_combine and cgamd_projection_dots on 8 slots.

The driver opens no GPU: the measurement is a child process under its own time limit.  Lines are appended to --out and echoed.
usage: shifts_ab.py [--grid 250x200x200] [--reps 7] [--iterations 200] [--shifts 1,4,8,16] [--out profiles/shifts/ab.log]"""
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
ap.add_argument("--iterations", type=int, default=200)
ap.add_argument("--shifts", default="1,4,8,16")
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--step-timeout", type=int, default=900, help="time limit of the measurement, in seconds")
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "shifts", "ab.log"))
ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
args = ap.parse_args()

if not args.child:                      # the driver
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--grid", args.grid, "--reps", str(args.reps), "--iterations", str(args.iterations),
           "--shifts", args.shifts, "--calls", str(args.calls)]
    lines = [f"# scripts/shifts_ab.py --grid {args.grid} --reps {args.reps} --iterations {args.iterations} --shifts {args.shifts}"]
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
SHIFTS = [int(v) for v in args.shifts.split(",")]
SIGMA = np.linspace(0.05, 2.0, 16)
gen = torch.Generator(device=dev)
gen.manual_seed(7)
b = torch.randn((n,), dtype=torch.float64, device=dev, generator=gen)
torch.cuda.synchronize()
V, K = 8, args.iterations


def drain():
    ctx.synchronize()
    torch.cuda.synchronize()


def timed(fn):
    drain()
    t0 = time.perf_counter()
    fn()
    drain()
    return (time.perf_counter() - t0) * 1e3


def summary(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


say = lambda d: print(json.dumps(d), flush=True)      # noqa: E731


def handle(values):
    s = pkg.Solver(ctx, n, nnz, values, indptr, cols, 1, flags=L.MATRIX_ON_DEVICE, dtype=np.float64)
    s._values = values
    return s


def form(s):
    return {"row_codes": s.row_codes, "row_pairs": s.row_pairs, "value_codes": s.value_codes, "launches": lib.cgamd_solver_loop_launches(s.handle)}


def solve_window(s):
    s.set_rhs(b, None, on_device=True)
    return timed(lambda: s.iterate(K))


diag = float(data.max())                # the one positive value class of the Laplacian
seed, shifted = handle(data), handle(data)
singles = [handle(torch.where(data == diag, data + float(sg), data)) for sg in SIGMA[:max(SHIFTS)]]
say({"rows": n, "grid": list(dims), "iterations": K, "reps": args.reps, "sigma": [round(float(v), 4) for v in SIGMA[:max(SHIFTS)]],
     "seed_form": form(seed), "single_forms_differ": sorted({json.dumps(form(s)) for s in singles} - {json.dumps(form(seed))})})

# ---- S = 0: the seed alone
solve_window(seed)
t_seed = [solve_window(seed) for _ in range(args.reps)]
say({"shifts": 0, "ms": summary(t_seed), "us_per_iteration": round(statistics.median(t_seed) * 1e3 / K, 2),
     "iterations_per_s": round(K / (statistics.median(t_seed) * 1e-3), 1)})

# ---- A/B
for S in SHIFTS:
    shifted.set_shifts(SIGMA[:S])
    sides = {"shifted": [], "separate": []}
    for rep in range(args.reps + 1):
        one = solve_window(shifted)
        sep = sum(solve_window(s) for s in [seed] + singles[:S])
        if rep:
            sides["shifted"].append(one)
            sides["separate"].append(sep)
    m1, m2, m0 = statistics.median(sides["shifted"]), statistics.median(sides["separate"]), statistics.median(t_seed)
    say({"shifts": S, "shifted_ms": summary(sides["shifted"]), "separate_ms": summary(sides["separate"]),
         "speedup_over_separate": round(m2 / m1, 3), "launches": lib.cgamd_solver_loop_launches(shifted.handle),
         "us_per_iteration": {"shifted": round(m1 * 1e3 / K, 2), "separate": round(m2 * 1e3 / K, 2), "seed": round(m0 * 1e3 / K, 2),
                              "shift_steps": round((m1 - m0) * 1e3 / K, 2)},
         "iter_moved_bytes": int(shifted.iter_moved_bytes)})
shifted.set_shifts(None)

# ---- the vector launch alone, and the yardsticks, on random data of the same size
vp = lambda t: L.ptr(t)      # noqa: E731


def window(fn):
    fn()
    got = []
    for _ in range(args.reps):
        got.append(timed(lambda: [fn() for _ in range(args.calls)]) / args.calls)
    return got


def tbs(bytes_, ms):
    return round(bytes_ / (statistics.median(ms) * 1e-3) / 1e12, 3)


Smax = max(SHIFTS)
r = torch.randn((n,), dtype=torch.float64, device=dev, generator=gen)
xs = torch.randn((Smax, n), dtype=torch.float64, device=dev, generator=gen)
ds = torch.randn((Smax, n), dtype=torch.float64, device=dev, generator=gen)
coef = [torch.full((Smax,), v, dtype=torch.float64, device=dev) for v in (1e-3, 0.5, 0.25)]     # (values that keep the vectors finite)
for S in SHIFTS:
    rec = {"kernel": "shift_update", "shifts": S, "bytes": (4 * S + 1) * n * V}
    for label, knob in (("plain", 0), ("non_temporal", 1)):
        L.check(lib.cgamd_tune(b"vec_nt", knob))
        ms = window(lambda: L.check(lib.cgamd_shift_update(ctx.handle, 1, n, n, 1, S, vp(r), vp(xs), vp(ds), vp(coef[0]), vp(coef[1]), vp(coef[2]))))
        rec[label] = {"us": round(statistics.median(ms) * 1e3, 1), "min_us": round(min(ms) * 1e3, 1), "max_us": round(max(ms) * 1e3, 1),
                      "TB_per_s": tbs(rec["bytes"], ms)}
    L.check(lib.cgamd_tune(b"vec_nt", -1))
    say(rec)
W, c, out, y = xs[:8], torch.randn((8,), dtype=torch.float64, device=dev, generator=gen), torch.zeros((8,), dtype=torch.float64, device=dev), torch.zeros_like(r)
dots = window(lambda: L.check(lib.cgamd_projection_dots(ctx.handle, 1, n, n, 8, 255, vp(W), n, vp(r), 1, vp(out))))
comb = window(lambda: L.check(lib.cgamd_projection_combine(ctx.handle, 1, n, n, 8, 255, vp(W), n, vp(r), vp(c), 1, vp(y), 1)))
say({"yardstick": "projection dots, 8 slots", "us": round(statistics.median(dots) * 1e3, 1), "TB_per_s": tbs(9 * n * V, dots)})
say({"yardstick": "projection combine, 8 slots", "us": round(statistics.median(comb) * 1e3, 1), "TB_per_s": tbs(10 * n * V, comb)})
for s in [seed, shifted] + singles:
    s.close()
ctx.close()
