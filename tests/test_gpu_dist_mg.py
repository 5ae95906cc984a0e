"""GPU tests of multigrid PCG on the row-partitioned handle (cgamd_dist_set_preconditioner_multigrid, _amg, cgamd_dist_mg_*;
DistSolver.set_preconditioner / mg_levels / mg_apply).  As in test_gpu_dist_pcg.py the ranks are separate processes that share cuda:0
over the peer-to-peer backend, at most 3 at a time.  The oracle is the serial PCG in complex double whose preconditioner is the
block diagonal of per-rank host hierarchies on the CUT blocks (dist_mg_oracle.py); the bit-level yardstick is a single-GPU Solver
made in the same process on the rank's cut matrix with the same options.

Tolerances are the project's own (test_gpu_dist_pcg.py): history 1e-10 over the entries above 1e-8 of the first and x 1e-9 in fp64 /
complex128; history 1e-4 over the entries above 1e-4 of the first and x 1e-3 in single precision.  The cycle alone is held to
test_gpu_multigrid.check_cycle's bound, which never looks at the code under test.

Launch counts.  An iteration is [SpMV + halo] [all-reduce d.q, alpha] [r -= alpha q, r.r] [the cycle's chain] [r.z] [last step]: the
count of the handle's plain loop, plus the cycle's launches, plus the r.z partials the cycle's output needs (a launch of their own,
as on the single handle, whose multigrid loop is 5 + cycle against 4 for its other preconditioned loops).  The cycle's launches with
one smoothing step and L levels: 1 (the first step on level 0) + 2 per level going down (product, restriction with the coarse
level's first step) + 14 on the coarsest level (7 later steps, a product each) + 3 per level going up = 15 + 5 (L - 1)."""
import functools
import importlib
import os
import socket
import sys
import tempfile
import types

import numpy as np
import pytest

from conftest import PKG_NAME, ROOT

pytestmark = pytest.mark.gpu

DIMS, OPTS = (13, 11, 12), {"min_rows": 16}
ERR_INVALID, ERR_STATE = 1, 7
ITERS = 12


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _tols(dtype):
    """(history, x, history entries compared: above this fraction of the first)"""
    return (1e-10, 1e-9, 1e-8) if np.dtype(dtype) in (np.dtype(np.float64), np.dtype(np.complex128)) else (1e-4, 1e-3, 1e-4)


def _cycle_launches(levels, steps=1):
    assert steps == 1
    return 15 + 5 * (levels - 1)


def _system(kind, dtype):
    """(A as scipy CSR in double / complex double holding the values rounded to dtype, b likewise, global dims or None)"""
    import dist_pcg_oracle as dpo
    import mg_ref
    import test_gpu_multigrid as tgm
    dtype = np.dtype(dtype)
    W = mg_ref.wide(dtype)
    if kind in ("var7", "var7_9", "big"):
        # big: the slab loop applies to its ranks' slabs (test_gpu_dist_pcg.py's 24 x 20 x 36 rows).  The same family as the small
        # system: on the constant-coefficient Laplacian of this size with a smooth right-hand side the ORACLE's own history moves by
        # 2.6e-10 over the compared entries between a cycle in double and one in extended precision, above the 1e-10 it is held
        # to; on this system it moves by 6e-16
        dims = {"var7": DIMS, "var7_9": (13, 11, 9), "big": (24, 20, 36)}[kind]
        A = tgm.system("var7", dims, dtype)
        b = tgm.rhs(dims, dtype, 1)[0]
    elif kind == "grid":            # 385 rows: the row ranges of 3 ranks fall mid-x-line
        dims, A = None, dpo.aniso_grid(11, 7, 5, cz=1.0)
        b = np.linspace(1.0, 2.0, A.shape[0])
    else:
        raise ValueError(kind)
    import scipy.sparse as sp
    A = sp.csr_matrix(A)
    A.sort_indices()
    return sp.csr_matrix(A.astype(dtype).astype(W)), np.asarray(b).astype(dtype).astype(W), dims


def _zeroed(A, world, nx):
    """the diagonal entry of one row of rank 1 zeroed (stored, value 0): (matrix, local row)"""
    import scipy.sparse as sp
    rb, re = A.shape[0] * 1 // world, A.shape[0] * 2 // world
    row = rb + (re - rb) // 3 // nx * nx
    A = sp.csr_matrix(A, copy=True)
    for j in range(A.indptr[row], A.indptr[row + 1]):
        if A.indices[j] == row:
            A.data[j] = 0.0
    return A, row - rb


def _pre(sc, dmod, dims, ranges, rank):
    if sc.get("pre", "multigrid") == "amg":
        return ("amg", dict(sc.get("opts", OPTS)))
    return ("multigrid", dmod.local_grid_dims(dims, ranges, rank), dict(sc.get("opts", OPTS)))


def _worker(rank, world, port, sc, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import torch.distributed as dist
    import dist_mg_oracle as dmo
    import dist_pcg_oracle as dpo
    pkg = importlib.import_module(PKG_NAME)
    dmod = importlib.import_module(PKG_NAME + ".dist")
    lib = pkg._lib.load()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        dev = torch.device("cuda", 0)
        ctx = pkg.Context(0)
        dtype = np.dtype(sc["dtype"])
        A, b, dims = _system(sc["kind"], dtype)
        mode, comm = sc["mode"], sc.get("comm", "p2p")
        if mode == "fail":
            A, bad_local = _zeroed(A, world, dims[0])
        n = A.shape[0]
        ranges = dmod.row_ranges(n, world)
        rb, re = ranges[rank]
        ip_loc, cols_glob, vals_loc = dpo.local_part(A, ranges, rank)
        plan = dmod.build_halo_plan(torch.from_numpy(cols_glob), ranges, rank)
        plan.cols_local = plan.cols_local.to(dev)
        plan.send_index = plan.send_index.to(dev)
        indptr = torch.from_numpy(ip_loc).to(dev)
        vals = torch.from_numpy(vals_loc.astype(dtype)).to(dev)
        bl = torch.from_numpy(b[rb:re].astype(dtype)).to(dev)
        pre = _pre(sc, dmod, dims, ranges, rank)
        if sc.get("flags", 0) & 512:     # slab loop: needs the column codes; the ranks' resident launches share the GPU
            pkg._lib.check(lib.cgamd_tune(b"index_codes_min_mb", 0))
            pkg._lib.check(lib.cgamd_tune(b"dev.resident_lock", 0))

        def make(flags=sc.get("flags", 0), values=vals):
            uid = dmod.broadcast_unique_id(rank) if comm == "rccl" else None
            return dmod.DistSolver(ctx, plan, indptr, values, dtype, unique_id=uid, flags=flags, comm=comm)

        def solve(s, parts):
            s.set_rhs(bl, None)
            for k in parts:
                s.iterate(k)
            x = s.x(torch.empty(plan.n_local, dtype=bl.dtype, device=dev)).cpu().numpy()
            return x, s.history()

        def single_on_cut():
            """the single-GPU handle on this rank's cut matrix (host arrays in the handle's type)"""
            B = dmo.cut_block(A, ranges, rank)
            return pkg.Solver(ctx, B.shape[0], B.nnz, B.data.astype(dtype), B.indptr.astype(np.int32), B.indices.astype(np.int32), 1), B

        out = {}
        s = None
        if mode == "hier":          # the cut matrix, every level and one cycle, beside the single handle on the cut matrix
            s = make()
            s.set_preconditioner(pre)
            ref, B = single_on_cut()
            ref.set_preconditioner(pre)
            lv, lr = s.mg_levels(), ref.mg_levels()
            out["levels"], out["levels_ref"] = len(lv), len(lr)
            out["info"] = np.array([[L[k] for k in ("rows", "nnz", "nx", "ny", "nz")] for L in lv])
            out["info_ref"] = np.array([[L[k] for k in ("rows", "nnz", "nx", "ny", "nz")] for L in lr])
            out["lmax"], out["lmax_ref"] = np.array([L["lmax"] for L in lv]), np.array([L["lmax"] for L in lr])
            for l in range(len(lv)):
                out[f"ip{l}"], out[f"ix{l}"], out[f"da{l}"] = s.mg_level_matrix(l)
            for l in range(len(lr)):
                out[f"rip{l}"], out[f"rix{l}"], out[f"rda{l}"] = ref.mg_level_matrix(l)
            out["z"] = s.mg_apply(bl).cpu().numpy()
            out["z_ref"] = ref.mg_apply(b[rb:re].astype(dtype))
            ref.close()
        elif mode == "parity":      # one handle per flag set, 12 iterations each
            for i, flags in enumerate(sc["flag_sets"]):
                s = make(flags)
                s.set_preconditioner(pre)
                out[f"launches{i}"], out[f"levels{i}"] = s.loop_launches(), len(s.mg_levels())
                out[f"x{i}"], out[f"h{i}"] = solve(s, (ITERS,))
                if i + 1 < len(sc["flag_sets"]):
                    out[f"err{i}"] = s.p2p_error()
                    s.close()
        elif mode == "one_rank":    # against the single-GPU handle on the same matrix with the same preconditioner
            s = make()
            out["launches_plain"] = s.loop_launches()
            s.set_preconditioner(pre)
            out["launches"], out["levels"] = s.loop_launches(), len(s.mg_levels())
            out["x"], out["h"] = solve(s, (ITERS,))
            ref = pkg.Solver(ctx, n, len(vals_loc), vals_loc.astype(dtype), ip_loc, cols_glob.astype(np.int32), 1)
            ref.set_preconditioner(pre)
            out["launches_ref"] = lib.cgamd_solver_loop_launches(ref.handle)
            xr, hr = ref.solve(b.astype(dtype), None, ITERS)
            out["xr"], out["hr"] = xr, hr[:, 0]
            ref.close()
        elif mode == "until":       # iterate_until to tol, then the same count by set_rhs; iterate
            s = make()
            s.set_preconditioner(pre)
            its = s.solve_until(bl, None, tol=sc["tol"], maxit=200, check_every=4)
            out["its"] = its
            out["x"] = s.x(torch.empty(plan.n_local, dtype=bl.dtype, device=dev)).cpu().numpy()
            out["h"] = s.history()
            out["x2"], out["h2"] = solve(s, (its,))
        elif mode == "contracts":
            s = make()
            out["x_fresh"], out["h_fresh"] = solve(s, (ITERS,))
            s.close()
            s = make()
            s.set_preconditioner(pre)
            out["x_mg"], out["h_mg"] = solve(s, (ITERS,))
            out["x_split"], out["h_split"] = solve(s, (5, 7))
            # a refused call (the box is not n_local rows) between two iterate calls: the handle goes on as if it had not been made
            s.set_rhs(bl, None)
            s.iterate(5)
            d3 = pre[1]
            out["bad_status"] = lib.cgamd_dist_set_preconditioner_multigrid(s.handle, d3[0], d3[1], d3[2] + 1, 0, 0.0, 0)
            out["bad_text"] = lib.cgamd_last_error().decode(errors="replace")
            out["levels_after_bad"] = len(s.mg_levels())
            s.iterate(7)
            out["x_bad"] = s.x(torch.empty(plan.n_local, dtype=bl.dtype, device=dev)).cpu().numpy()
            out["h_bad"] = s.history()
            s.set_preconditioner(None)
            out["levels_removed"] = len(s.mg_levels())
            out["x_after"], out["h_after"] = solve(s, (ITERS,))
            # refresh_values after scaling the borrowed values in place, against a fresh handle on the new values
            s.set_preconditioner(pre)
            vals.mul_(1.5)
            torch.cuda.synchronize()
            s.refresh_values()
            out["levels_refreshed"] = len(s.mg_levels())
            out["x_refresh"], out["h_refresh"] = solve(s, (ITERS,))
            s.close()
            s = make()
            s.set_preconditioner(pre)
            out["x_new"], out["h_new"] = solve(s, (ITERS,))
        elif mode == "fail":        # rank 1 fails locally; EVERY rank must raise, name rank 1 and the local row, and keep no preconditioner
            s = make()
            out["launches_plain"] = s.loop_launches()
            try:
                s.set_preconditioner(pre)
                out["msg"] = "no error"
            except pkg._lib.CgAmdError as e:
                out["msg"] = f"{e.status}|{e}"
            out["bad_local"] = bad_local
            out["launches"], out["levels"] = s.loop_launches(), len(s.mg_levels())
            out["x"], out["h"] = solve(s, (ITERS,))
        elif mode == "excluded_sr":  # single-reduction handle: both setters return CGAMD_ERR_STATE
            s = make()
            d3 = pre[1]
            codes, texts = [], []
            for call in (lambda: lib.cgamd_dist_set_preconditioner_multigrid(s.handle, d3[0], d3[1], d3[2], 0, 0.0, 16),
                         lambda: lib.cgamd_dist_set_preconditioner_amg(s.handle, 0, 0.0, 0, 0.0, 16)):
                codes.append(call())
                texts.append(lib.cgamd_last_error().decode(errors="replace"))
            out["codes"], out["texts"] = np.array(codes), np.array(texts)
            out["x"], out["h"] = solve(s, (ITERS,))          # the handle still runs its own loop
        elif mode == "resident":    # slab handle: with the hierarchy set it runs (and reports) a launched loop
            s = make()
            out["launches_before"] = s.loop_launches()
            s.set_preconditioner(pre)
            out["launches_mg"], out["levels"] = s.loop_launches(), len(s.mg_levels())
            out["x"], out["h"] = solve(s, (sc["iters"],))      # one call of >= 16 iterations: what the slab loop would take whole
            s.set_preconditioner(None)
            out["launches_after"] = s.loop_launches()
        else:
            raise ValueError(mode)
        out["err"] = s.p2p_error() if comm == "p2p" else 0
        s.close()
        ctx.close()
        np.savez(os.path.join(out_dir, f"r{rank}.npz"), **out)
        dist.barrier()
    finally:
        dist.destroy_process_group()


def _spawn(out_dir, world, sc):
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(world, _free_port(), sc, str(out_dir)), nprocs=world, join=True)
    parts = [dict(np.load(os.path.join(str(out_dir), f"r{r}.npz"))) for r in range(world)]
    assert all(int(p["err"]) == 0 for p in parts)
    return parts


@functools.lru_cache(maxsize=None)
def _shared(world, mode, kind, dtype, extra=()):
    """one spawn whose results several tests read (left unchanged by all of them)"""
    return _spawn(tempfile.mkdtemp(prefix="dist_mg_"), world, dict(mode=mode, kind=kind, dtype=dtype, **dict(extra)))


@functools.lru_cache(maxsize=None)
def _oracle(kind, dtype, world, pre="multigrid", cut=True, iters=ITERS):
    """(x, history, levels per rank) of the serial oracle, computed once per case"""
    import dist_mg_oracle as dmo
    A, b, dims = _system(kind, dtype)
    ranges = dmo.row_ranges(A.shape[0], world)
    use_dims = dims if pre == "multigrid" else None
    if cut:
        hs = dmo.hierarchies(A, ranges, dtype, use_dims, OPTS)
        solve, levels = dmo.block_solve(hs, ranges), [len(h.levels) for h in hs]
    else:
        solve, levels = dmo.uncut_solve(A, dtype, use_dims, OPTS), None
    x, h = dmo.oracle(A, b, solve, iters)
    return x, h, levels


def _check(parts, key, oracle, dtype, label, iters=ITERS):
    """x / history `key` of all ranks against the serial oracle; returns the kept entries"""
    import dist_mg_oracle as dmo
    ht, xt, floor = _tols(dtype)
    xo, ho = oracle[0], oracle[1]
    for p in parts[1:]:
        assert np.array_equal(p[f"h{key}"].view(np.uint8), parts[0][f"h{key}"].view(np.uint8)), label       # rank-ordered sums: the same bits on all ranks
    h = parts[0][f"h{key}"]
    assert len(h) == iters + 1, (label, len(h))
    keep = np.abs(ho) / np.abs(ho[0]) > floor
    eh = dmo.hist_dev(h, ho, ho, keep)
    x = np.concatenate([p[f"x{key}"] for p in parts])
    ex = float(np.linalg.norm(x - xo) / np.linalg.norm(xo))
    print(f"  {label}: {int(keep.sum())} history entries compared, max rel dev {eh:.3e} (< {ht:g}), x rel err {ex:.3e} (< {xt:g})")
    assert eh < ht, (label, eh)
    assert ex < xt, (label, ex)
    return keep


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# 1. the cut matrix and the hierarchy, bit for bit
@pytest.mark.parametrize("dtype", ["float32", "complex128"])
@pytest.mark.parametrize("world", [2, 3])
def test_cut_matrix_and_hierarchy_bits(world, dtype):
    import dist_mg_oracle as dmo
    parts = _shared(world, "hier", "var7", dtype)
    A, _, dims = _system("var7", dtype)
    ranges = dmo.row_ranges(A.shape[0], world)
    for rank, p in enumerate(parts):
        B = dmo.cut_block(A, ranges, rank)
        ldims = dmo.local_dims(dims, ranges, rank)
        assert int(p["levels"]) == int(p["levels_ref"]) == (4 if world == 2 else 3)
        assert tuple(p["info"][0]) == (B.shape[0], B.nnz) + ldims
        # level 0 is the scipy cut of the rank's block in stored order, exactly
        assert np.array_equal(p["ip0"], B.indptr) and np.array_equal(p["ix0"], B.indices) and _same(p["da0"], B.data.astype(dtype)), (world, rank)
        assert B.nnz < A[ranges[rank][0]:ranges[rank][1]].nnz           # (something was cut)
        # every level has the bits of the single handle on the cut matrix
        assert np.array_equal(p["info"], p["info_ref"])
        assert _same(p["lmax"], p["lmax_ref"]), (p["lmax"], p["lmax_ref"])
        for l in range(int(p["levels"])):
            assert _same(p[f"ip{l}"], p[f"rip{l}"]) and _same(p[f"ix{l}"], p[f"rix{l}"]) and _same(p[f"da{l}"], p[f"rda{l}"]), (world, rank, l)
    if dtype == "float32" and world == 2:
        assert all(int(p["info"][0][0]) % 4 for p in parts)           # 858 rows: not whole 16-byte packs


# 2. the cycle alone
@pytest.mark.parametrize("dtype", ["float32", "float64", "complex64", "complex128"])
def test_cycle_alone(dtype):
    import dist_mg_oracle as dmo
    import mg_ref
    import test_gpu_multigrid as tgm
    world = 2
    parts = _shared(world, "hier", "var7", dtype)
    A, b, dims = _system("var7", dtype)
    ranges = dmo.row_ranges(A.shape[0], world)
    for rank, p in enumerate(parts):
        lo, hi = ranges[rank]
        assert _same(p["z"], p["z_ref"]), (dtype, rank)          # the bits of cgamd_solver_mg_apply on the cut matrix
        H = mg_ref.Hierarchy(dmo.cut_block(A, ranges, rank), dmo.local_dims(dims, ranges, rank), dtype, **OPTS)
        z = p["z"]
        tgm.check_cycle(types.SimpleNamespace(mg_apply=lambda r: z), H, b[lo:hi].astype(dtype).reshape(1, -1), np.dtype(dtype).type,
                        f"rank {rank} of {world}")


# 3. loop parity with the cut oracle.  flags: 0 = four-launch loop, 8 = from a hipGraph, 128 = staged push / unpack / all-reduce launches
FLAG_SETS = (0, 8, 128, 128 | 8)


def _check_launches(parts, key, flags, label):
    for p in parts:
        launches, cycle = int(p[f"launches{key}"]), _cycle_launches(int(p[f"levels{key}"]))
        plain = launches - 1 - cycle
        print(f"  {label}: {launches} launches per iteration = {plain} + 1 + {cycle}")
        assert plain == 7 if flags & 128 else plain in (4, 7), (label, launches, cycle)


@pytest.mark.parametrize("flags", FLAG_SETS)
@pytest.mark.parametrize("world", [2, 3])
def test_parity_fp64(world, flags):
    parts = _shared(world, "parity", "var7", "float64", (("flag_sets", FLAG_SETS),))
    i = FLAG_SETS.index(flags)
    if i + 1 < len(FLAG_SETS):
        assert all(int(p[f"err{i}"]) == 0 for p in parts)
    oracle = _oracle("var7", "float64", world)
    assert [int(p[f"levels{i}"]) for p in parts] == oracle[2]
    _check(parts, i, oracle, np.float64, f"world {world} flags {flags}")
    _check_launches(parts, i, flags, f"world {world} flags {flags}")


@pytest.mark.parametrize("world,dtype,flags", [(2, "float32", 0), (3, "complex64", 0), (2, "complex128", 8)])
def test_parity_other_types(tmp_path, world, dtype, flags):
    parts = _spawn(tmp_path, world, dict(mode="parity", kind="var7", dtype=dtype, flag_sets=(flags,)))
    _check(parts, 0, _oracle("var7", dtype, world), dtype, f"{dtype} world {world} flags {flags}")
    _check_launches(parts, 0, flags, f"{dtype} world {world}")


# 4. the device applies the CUT hierarchy: it matches the cut oracle and is away from the uncut one
def test_sees_the_cut():
    import dist_mg_oracle as dmo
    world = 3
    ht = _tols(np.float64)[0]
    cut, uncut = _oracle("var7", "float64", world), _oracle("var7", "float64", world, cut=False)
    keep = np.abs(cut[1]) / np.abs(cut[1][0]) > 1e-8
    apart = dmo.hist_dev(uncut[1], cut[1], cut[1], keep)
    assert apart >= 100 * ht, apart            # on the CPU first: otherwise this test could not see a wrong cut
    parts = _shared(world, "parity", "var7", "float64", (("flag_sets", FLAG_SETS),))
    _check(parts, 0, cut, np.float64, "cut M")
    wrong = dmo.hist_dev(parts[0]["h0"], uncut[1], cut[1], keep)
    print(f"  the two oracles are {apart:.3e} apart; the device is {wrong:.3e} from the uncut one")
    assert wrong > ht


# 5. one rank, no peers: 13 x 11 x 9 = 1287 rows (not whole packs in fp64) against the single-GPU handle with ("multigrid", dims)
@pytest.mark.parametrize("comm", ["p2p", "rccl"])
def test_one_rank_matches_the_single_gpu_handle(tmp_path, comm):
    p = _spawn(tmp_path, 1, dict(mode="one_rank", kind="var7_9", dtype="float64", comm=comm))[0]
    ht, xt, floor = _tols(np.float64)
    import dist_mg_oracle as dmo
    hr = p["hr"]
    keep = np.abs(hr) / np.abs(hr[0]) > floor
    eh = dmo.hist_dev(p["h"], hr, hr, keep)
    ex = float(np.linalg.norm(p["x"] - p["xr"]) / np.linalg.norm(p["xr"]))
    print(f"  {comm}: history {eh:.3e}, x {ex:.3e}")
    assert eh < ht and ex < xt, (comm, eh, ex)
    _check([p], "", _oracle("var7_9", "float64", 1), np.float64, f"one rank {comm} against the oracle")
    # launches: the plain loop's, the cycle's (the single handle's multigrid loop is 5 + cycle) and the r.z partials
    cycle = int(p["launches_ref"]) - 5
    assert cycle == _cycle_launches(int(p["levels"]))
    print(f"  {comm}: plain loop {int(p['launches_plain'])}, cycle {cycle}, with the hierarchy {int(p['launches'])}")
    assert int(p["launches_plain"]) == (5 if comm == "p2p" else 9)
    assert int(p["launches"]) == int(p["launches_plain"]) + cycle + 1


# 6. the algebraic form on row ranges that fall mid-line
def test_amg_on_a_range_that_falls_mid_line(tmp_path):
    import dist_mg_oracle as dmo
    world = 3
    A, _, _ = _system("grid", "float64")
    ranges = dmo.row_ranges(A.shape[0], world)
    assert all(rb % 11 for rb, _ in ranges[1:])
    parts = _spawn(tmp_path, world, dict(mode="parity", kind="grid", dtype="float64", pre="amg", flag_sets=(0,)))
    oracle = _oracle("grid", "float64", world, pre="amg")
    assert [int(p["levels0"]) for p in parts] == oracle[2] and min(oracle[2]) >= 2
    _check(parts, 0, oracle, np.float64, "amg, cut mid-line")


# 7. iterate_until
def test_iterate_until(tmp_path):
    import dist_mg_oracle as dmo
    world = 2
    A, b, dims = _system("var7", "float64")
    ranges = dmo.row_ranges(A.shape[0], world)
    tol = 1e-6 * float(np.linalg.norm(b))
    _, ho, _ = _oracle("var7", "float64", world, iters=40)
    k_oracle = dmo.first_below(ho, b)
    k_jacobi = dmo.first_below(dmo.oracle(A, b, dmo.jacobi_solve(A), 200)[1], b)
    assert k_oracle is not None and k_jacobi is not None
    parts = _spawn(tmp_path, world, dict(mode="until", kind="var7", dtype="float64", tol=tol))
    its = [int(p["its"]) for p in parts]
    print(f"  stopped after {its} iterations; the serial oracle needs {k_oracle}, Jacobi {k_jacobi}")
    assert len(set(its)) == 1 and abs(its[0] - k_oracle) <= 1 and its[0] < k_jacobi, (its, k_oracle, k_jacobi)
    for p in parts:
        assert len(p["h"]) == its[0] + 1 and np.sqrt(abs(p["h"][-1])) < tol <= np.sqrt(abs(p["h"][-2]))
        assert _same(p["h"], p["h2"]) and _same(p["x"], p["x2"])          # the bits of set_rhs; iterate(its)


# 8. contracts
@pytest.mark.parametrize("flags", [0, 8])
def test_contracts(tmp_path, flags):
    parts = _spawn(tmp_path, 2, dict(mode="contracts", kind="var7", dtype="float64", flags=flags))
    for p in parts:
        assert not _same(p["h_mg"], p["h_fresh"])                              # (the preconditioner was in force)
        assert int(p["levels_removed"]) == 0
        assert _same(p["h_after"], p["h_fresh"]) and _same(p["x_after"], p["x_fresh"])          # removal: a handle that never had any
        assert _same(p["h_split"], p["h_mg"]) and _same(p["x_split"], p["x_mg"])                # iterate(5); iterate(7) = iterate(12)
        assert int(p["bad_status"]) == ERR_INVALID and "nx * ny * nz must equal" in str(p["bad_text"]), p["bad_text"]
        assert int(p["levels_after_bad"]) == 4
        assert _same(p["h_bad"], p["h_mg"]) and _same(p["x_bad"], p["x_mg"])                    # the refused call touched nothing
        assert int(p["levels_refreshed"]) == 4
        assert not _same(p["h_refresh"], p["h_mg"])
        assert _same(p["h_refresh"], p["h_new"]) and _same(p["x_refresh"], p["x_new"])          # refresh_values: a fresh handle on the new values


def test_all_ranks_raise_when_one_fails(tmp_path):
    import dist_mg_oracle as dmo
    world = 3
    parts = _spawn(tmp_path, world, dict(mode="fail", kind="var7", dtype="float64"))
    A, b, dims = _system("var7", "float64")
    A0, bad_local = _zeroed(A, world, dims[0])
    for p in parts:
        assert int(p["bad_local"]) == bad_local
        status, text = str(p["msg"]).split("|", 1)
        assert int(status) == ERR_INVALID, p["msg"]
        assert "rank 1" in text and "dist_set_preconditioner_multigrid" in text and f"row {bad_local}" in text, p["msg"]
        assert int(p["levels"]) == 0 and int(p["launches"]) == int(p["launches_plain"])       # no preconditioner anywhere
    # afterwards the same handles run plain CG (the zeroed diagonal is part of the system)
    xo, ho = dmo.oracle(A0, b, lambda r: r, ITERS)
    _check(parts, "", (xo, ho), np.float64, "plain CG after the failure")


def test_single_reduction_handle_refuses(tmp_path):
    parts = _spawn(tmp_path, 2, dict(mode="excluded_sr", kind="var7", dtype="float64", flags=256))
    for p in parts:
        assert list(p["codes"]) == [ERR_STATE] * 2, p["codes"]
        assert all("single-reduction loop" in str(t) and "no PCG form" in str(t) for t in p["texts"]), p["texts"]
        assert np.all(np.isfinite(p["h"])) and len(p["h"]) == ITERS + 1


def test_resident_handle_runs_its_launched_loop(tmp_path):
    world, iters = 2, 16
    parts = _spawn(tmp_path, world, dict(mode="resident", kind="big", dtype="float64", flags=512, iters=iters))
    print("  launches before / with / after the hierarchy:", [(int(p["launches_before"]), int(p["launches_mg"]), int(p["launches_after"])) for p in parts])
    for p in parts:
        assert int(p["launches_before"]) == 0 and int(p["launches_after"]) == 0       # the slab loop: whole calls in one launch
        assert int(p["launches_mg"]) - 1 - _cycle_launches(int(p["levels"])) in (4, 7)
    _check(parts, "", _oracle("big", "float64", world, iters=iters), np.float64, "slab handle, cut hierarchies", iters=iters)
