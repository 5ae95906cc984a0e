"""GPU test of replacing one preconditioner by another on a live handle -- single, batched and row-partitioned.

The system is the variable-coefficient 7-point matrix on 12 x 10 x 8 (960 rows): the smallest 3-D system the grid multigrid coarsens
at least once with min_rows lowered (the level count is read back and must exceed 1).  The states are none, a diagonal from the
caller, Jacobi from the matrix, the lines at stride 1 and 12, grid multigrid and AMG (the batched handle has no AMG entry).  ONE
handle walks a closed path through every ordered pair (A, B) of states, A = B included: at each state it runs set_rhs; iterate(12),
which is compared, then set_rhs; iterate(3), then the next state is installed.  So for every pair: A stood, set_rhs, iterate(3),
install B, set_rhs, iterate(12).  After every install iterate must be refused with CGAMD_ERR_STATE until set_rhs, and the 12
iterations must be those of a fresh handle that only ever had B: x and history bit for bit, preconditioner source, multigrid levels
and launches per iteration equal.  The fresh handles are made once per state and shared.

One more case per handle type: an install that fails (a box that does not hold the rows) after A stood leaves A in force -- the next
solve is bit-equal to the handle with A alone.  The row-partitioned handle runs in two processes of 480 rows each over the
peer-to-peer backend, as test_gpu_dist_mg.py sets them up."""
import functools
import importlib
import os
import socket
import sys
import tempfile

import numpy as np
import pytest

from conftest import PKG_NAME, ROOT
from spmv_ref import bit_equal

pytestmark = pytest.mark.gpu

DIMS = (12, 10, 8)
N = 960
MG_OPTS = {"min_rows": 64}
ERR_INVALID, ERR_STATE = 1, 7
STATES = ("none", "diag", "jacobi", "line1", "line12", "multigrid", "amg")


def closed_walk(k):
    """nodes of a closed walk over every ordered pair of range(k), loops included (Hierholzer on the complete digraph)"""
    unused = {a: list(range(k)) for a in range(k)}
    stack, walk = [0], []
    while stack:
        a = stack[-1]
        if unused[a]:
            stack.append(unused[a].pop())
        else:
            walk.append(stack.pop())
    walk.reverse()
    assert len(walk) == k * k + 1 and len(set(zip(walk, walk[1:]))) == k * k
    return walk


def system(dtype):
    import test_gpu_multigrid as tgm
    A = tgm.system("var7", DIMS, dtype).tocsr()
    A.sort_indices()
    assert A.shape == (N, N)
    return A


def caller_diagonal(A, dtype):
    """not Jacobi's: 1 / diag(A) scaled row by row"""
    return ((1.0 + 0.25 * np.cos(np.arange(A.shape[0]))) / A.diagonal()).astype(dtype)


def spec(state, dims=DIMS):
    return {"none": None, "jacobi": "jacobi", "line1": ("line", 1), "line12": ("line", 12), "multigrid": ("multigrid", dims, dict(MG_OPTS)),
            "amg": ("amg", dict(MG_OPTS))}[state]


# ---- single and batched handles -----------------------------------------------------------------------------------------------------
def make_handle(pkg, ctx, A, dtype, nrhs, batched):
    da = A.data.astype(dtype)
    if batched:     # system r: the values scaled and perturbed entry by entry, symmetric
        sym = 1.0 + 0.1 * np.cos(np.minimum(A.tocoo().row, A.tocoo().col) + 3.0 * np.maximum(A.tocoo().row, A.tocoo().col))
        da = np.concatenate([A.data, 1.5 * A.data * sym]).astype(dtype)
    return pkg.Solver(ctx, N, A.nnz, da, A.indptr.astype(np.int32), A.indices.astype(np.int32), nrhs, batched=batched)


def install(s, state, A, dtype, batched):
    if state == "diag":
        m = caller_diagonal(A, dtype)
        s.set_preconditioner(np.concatenate([m, 0.5 * m]) if batched else m)
    else:
        s.set_preconditioner(spec(state))


def observe(pkg, s, b, iters):
    lib = pkg._lib.load()
    s.set_rhs(b, None)
    s.iterate(iters)
    return {"x": s.x().copy(), "h": s.history().copy(), "source": s.preconditioner_source, "levels": len(s.mg_levels()),
            "launches": lib.cgamd_solver_loop_launches(s.handle)}


def same(got, want, label):
    assert bit_equal(got["x"], want["x"]), label
    assert bit_equal(got["h"], want["h"]), label
    assert (got["source"], got["levels"], got["launches"]) == (want["source"], want["levels"], want["launches"]), label


def walk_every_ordered_pair(pkg, gpu, dtype, nrhs, batched):
    ctx = gpu[0]
    lib = pkg._lib.load()
    A = system(dtype)
    import test_gpu_multigrid as tgm
    b = tgm.rhs(DIMS, dtype, nrhs).reshape(-1)
    states = [st for st in STATES if not (batched and st == "amg")]
    fresh = {}
    for st in states:
        s = make_handle(pkg, ctx, A, dtype, nrhs, batched)
        install(s, st, A, dtype, batched)
        fresh[st] = observe(pkg, s, b, 12)
        s.close()
    assert fresh["multigrid"]["levels"] > 1 and fresh["none"]["levels"] == 0
    assert fresh["none"]["source"] == 0 and fresh["diag"]["source"] == 1 and all(fresh[st]["source"] in (2, 3) for st in states[2:])
    assert not bit_equal(fresh["diag"]["x"], fresh["jacobi"]["x"]) and not bit_equal(fresh["line1"]["x"], fresh["line12"]["x"])
    s = make_handle(pkg, ctx, A, dtype, nrhs, batched)
    walk = [states[i] for i in closed_walk(len(states))]
    prev = "(new)"
    for st in walk:
        if prev != "(new)":
            s.set_rhs(b, None)
            s.iterate(3)
        install(s, st, A, dtype, batched)
        if not (batched and prev == st == "none"):      # (removing nothing from a batched handle is no call at all: nothing to refuse)
            assert lib.cgamd_solver_iterate(s.handle, 1) == ERR_STATE, (prev, st)
        same(observe(pkg, s, b, 12), fresh[st], f"{prev} -> {st}")
        prev = st
    s.close()


@pytest.mark.parametrize("nrhs", [1, 3])
@pytest.mark.parametrize("dtype", [np.float64, np.complex64])
def test_every_ordered_pair_on_one_handle(pkg, gpu, dtype, nrhs):
    walk_every_ordered_pair(pkg, gpu, dtype, nrhs, False)


@pytest.mark.parametrize("dtype", [np.float64, np.complex64])
def test_every_ordered_pair_on_a_batched_handle(pkg, gpu, dtype):
    walk_every_ordered_pair(pkg, gpu, dtype, 2, True)


@pytest.mark.parametrize("batched", [False, True], ids=["single", "batched"])
@pytest.mark.parametrize("first", ["jacobi", "line12", "multigrid"])
def test_a_failed_install_leaves_the_first_in_force(pkg, gpu, first, batched):
    ctx = gpu[0]
    lib = pkg._lib.load()
    dtype, nrhs = np.float64, 2
    A = system(dtype)
    import test_gpu_multigrid as tgm
    b = tgm.rhs(DIMS, dtype, nrhs).reshape(-1)
    s = make_handle(pkg, ctx, A, dtype, nrhs, batched)
    install(s, first, A, dtype, batched)
    want = observe(pkg, s, b, 12)
    s.set_rhs(b, None)
    s.iterate(3)
    entry = lib.cgamd_solver_set_preconditioner_batched_multigrid if batched else lib.cgamd_solver_set_preconditioner_multigrid
    assert entry(s.handle, DIMS[0], DIMS[1], DIMS[2] + 1, 0, 0.0, 64) == ERR_INVALID
    assert b"nx * ny * nz must equal the size of the system" in lib.cgamd_last_error()
    s.iterate(2)        # nothing on the handle changed: the right-hand side is still set
    same(observe(pkg, s, b, 12), want, first)
    s.close()


# ---- the row-partitioned handle: two ranks -----------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import torch
    import torch.distributed as dist
    import dist_pcg_oracle as dpo
    pkg = importlib.import_module(PKG_NAME)
    dmod = importlib.import_module(PKG_NAME + ".dist")
    lib = pkg._lib.load()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        dev = torch.device("cuda", 0)
        ctx = pkg.Context(0)
        out = {"err": 0}
        for dtype in (np.dtype(np.float64), np.dtype(np.complex64)):
            tag = dtype.name
            A = system(dtype)
            import test_gpu_multigrid as tgm
            b = tgm.rhs(DIMS, dtype, 1)[0]
            ranges = dmod.row_ranges(N, world)
            rb, re = ranges[rank]
            assert re - rb == N // world
            ip_loc, cols_glob, vals_loc = dpo.local_part(A, ranges, rank)
            plan = dmod.build_halo_plan(torch.from_numpy(cols_glob), ranges, rank)
            plan.cols_local = plan.cols_local.to(dev)
            plan.send_index = plan.send_index.to(dev)
            indptr = torch.from_numpy(ip_loc).to(dev)
            vals = torch.from_numpy(vals_loc.astype(dtype)).to(dev)
            bl = torch.from_numpy(b[rb:re].astype(dtype)).to(dev)
            mdiag = torch.from_numpy(caller_diagonal(A, dtype)[rb:re]).to(dev)
            local_dims = dmod.local_grid_dims(DIMS, ranges, rank)

            def make():
                return dmod.DistSolver(ctx, plan, indptr, vals, dtype, unique_id=None, flags=0, comm="p2p")

            def install(s, st):
                s.set_preconditioner(mdiag if st == "diag" else spec(st, local_dims))

            def observe(s, iters=12):
                s.set_rhs(bl, None)
                s.iterate(iters)
                x = s.x(torch.empty(plan.n_local, dtype=bl.dtype, device=dev)).cpu().numpy()
                return x, s.history(), np.array([len(s.mg_levels()), s.loop_launches()])

            def close(s):
                out["err"] += int(s.p2p_error())
                s.close()

            fresh = {}
            for st in STATES:
                s = make()
                install(s, st)
                fresh[st] = observe(s)
                out[f"{tag}_fresh_levels_{st}"] = fresh[st][2][0]
                close(s)
            s = make()
            walk = [STATES[i] for i in closed_walk(len(STATES))]
            bad, prev = [], None
            for st in walk:
                if prev is not None:
                    s.set_rhs(bl, None)
                    s.iterate(3)
                install(s, st)
                refused = lib.cgamd_dist_iterate(s.handle, 1)
                x, h, info = observe(s)
                fx, fh, finfo = fresh[st]
                if not (refused == ERR_STATE and bit_equal(x, fx) and bit_equal(h, fh) and np.array_equal(info, finfo)):
                    bad.append(f"{prev} -> {st}")
                prev = st
            out[f"{tag}_pairs"] = len(walk) - 1
            out[f"{tag}_bad"] = np.array(bad if bad else [""])
            # a failed install after A stood (every rank refuses: the box holds one plane too many), then A's own solve again
            for st in ("jacobi", "line12", "multigrid"):
                install(s, st)
                s.set_rhs(bl, None)
                s.iterate(3)
                status = lib.cgamd_dist_set_preconditioner_multigrid(s.handle, local_dims[0], local_dims[1], local_dims[2] + 1, 0, 0.0, 64)
                text = lib.cgamd_last_error().decode(errors="replace")
                s.iterate(2)
                x, h, info = observe(s)
                fx, fh, finfo = fresh[st]
                out[f"{tag}_failed_{st}"] = int(status == ERR_INVALID and "the rank's own box" in text and bit_equal(x, fx) and bit_equal(h, fh)
                                              and np.array_equal(info, finfo))
            close(s)
        ctx.close()
        np.savez(os.path.join(out_dir, f"r{rank}.npz"), **out)
        dist.barrier()
    finally:
        dist.destroy_process_group()


@functools.lru_cache(maxsize=None)
def two_ranks():
    import torch.multiprocessing as mp
    out_dir = tempfile.mkdtemp(prefix="precond_succession_")
    mp.spawn(_worker, args=(2, _free_port(), out_dir), nprocs=2, join=True)
    return [dict(np.load(os.path.join(out_dir, f"r{r}.npz"))) for r in range(2)]


@pytest.mark.parametrize("dtype", ["float64", "complex64"])
def test_every_ordered_pair_on_two_ranks(dtype):
    for part in two_ranks():
        assert int(part["err"]) == 0
        assert int(part[f"{dtype}_pairs"]) == len(STATES) ** 2
        assert int(part[f"{dtype}_fresh_levels_multigrid"]) > 1 and int(part[f"{dtype}_fresh_levels_amg"]) > 1
        assert list(part[f"{dtype}_bad"]) == [""], list(part[f"{dtype}_bad"])


@pytest.mark.parametrize("dtype", ["float64", "complex64"])
def test_a_failed_install_leaves_the_first_in_force_on_two_ranks(dtype):
    for part in two_ranks():
        for st in ("jacobi", "line12", "multigrid"):
            assert int(part[f"{dtype}_failed_{st}"]) == 1, st
