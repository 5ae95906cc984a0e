"""cgamd_dist_refresh_values / DistSolver.refresh_values: the ranks' borrowed matrix values change in place on the same pattern.  As in
test_gpu_dist_pcg.py the ranks are separate processes that share cuda:0 over the peer-to-peer backend.  The yardstick is a FRESH
DistSolver built from the new values in the same group under the same keys and flags: history and local x bit for bit (the value
codes are a re-encoding, the rank-ordered sums are the same sums).  Every rank is held to RANK_LIMIT_S from its start; a rank that
is not done by then counts as hung: the ranks are killed and the SESSION ends there, so nothing more is started on that GPU."""
import importlib
import os
import socket
import sys
import time

import numpy as np
import pytest

from conftest import PKG_NAME, ROOT

pytestmark = pytest.mark.gpu

GRID = (12, 10, 18)             # 2 160 rows; two ranks hold 9 z-planes each
GRID_SLAB = (24, 20, 36)        # 17 280 rows: the slab loop applies to the ranks' slabs (as in test_gpu_dist_pcg.py)
ITERS = 30
RANK_LIMIT_S = 120
ERR_INVALID = 1


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _matrix(step, fail=False, grid=GRID):
    """scipy CSR of the 7-point stencil: step 0 diag 6 / off -1; 1: I + 0.375 L; 2: step 1 with ONE entry of row 0 (rank 0) changed;
    fail: step 1 with the diagonal of a row of the last rank zeroed (stored)"""
    import cg_numpy
    import scipy.sparse as sp
    ip, ix, da = cg_numpy.laplace3d(*grid)
    rows = np.repeat(np.arange(len(ip) - 1), np.diff(ip))
    if step >= 1:
        da = np.where(ix == rows, 1.0 + 6 * 0.375, -0.375)
    if step == 2:
        da[1] *= 1.5
    if fail:
        row = len(ip) - 1 - 77
        da[(rows == row) & (ix == row)] = 0.0
    return sp.csr_matrix((da, ix, ip), shape=(len(ip) - 1,) * 2)


def _worker(rank, world, port, sc, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
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
        dtype = np.dtype("float64")
        flags, pre, fail = sc.get("flags", 0), sc.get("pre"), sc.get("fail", False)
        pkg._lib.check(lib.cgamd_tune(b"index_codes_min_mb", 0))       # such small local matrices then build the column and value codes
        if flags & 512:
            pkg._lib.check(lib.cgamd_tune(b"dev.resident_lock", 0))    # the ranks' resident launches share the GPU
        grid = tuple(sc.get("grid", GRID))
        A0 = _matrix(0, grid=grid)
        n = A0.shape[0]
        ranges = dmod.row_ranges(n, world)
        rb, re = ranges[rank]
        ip_loc, cols_glob, v0 = dpo.local_part(A0, ranges, rank)
        plan = dmod.build_halo_plan(torch.from_numpy(cols_glob), ranges, rank)
        plan.cols_local = plan.cols_local.to(dev)
        plan.send_index = plan.send_index.to(dev)
        indptr = torch.from_numpy(ip_loc).to(dev)
        bl = torch.from_numpy(np.linspace(1.0, 2.0, n)[rb:re].astype(dtype)).to(dev)
        steps = [dpo.local_part(_matrix(k, fail, grid), ranges, rank)[2] for k in ((1,) if fail else (1, 2))]

        def make(values):
            return dmod.DistSolver(ctx, plan, indptr, values, dtype, flags=flags, comm="p2p")

        def solve(s):
            s.set_rhs(bl, None)
            s.iterate(ITERS)
            return s.x(torch.empty(plan.n_local, dtype=bl.dtype, device=dev)).cpu().numpy(), s.history()

        out = {}
        # the yardsticks first, one handle at a time: fresh handles on the new values (after a failed refresh: without preconditioner)
        for k, v in enumerate(steps):
            f = make(torch.from_numpy(v.astype(dtype)).to(dev))
            assert f.index_codes() > 0
            if pre is not None and not fail:
                f.set_preconditioner(pre)
            out[f"xf{k}"], out[f"hf{k}"] = solve(f)
            out[f"launches_f{k}"] = f.loop_launches()
            f.close()
        vals = torch.from_numpy(v0.astype(dtype)).to(dev)
        s = make(vals)
        if pre is not None:
            s.set_preconditioner(pre)
        out["last0"] = s.last_refresh
        solve(s)                            # (with CGAMD_DIST_GRAPH: the graph is captured on the old values)
        for k, v in enumerate(steps):
            vals.copy_(torch.from_numpy(v.astype(dtype)))
            torch.cuda.synchronize()
            try:
                s.refresh_values()
                out[f"msg{k}"] = "no error"
            except pkg._lib.CgAmdError as e:
                out[f"msg{k}"] = f"{e.status}|{e}"
            out[f"last{k + 1}"] = s.last_refresh
            out[f"launches{k}"] = s.loop_launches()
            out[f"x{k}"], out[f"h{k}"] = solve(s)
        out["steps"] = len(steps)
        out["err"] = s.p2p_error()
        s.close()
        ctx.close()
        np.savez(os.path.join(out_dir, f"r{rank}.npz"), **out)
        dist.barrier()
    finally:
        dist.destroy_process_group()


def _spawn(tmp_path, world, sc):
    """the ranks as processes of their own, started together, each held to RANK_LIMIT_S from its start.  A rank still alive after that
    is taken for hung: all ranks are killed and the session ends (as the single-GPU file does on a HIP error), nothing is run again"""
    import torch.multiprocessing as mp
    pc = mp.spawn(_worker, args=(world, _free_port(), sc, str(tmp_path)), nprocs=world, join=False)
    deadline = [time.monotonic() + RANK_LIMIT_S] * world            # per rank; the ranks were started at the same time
    while not pc.join(timeout=2):
        late = [r for r, p in enumerate(pc.processes) if p.is_alive() and time.monotonic() > deadline[r]]
        if late:
            for p in pc.processes:
                if p.is_alive():
                    p.kill()
            pytest.exit(f"rank(s) {late} not done after {RANK_LIMIT_S} s: taken for hung, the session ends here", returncode=3)
    parts = [np.load(os.path.join(str(tmp_path), f"r{r}.npz")) for r in range(world)]
    assert all(int(p["err"]) == 0 for p in parts)
    return parts


def _same_bits(parts):
    for r, p in enumerate(parts):
        for k in range(int(p["steps"])):
            assert len(p[f"h{k}"]) == ITERS + 1 and np.all(np.isfinite(p[f"h{k}"]))
            assert np.array_equal(p[f"h{k}"].view(np.uint8), p[f"hf{k}"].view(np.uint8)), f"rank {r} step {k}: history differs from the fresh handle"
            assert np.array_equal(p[f"x{k}"].view(np.uint8), p[f"xf{k}"].view(np.uint8)), f"rank {r} step {k}: x differs from the fresh handle"
            assert int(p[f"launches{k}"]) == int(p[f"launches_f{k}"])
    assert not np.array_equal(parts[0]["h0"], parts[0]["h1"])           # (the perturbed entry is part of the system)


# flags: 0 the four-launch peer-to-peer loop, 8 from a hipGraph, 128 the staged loop, 256 single reduction, 512 the slab loop
@pytest.mark.parametrize("world,flags,pre", [(1, 0, None), (2, 0, None), (2, 8, None), (2, 0, ("line", GRID[0] * GRID[1])), (2, 8, "jacobi"), (2, 128, None),
                                             (2, 256, None), (1, 512, None), (2, 512, None)],
                         ids=["1-rank", "2-ranks", "2-ranks-graph", "2-ranks-line", "2-ranks-graph-jacobi", "2-ranks-staged", "2-ranks-single-reduction",
                              "1-rank-slab", "2-ranks-slab"])
def test_refresh_gives_the_bits_of_a_fresh_handle(tmp_path, world, flags, pre):
    """the rescaled stencil on every rank (dictionaries rewritten in place: outcome 1 everywhere), then one entry changed on rank 0
    (its codes are rebuilt: 2; the other rank's classes are intact: 1)"""
    parts = _spawn(tmp_path, world, dict(flags=flags, pre=pre, grid=GRID_SLAB if flags & 512 else GRID))
    for r, p in enumerate(parts):
        print(f"  rank {r}: last_refresh {int(p['last0'])}, {int(p['last1'])}, {int(p['last2'])}; launches {int(p['launches0'])}; {p['msg0']}, {p['msg1']}")
        assert str(p["msg0"]) == "no error" and str(p["msg1"]) == "no error"
        assert (int(p["last0"]), int(p["last1"]), int(p["last2"])) == (0, 1, 2 if r == 0 else 1)
        assert (int(p["launches0"]) == 0) == bool(flags & 512)         # the slab loop where it was asked for: whole calls in one launch
    _same_bits(parts)


def test_all_ranks_raise_when_one_fails(tmp_path):
    """Jacobi from the matrix, new values with a zero diagonal on the last rank: every rank raises and names that rank and its local row,
    every rank is left without preconditioner -- the bits of fresh plain handles on the new values"""
    world = 2
    parts = _spawn(tmp_path, world, dict(flags=0, pre="jacobi", fail=True))
    n = GRID[0] * GRID[1] * GRID[2]
    bad_local = (n - 77) - n // 2          # _matrix zeroes the diagonal of row n - 77
    for r, p in enumerate(parts):
        status, text = str(p["msg0"]).split("|", 1)
        assert int(status) == ERR_INVALID, p["msg0"]
        assert "rank 1" in text and f"row {bad_local}" in text, text
        assert int(p["last1"]) == (1 if r == 0 else 2)                   # the values are in force (rank 1: the zero split the diagonal's class)
        assert np.array_equal(p["h0"].view(np.uint8), p["hf0"].view(np.uint8)) and np.array_equal(p["x0"].view(np.uint8), p["xf0"].view(np.uint8))
        assert int(p["launches0"]) == int(p["launches_f0"])
