"""CPU tests of the row-partitioned PCG recurrence (dist.pcg_loop, the torch statement of what csrc/dist.cpp runs with a
preconditioner) with world sizes 2 and 3 over gloo.  The preconditioner is rank-local: a diagonal, or line solves cut at the rank's
row range.  The oracle is the serial PCG in double / complex double with the SAME preconditioner assembled globally as the
block-diagonal of the per-rank M (dist_pcg_oracle.global_m).  Local kernels: the CPU oracle's, as in test_dist_gloo.py."""
import importlib
import os
import socket
import sys

import numpy as np
import pytest

from conftest import PKG_NAME, ROOT


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


NX, NY, NZ = 12, 10, 9


def _system(kind):
    import dist_pcg_oracle as dpo
    if kind == "aniso":           # 12 x 10 x 9, 100x z-coupling, fp64
        A = dpo.aniso_grid(NX, NY, NZ)
        return A, np.linspace(1.0, 2.0, A.shape[0])
    A, b = dpo.helm(20)           # complex128
    return A, b


def _worker(rank, world, port, kind, pre, iters, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    import torch
    import torch.distributed as dist
    import cg_oracle
    import dist_pcg_oracle as dpo
    dmod = importlib.import_module(PKG_NAME + ".dist")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        A, b = _system(kind)
        n = A.shape[0]
        ranges = dmod.row_ranges(n, world)
        rb, re = ranges[rank]
        ip_loc, cols_glob, vals_loc = dpo.local_part(A, ranges, rank)
        plan = dmod.build_halo_plan(torch.from_numpy(cols_glob), ranges, rank)
        cols_loc = plan.cols_local.numpy()

        class OracleOps:
            def spmv(self, v_ext):
                ptr_ext = np.concatenate([ip_loc, np.full(plan.n_halo, ip_loc[-1], dtype=np.int32)])
                y = cg_oracle.spmv(ptr_ext, cols_loc, vals_loc, v_ext.numpy(), mode=cg_oracle.MODE_SEQUENTIAL)
                return torch.from_numpy(y[:plan.n_local])

            def dot(self, a, c):
                return torch.from_numpy(cg_oracle.vdot(a.numpy().copy(), c.numpy().copy(), mode=cg_oracle.MODE_SEQUENTIAL))[0]

        comm = dmod.TorchComm(plan)
        bl = torch.from_numpy(b[rb:re].astype(A.dtype))
        x0 = torch.zeros_like(bl)
        if pre == "identity":       # the plain recurrence, bit for bit
            class RankOrderComm(dmod.TorchComm):
                """sums in rank order, element by element, as the device's peer-to-peer backend does: a library all-reduce may
                add the elements of a two-value message in another rank order than those of a one-value message (ring chunks),
                which says nothing about the two loops compared here"""
                def allreduce(self, t):
                    parts = [torch.empty_like(t) for _ in range(world)]
                    dist.all_gather(parts, t.contiguous())
                    acc = parts[0].clone()
                    for p in parts[1:]:
                        acc = acc + p
                    t.copy_(acc)
                    return t
            comm = RankOrderComm(plan)
            x, hist = dmod.pcg_loop(OracleOps(), comm, plan, bl, x0, iters, lambda r: r)
            xc, hc = dmod.cg_loop(OracleOps(), comm, plan, bl, x0, iters)
            assert np.array_equal(x.numpy().view(np.uint8), xc.numpy().view(np.uint8))
            assert np.array_equal(hist.numpy().view(np.uint8), hc.numpy().view(np.uint8))
        else:
            # the rank's own M from its LOCAL matrix, as the C handle builds it: columns below n_local only
            local = sp.csr_matrix((vals_loc, cols_loc, ip_loc), shape=(plan.n_local, plan.n_local + plan.n_halo))[:, :plan.n_local]
            if pre == "jacobi":
                m = torch.from_numpy(1.0 / local.diagonal())
                apply_m = lambda r: m * r
            else:
                Ml = dpo.global_m(local, [(0, plan.n_local)], pre)
                lu = spla.splu(sp.csc_matrix(Ml))
                apply_m = lambda r: torch.from_numpy(lu.solve(r.numpy()))
            x, hist = dmod.pcg_loop(OracleOps(), comm, plan, bl, x0, iters, apply_m)
        np.savez(os.path.join(out_dir, f"r{rank}.npz"), x=x.numpy(), hist=hist.numpy())
    finally:
        dist.destroy_process_group()


def _run(tmp_path, world, kind, pre, iters):
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(world, _free_port(), kind, pre, iters, str(tmp_path)), nprocs=world, join=True)
    parts = [np.load(os.path.join(str(tmp_path), f"r{r}.npz")) for r in range(world)]
    return np.concatenate([p["x"] for p in parts]), [p["hist"] for p in parts]


# x-lines (stride 1) and y-lines (stride nx) lie inside a z-slab; z-lines (stride nx ny) are cut at the rank boundaries
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("kind,pre", [("aniso", "jacobi"), ("aniso", ("line", 1)), ("aniso", ("line", NX * NY)), ("helm", "jacobi")])
def test_pcg_loop_matches_serial_oracle(tmp_path, world, kind, pre):
    import dist_pcg_oracle as dpo
    iters = 12
    x, hists = _run(tmp_path, world, kind, pre, iters)
    A, b = _system(kind)
    ranges = dpo.row_ranges(A.shape[0], world)
    M = dpo.global_m(A, ranges, pre)
    if pre == ("line", NX * NY):       # the z-lines are really cut: the block-diagonal M differs from the uncut one
        assert (dpo.global_m(A, ranges, pre, cut=False) - M).nnz == 2 * NX * NY * (world - 1)
    xo, ho = dpo.oracle(A, b, M, iters)
    for h in hists[1:]:
        assert np.allclose(h, hists[0], rtol=1e-12)
    # test_dist_gloo.py's fp64 tolerances (history 1e-10, x 1e-9), the history while it is above reduction-order noise (1e-8 of
    # its first entry, as test_gpu_tridiag.py does for a recurrence that converges within the run)
    keep = np.abs(ho) / np.abs(ho[0]) > 1e-8
    assert keep.sum() >= 4
    assert np.max(np.abs(hists[0][keep] - ho[keep]) / np.abs(ho[keep])) < 1e-10
    assert np.linalg.norm(x - xo) / np.linalg.norm(xo) < 1e-9


@pytest.mark.parametrize("world,kind", [(2, "aniso"), (3, "helm")])
def test_pcg_loop_with_identity_is_cg_loop_bit_for_bit(tmp_path, world, kind):
    _run(tmp_path, world, kind, "identity", 8)       # asserted inside every worker
