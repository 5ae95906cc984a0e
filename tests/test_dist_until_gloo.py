"""CPU tests of the tolerance-stopped row-partitioned recurrences (dist.cg_loop_until / dist.pcg_loop_until, the host mirrors of
cgamd_dist_iterate_until) with world sizes 2 and 3 over gloo, on the 12 x 10 x 18 anisotropic grid in float64: against the serial
oracle stopped by the same rule (oracle/cg_numpy.py cg_tol / pcg_diag), and bit for bit against cg_loop / pcg_loop run for the
stopping iteration.  They also pin the fixture of test_gpu_dist_until.py: with the tolerance chosen by dist_until_fixture.choose_tol
the stopping iteration k* satisfies 8 < k* < 24 and k* % 8 != 0.  Local kernels: the CPU oracle's, as in test_dist_pcg_gloo.py."""
import importlib
import os
import socket
import sys

import numpy as np
import pytest

from conftest import PKG_NAME, ROOT

NX, NY, NZ = 12, 10, 18


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _system():
    import dist_pcg_oracle as dpo
    A = dpo.aniso_grid(NX, NY, NZ)
    return A, np.linspace(1.0, 2.0, A.shape[0])


def _worker(rank, world, port, pre, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import scipy.sparse as sp
    import torch
    import torch.distributed as dist
    import cg_oracle
    import dist_pcg_oracle as dpo
    import dist_until_fixture as fx
    dmod = importlib.import_module(PKG_NAME + ".dist")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        A, b = _system()
        ranges = dmod.row_ranges(A.shape[0], world)
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

        ops, comm = OracleOps(), dmod.TorchComm(plan)
        bl = torch.from_numpy(b[rb:re].astype(A.dtype))
        x0 = torch.zeros_like(bl)
        if pre == "jacobi":     # the rank's own M from its LOCAL matrix, as the C handle builds it
            local = sp.csr_matrix((vals_loc, cols_loc, ip_loc), shape=(plan.n_local, plan.n_local + plan.n_halo))[:, :plan.n_local]
            m = torch.from_numpy(1.0 / local.diagonal())
            fixed = lambda k: dmod.pcg_loop(ops, comm, plan, bl, x0, k, lambda r: m * r)
            until = lambda tol, maxit: dmod.pcg_loop_until(ops, comm, plan, bl, x0, tol, maxit, lambda r: m * r)
        else:
            fixed = lambda k: dmod.cg_loop(ops, comm, plan, bl, x0, k)
            until = lambda tol, maxit: dmod.cg_loop_until(ops, comm, plan, bl, x0, tol, maxit)
        _, H = fixed(fx.MAXIT)
        tol, k_star = fx.choose_tol(H.numpy())
        x, h, its = until(tol, fx.MAXIT)
        xk, hk = fixed(its)
        short = its - 3                         # maxit < its: no stop, its == maxit
        xs, hs, its_s = until(tol, short)
        xsk, hsk = fixed(short)
        bits = lambda t: t.numpy().view(np.uint8)
        np.savez(os.path.join(out_dir, f"r{rank}.npz"), H=H.numpy(), tol=tol, k_star=k_star, x=x.numpy(), h=h.numpy(), its=its,
                 same=np.array_equal(bits(x), bits(xk)) and np.array_equal(bits(h), bits(hk)) and np.array_equal(bits(h), bits(H[:its + 1])),
                 its_short=its_s, short=short, h_short_len=len(hs),
                 same_short=np.array_equal(bits(xs), bits(xsk)) and np.array_equal(bits(hs), bits(hsk)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("pre", [None, "jacobi"])
def test_until_loops_stop_by_the_rule_with_the_bits_of_the_fixed_loops(tmp_path, world, pre):
    import torch.multiprocessing as mp
    import cg_numpy
    import dist_until_fixture as fx
    mp.spawn(_worker, args=(world, _free_port(), pre, str(tmp_path)), nprocs=world, join=True)
    parts = [np.load(os.path.join(str(tmp_path), f"r{r}.npz")) for r in range(world)]
    k_star, tol = int(parts[0]["k_star"]), float(parts[0]["tol"])
    print(f"  world {world} {pre}: tol {tol:.6e}, k* {k_star}")
    # the fixture of the GPU tests: inside the run, behind the first chunk of 8, off every chunk boundary
    assert 8 < k_star < fx.MAXIT and k_star % 8 != 0
    for p in parts:
        assert int(p["its"]) == k_star                          # equal on all ranks, and the index the rule gives on the history
        assert fx.stop_index(p["H"], tol) == k_star
        assert len(p["h"]) == k_star + 1
        assert bool(p["same"])                                  # x and history: the bits of the fixed-count loop run for `its`
        assert int(p["its_short"]) == int(p["short"]) == k_star - 3 and int(p["h_short_len"]) == k_star - 2
        assert bool(p["same_short"])
        assert np.allclose(p["h"], parts[0]["h"], rtol=1e-12)
    # against the serial oracle stopped by the same rule: test_dist_gloo.py's fp64 tolerances (history 1e-10, x 1e-9)
    A, b = _system()
    if pre is None:
        xo, its_o = cg_numpy.cg_tol(A.indptr, A.indices, A.data, b, tol=tol)
        ho = None
    else:
        xo, last, ho = cg_numpy.pcg_diag(A.indptr, A.indices, A.data, b, m=1.0 / A.diagonal(), tol=tol, maxit=fx.MAXIT, history=True)
        its_o = last + 1
    assert its_o == k_star
    x = np.concatenate([p["x"] for p in parts])
    assert np.linalg.norm(x - xo) / np.linalg.norm(xo) < 1e-9
    if ho is not None:
        assert len(ho) == k_star + 1
        assert np.max(np.abs(parts[0]["h"] - ho) / np.abs(ho)) < 1e-10
