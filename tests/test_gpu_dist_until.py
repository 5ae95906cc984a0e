"""GPU tests of the tolerance stop on the device for the row-partitioned handle (cgamd_dist_iterate_until, DistSolver.iterate_until /
solve_until).  As in test_gpu_dist_pcg.py the ranks are separate processes that share cuda:0; ONE spawn per world size runs all of
that world's scenarios (a scenario = one handle: loop form, preconditioner, type), and the tests below read what it left.

Per scenario, on one handle: the fixed-count run of 24 iterations gives the reference history H; the tolerance is chosen from H
(dist_until_fixture.choose_tol, pinned on the CPU by test_dist_until_gloo.py) so that the rule stops at a known k*, 8 < k* < 24,
off every chunk boundary; then every way of getting there -- solve_until with check_every 8, 1, 5, 64, two until calls, iterate
followed by until -- must return k* on every rank and leave the bits of set_rhs; iterate(k*): x, and the history rows 0..k*.

Tolerances against the serial oracle are test_gpu_dist_p2p.py's: history 1e-10 (fp64) / 1e-4 (single), x 1e-9 / 1e-3."""
import importlib
import os
import socket
import sys
import time

import numpy as np
import pytest

from conftest import PKG_NAME, ROOT

pytestmark = pytest.mark.gpu

NX, NY, NZ = 12, 10, 18
ERR_STATE = 7
GRAPH, NO_OVERLAP, STAGED, SINGLE_REDUCTION, RESIDENT = 8, 32, 128, 256, 512
CHECK_EVERY = (1, 5, 8, 64)     # 64 > 24: one chunk
WORKER_TIMEOUT = 300            # seconds for one world's ranks, all scenarios (they take a fraction of it)


def _scenarios(world):
    """one handle each; `oracle`: compared against the serial oracle too (M assembled globally)"""
    if world == 1:
        return [dict(name="rccl", kind="aniso", dtype="float64", comm="rccl", flags=0, pre=None, oracle=True),
                dict(name="rccl jacobi", kind="aniso", dtype="float64", comm="rccl", flags=0, pre="jacobi", oracle=True),
                dict(name="rccl graph", kind="aniso", dtype="float64", comm="rccl", flags=GRAPH, pre=None),
                dict(name="rccl complex64", kind="helm", dtype="complex64", comm="rccl", flags=0, pre=None, oracle=True)]
    return [dict(name="p2p4", kind="aniso", dtype="float64", flags=0, pre=None, oracle=True),
            dict(name="p2p4 jacobi", kind="aniso", dtype="float64", flags=0, pre="jacobi", oracle=True),
            dict(name="p2p4 x-lines", kind="aniso", dtype="float64", flags=0, pre=("line", 1)),
            dict(name="p2p4 cut z-lines", kind="aniso", dtype="float64", flags=0, pre=("line", NX * NY), oracle=True),
            dict(name="staged", kind="aniso", dtype="float64", flags=STAGED, pre=None),
            dict(name="staged jacobi", kind="aniso", dtype="float64", flags=STAGED, pre="jacobi"),
            dict(name="staged no overlap", kind="aniso", dtype="float64", flags=STAGED | NO_OVERLAP, pre=None),
            dict(name="staged, overlapped exchange", kind="aniso_big", dtype="float64", flags=STAGED, pre=None),
            dict(name="p2p4 complex64", kind="helm", dtype="complex64", flags=0, pre=None, oracle=True),
            dict(name="p2p4 complex64 jacobi", kind="helm", dtype="complex64", flags=0, pre="jacobi"),
            dict(name="staged complex64", kind="helm", dtype="complex64", flags=STAGED, pre=None),
            # (last: its tuning keys are the process's from here on) a slab handle runs its launched loop in iterate_until, as it does
            # while a preconditioner is set -- set here, so that the fixed-count reference runs the same loop
            dict(name="resident", kind="aniso_big", dtype="float64", flags=RESIDENT, pre=("line", 24 * 20))]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _system(kind):
    import dist_pcg_oracle as dpo
    if kind == "aniso":
        A = dpo.aniso_grid(NX, NY, NZ)
    elif kind == "aniso_big":
        A = dpo.aniso_grid(24, 20, 36)
    elif kind == "helm":
        return dpo.helm(60)
    else:
        raise ValueError(kind)
    return A, np.linspace(1.0, 2.0, A.shape[0])


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import torch.distributed as dist
    import dist_pcg_oracle as dpo
    import dist_until_fixture as fx
    pkg = importlib.import_module(PKG_NAME)
    dmod = importlib.import_module(PKG_NAME + ".dist")
    lib = pkg._lib.load()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        dev = torch.device("cuda", 0)
        ctx = pkg.Context(0)
        out = {}
        bits = lambda a: np.ascontiguousarray(a).view(np.uint8)
        same = lambda a, b: bool(a.shape == b.shape and np.array_equal(bits(a), bits(b)))

        def build(sc, flags=None):
            A, b = _system(sc["kind"])
            dtype = np.dtype(sc["dtype"])
            ranges = dmod.row_ranges(A.shape[0], world)
            rb, re = ranges[rank]
            ip_loc, cols_glob, vals_loc = dpo.local_part(A, ranges, rank)
            plan = dmod.build_halo_plan(torch.from_numpy(cols_glob), ranges, rank)
            plan.cols_local = plan.cols_local.to(dev)
            plan.send_index = plan.send_index.to(dev)
            indptr = torch.from_numpy(ip_loc).to(dev)
            vals = torch.from_numpy(vals_loc.astype(dtype)).to(dev)
            b_host = b[rb:re].astype(dtype)
            comm = sc.get("comm", "p2p")
            uid = dmod.broadcast_unique_id(rank) if comm == "rccl" else None
            s = dmod.DistSolver(ctx, plan, indptr, vals, dtype, unique_id=uid, flags=sc["flags"] if flags is None else flags, comm=comm)
            return s, plan, b_host

        def get_x(s, plan, bl):
            return s.x(torch.empty(plan.n_local, dtype=bl.dtype, device=dev)).cpu().numpy()

        def p2p_err(s, sc):
            return int(s.p2p_error()) if sc.get("comm", "p2p") == "p2p" else 0

        for i, sc in enumerate(_scenarios(world)):
            k = f"s{i}_"
            if sc["flags"] & RESIDENT:      # slab loop: needs the column codes; the ranks' resident launches share the GPU
                pkg._lib.check(lib.cgamd_tune(b"index_codes_min_mb", 0))
                pkg._lib.check(lib.cgamd_tune(b"dev.resident_lock", 0))
            s, plan, b_host = build(sc)
            bl = torch.from_numpy(b_host).to(dev)
            torch.cuda.synchronize()
            if sc["pre"] is not None:
                s.set_preconditioner(sc["pre"])
            out[k + "launches"] = s.loop_launches()
            # 1. the fixed-count reference
            s.set_rhs(bl, None)
            s.iterate(fx.MAXIT)
            H = s.history()
            out[k + "H"], out[k + "x24"] = H, get_x(s, plan, bl)
            # 2. the tolerance and the iteration the rule stops in
            tol, k_star = fx.choose_tol(H)
            out[k + "tol"], out[k + "k_star"] = tol, k_star
            s.set_rhs(bl, None)
            s.iterate(k_star)
            x_ref = get_x(s, plan, bl)
            out[k + "h_ref_ok"] = same(s.history(), H[:k_star + 1])
            # 3. solve_until
            its = s.solve_until(bl, None, tol, fx.MAXIT)
            x, h = get_x(s, plan, bl), s.history()
            out[k + "its"], out[k + "x"], out[k + "h"], out[k + "done"] = its, x, h, s.iterations_done
            out[k + "x_ok"], out[k + "h_ok"] = same(x, x_ref), same(h, H[:k_star + 1])
            out[k + "its_again"] = s.iterate_until(tol * 1e-3, fx.MAXIT)        # a stopped handle returns at once, whatever the tolerance
            out[k + "x_again_ok"] = same(get_x(s, plan, bl), x_ref)
            try:
                s.iterate(1)
                out[k + "iterate_status"] = 0
            except pkg._lib.CgAmdError as e:
                out[k + "iterate_status"] = e.status
            out[k + "x_after_refusal_ok"] = same(get_x(s, plan, bl), x_ref)
            s.set_rhs(bl, None)
            s.iterate(2)                                                        # after set_rhs the handle iterates again
            out[k + "h_after_set_rhs_ok"] = same(s.history(), H[:3])
            # 4. the same bits whatever the chunk length
            oks = []
            for ce in CHECK_EVERY:
                got = s.solve_until(bl, None, tol, fx.MAXIT, check_every=ce)
                oks.append(got == k_star and same(get_x(s, plan, bl), x_ref) and same(s.history(), H[:k_star + 1]) and s.iterations_done == k_star)
            out[k + "check_every_ok"] = np.array(oks)
            # 5. until(5); until(19)
            s.set_rhs(bl, None)
            first = s.iterate_until(tol, 5)
            h5_ok = same(s.history(), H[:6])
            second = s.iterate_until(tol, fx.MAXIT - 5)
            out[k + "two_calls"] = np.array([first, second])
            out[k + "two_calls_ok"] = h5_ok and same(get_x(s, plan, bl), x_ref) and same(s.history(), H[:k_star + 1])
            # 6. iterate(3); until
            s.set_rhs(bl, None)
            s.iterate(3)
            out[k + "after_iterate"] = s.iterate_until(tol, fx.MAXIT - 3)
            out[k + "after_iterate_ok"] = same(get_x(s, plan, bl), x_ref) and same(s.history(), H[:k_star + 1])
            out[k + "err"] = p2p_err(s, sc)
            if i == 0:
                # 7. one NaN entry in b on one rank: every rank stops at iteration 1, nobody times out
                b_nan = b_host.copy()
                if rank == min(1, world - 1):
                    b_nan[len(b_nan) // 2] = np.nan
                bn = torch.from_numpy(b_nan).to(dev)
                torch.cuda.synchronize()
                out["nan_its"] = s.solve_until(bn, None, tol, fx.MAXIT)
                out["nan_h"] = s.history()
                out["nan_err"] = p2p_err(s, sc)
                # unchanged behaviour: a handle that never calls iterate_until
                s0, plan0, _ = build(sc)
                s0.set_rhs(bl, None)
                s0.iterate(fx.MAXIT)
                out["plain_ok"] = same(s0.history(), H) and same(get_x(s0, plan0, bl), out[k + "x24"])
                out["plain_err"] = p2p_err(s0, sc)
                s0.close()
                if world == 2:
                    # 8. the single-reduction loop has no guarded form: CGAMD_ERR_STATE, and the handle still iterates
                    s1, plan1, _ = build(sc, flags=SINGLE_REDUCTION)
                    s1.set_rhs(bl, None)
                    its1 = __import__("ctypes").c_int(-1)
                    out["sr_status"] = lib.cgamd_dist_iterate_until(s1.handle, fx.MAXIT, tol, 8, __import__("ctypes").byref(its1))
                    out["sr_text"] = np.array(lib.cgamd_last_error().decode(errors="replace"))
                    s1.iterate(12)
                    out["sr_h"] = s1.history()
                    out["sr_err"] = p2p_err(s1, sc)
                    s1.close()
            s.close()
        ctx.close()
        np.savez(os.path.join(out_dir, f"r{rank}.npz"), **out)
        dist.barrier()
    finally:
        dist.destroy_process_group()


_RESULTS = {}


def _results(world, tmp_path_factory):
    """the ranks of one world, run once for all its scenarios, under a time limit of their own"""
    if world not in _RESULTS:
        import torch.multiprocessing as mp
        out_dir = str(tmp_path_factory.mktemp(f"dist_until_w{world}"))
        ctx = mp.spawn(_worker, args=(world, _free_port(), out_dir), nprocs=world, join=False)
        deadline = time.monotonic() + WORKER_TIMEOUT
        try:
            while not ctx.join(timeout=2.0):
                if time.monotonic() > deadline:
                    raise AssertionError(f"the ranks of world {world} ran past {WORKER_TIMEOUT} s")
        finally:
            for p in ctx.processes:
                if p.is_alive():
                    p.kill()
        _RESULTS[world] = [np.load(os.path.join(out_dir, f"r{r}.npz")) for r in range(world)]
    return _RESULTS[world]


CASES = [(w, i) for w in (1, 2, 3) for i in range(len(_scenarios(w)))]
IDS = [f"w{w}-{_scenarios(w)[i]['name'].replace(' ', '_')}" for w, i in CASES]


@pytest.mark.parametrize("world,i", CASES, ids=IDS)
def test_stop_leaves_the_bits_of_the_fixed_count_run(tmp_path_factory, world, i):
    import dist_until_fixture as fx
    parts = _results(world, tmp_path_factory)
    sc, k = _scenarios(world)[i], f"s{i}_"
    k_star, tol = int(parts[0][k + "k_star"]), float(parts[0][k + "tol"])
    print(f"  world {world} {sc['name']}: launches {[int(p[k + 'launches']) for p in parts]}, tol {tol:.6e}, k* {k_star}")
    assert 8 < k_star < fx.MAXIT and k_star % 8 != 0
    for r, p in enumerate(parts):
        label = (world, sc["name"], r)
        assert int(p[k + "err"]) == 0, label                                    # 9. no peer-to-peer time-out
        assert np.array_equal(bits_of(p[k + "H"]), bits_of(parts[0][k + "H"])), label      # reduced values: the same bits on every rank
        assert int(p[k + "k_star"]) == k_star and bool(p[k + "h_ref_ok"]), label
        # 3.
        assert int(p[k + "its"]) == k_star and int(p[k + "done"]) == k_star, (label, int(p[k + "its"]))
        assert len(p[k + "h"]) == k_star + 1, label
        assert bool(p[k + "x_ok"]) and bool(p[k + "h_ok"]), label
        assert int(p[k + "its_again"]) == k_star and bool(p[k + "x_again_ok"]), label
        assert int(p[k + "iterate_status"]) == ERR_STATE and bool(p[k + "x_after_refusal_ok"]), label
        assert bool(p[k + "h_after_set_rhs_ok"]), label
        # 4. - 6.
        assert list(p[k + "check_every_ok"]) == [True] * len(CHECK_EVERY), (label, list(p[k + "check_every_ok"]))
        assert list(p[k + "two_calls"]) == [5, k_star] and bool(p[k + "two_calls_ok"]), (label, list(p[k + "two_calls"]))
        assert int(p[k + "after_iterate"]) == k_star and bool(p[k + "after_iterate_ok"]), label
    if sc["flags"] & RESIDENT:
        assert all(int(p[k + "launches"]) in (4, 7) for p in parts)            # the launched loop, as the preconditioner demands


def bits_of(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("world,i", [c for c in CASES if _scenarios(c[0])[c[1]].get("oracle")],
                         ids=[n for c, n in zip(CASES, IDS) if _scenarios(c[0])[c[1]].get("oracle")])
def test_stopped_solve_against_the_serial_oracle(tmp_path_factory, world, i):
    """x and history of the stopped solve against the serial oracle stopped by the same rule (test_gpu_dist_p2p.py's tolerances)"""
    import dist_pcg_oracle as dpo
    import dist_until_fixture as fx
    parts = _results(world, tmp_path_factory)
    sc, k = _scenarios(world)[i], f"s{i}_"
    dtype = np.dtype(sc["dtype"])
    ht, xt = (1e-10, 1e-9) if dtype in (np.dtype(np.float64), np.dtype(np.complex128)) else (1e-4, 1e-3)
    A, b = _system(sc["kind"])
    # the oracle works on the values the device holds: the matrix and b rounded to the handle's type
    A, b = A.astype(dtype).astype(A.dtype), b.astype(dtype).astype(b.dtype if dtype.kind == "c" else np.float64)
    M = None if sc["pre"] is None else dpo.global_m(A, dpo.row_ranges(A.shape[0], world), sc["pre"])
    tol = float(parts[0][k + "tol"])
    _, ho = dpo.oracle(A, b, M, fx.MAXIT)
    k_o = fx.stop_index(ho, tol)
    its = int(parts[0][k + "its"])
    assert k_o == its, (k_o, its)
    xo, ho = dpo.oracle(A, b, M, k_o)
    h = parts[0][k + "h"]
    x = np.concatenate([p[k + "x"] for p in parts])
    eh = float(np.max(np.abs(h - ho) / np.abs(ho)))
    ex = float(np.linalg.norm(x - xo) / np.linalg.norm(xo))
    print(f"  world {world} {sc['name']}: stopped at {its}, history max rel dev {eh:.3e} (< {ht:g}), x rel err {ex:.3e} (< {xt:g})")
    assert eh < ht and ex < xt, (eh, ex)


@pytest.mark.parametrize("world", [1, 2, 3], ids=["w1", "w2", "w3"])
def test_nan_stops_every_rank_at_once(tmp_path_factory, world):
    """b with one NaN entry on one rank: r.r is NaN on every rank from the first reduction on, and NaN stops"""
    parts = _results(world, tmp_path_factory)
    for p in parts:
        assert int(p["nan_its"]) == 1 and len(p["nan_h"]) == 2 and np.isnan(p["nan_h"][1])
        assert int(p["nan_err"]) == 0


@pytest.mark.parametrize("world", [1, 2, 3], ids=["w1", "w2", "w3"])
def test_a_handle_that_never_stops_is_unchanged(tmp_path_factory, world):
    """set_rhs; iterate(24) on a handle that never calls iterate_until: the bits of the fixed-count run of one that later does (and
    the ranks' histories are each other's, asserted with the scenarios)"""
    parts = _results(world, tmp_path_factory)
    for p in parts:
        assert bool(p["plain_ok"]) and int(p["plain_err"]) == 0


def test_single_reduction_handle_refuses(tmp_path_factory):
    parts = _results(2, tmp_path_factory)
    for p in parts:
        assert int(p["sr_status"]) == ERR_STATE
        assert "single-reduction" in str(p["sr_text"]) and "CGAMD_DIST_SINGLE_REDUCTION" in str(p["sr_text"])
        assert len(p["sr_h"]) == 13 and np.all(np.isfinite(p["sr_h"])) and int(p["sr_err"]) == 0
