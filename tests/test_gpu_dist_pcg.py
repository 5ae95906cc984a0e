"""GPU tests of preconditioned CG on the row-partitioned handle (cgamd_dist_set_preconditioner, _jacobi, _line;
DistSolver.set_preconditioner).  As in test_gpu_dist_p2p.py the ranks are separate processes that share cuda:0 over the peer-to-peer
backend.  The oracle is the serial PCG in double / complex double whose preconditioner is the block-diagonal of the per-rank M,
assembled globally (dist_pcg_oracle.py): the global diagonal for Jacobi, the global tridiagonal at the stride with every link
that crosses a rank boundary removed for the lines.

Tolerances.  test_gpu_dist_p2p.py (dist against oracle) holds the history to 1e-10 (fp64 / complex128) or 1e-4 (single) while it
is above 1e-8 / 1e-4 of its first entry, and x to 1e-9 / 1e-3; test_gpu_tridiag.py (line PCG against oracle) holds the history to
1e-10 / 1e-4 over the same entries and x to 1e-9 / 1e-4.  They differ only in x for the single-precision types; the looser one,
test_gpu_dist_p2p.py's 1e-3, is used."""
import importlib
import os
import socket
import sys

import numpy as np
import pytest

from conftest import PKG_NAME, ROOT

pytestmark = pytest.mark.gpu

NX, NY, NZ = 12, 10, 18
ERR_INVALID, ERR_STATE = 1, 7


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _tols(dtype):
    """(history, x, history entries compared: above this fraction of the first)"""
    return (1e-10, 1e-9, 1e-8) if np.dtype(dtype) in (np.dtype(np.float64), np.dtype(np.complex128)) else (1e-4, 1e-3, 1e-4)


def _system(kind):
    """(A as scipy CSR in double / complex double, b)"""
    import dist_pcg_oracle as dpo
    if kind == "aniso":
        A = dpo.aniso_grid(NX, NY, NZ)
    elif kind == "aniso_big":       # the slab loop applies to its ranks' slabs (test_gpu_dist_p2p.py's 24 x 20 x 36 rows)
        A = dpo.aniso_grid(24, 20, 36)
    elif kind == "chain":
        A = dpo.chain(1001)
    elif kind == "chain_long":      # more rows per rank than one chunk of the stride-1 sweep holds: its three-launch form
        A = dpo.chain(4001)
    elif kind == "grid":
        A = dpo.aniso_grid(11, 7, 5, cz=1.0)
    elif kind == "helm":
        return dpo.helm(60)
    else:
        raise ValueError(kind)
    return A, np.linspace(1.0, 2.0, A.shape[0])


def _zeroed(A, world):
    """the diagonal entry of one row of rank 1 zeroed (stored, value 0): (matrix, global row, local row)"""
    import scipy.sparse as sp
    rb, re = A.shape[0] * 1 // world, A.shape[0] * 2 // world
    row = rb + (re - rb) // 3 // NX * NX        # the first row of an x-line: the line factorisation meets the zero as a pivot
    A = sp.csr_matrix(A, copy=True)
    for j in range(A.indptr[row], A.indptr[row + 1]):
        if A.indices[j] == row:
            A.data[j] = 0.0
    return A, row, row - rb


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
        A, b = _system(sc["kind"])
        dtype = np.dtype(sc["dtype"])
        mode, flags, comm = sc["mode"], sc.get("flags", 0), sc.get("comm", "p2p")
        if mode == "fail":
            A, _, bad_local = _zeroed(A, world)
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
        if flags & 512:     # slab loop: needs the column codes; the ranks' resident launches share the GPU
            pkg._lib.check(lib.cgamd_tune(b"index_codes_min_mb", 0))
            pkg._lib.check(lib.cgamd_tune(b"dev.resident_lock", 0))

        def make():
            uid = dmod.broadcast_unique_id(rank) if comm == "rccl" else None
            return dmod.DistSolver(ctx, plan, indptr, vals, dtype, unique_id=uid, flags=flags, comm=comm)

        def solve(s, parts):
            s.set_rhs(bl, None)
            for k in parts:
                s.iterate(k)
            x = s.x(torch.empty(plan.n_local, dtype=bl.dtype, device=dev)).cpu().numpy()
            return x, s.history()

        out = {}
        s = make()
        if mode == "parity":        # one handle, the preconditioners one after the other (a captured graph is dropped at each change)
            for i, pre in enumerate(sc["pres"]):
                s.set_preconditioner(pre)
                out[f"launches{i}"] = s.loop_launches()
                out[f"x{i}"], out[f"h{i}"] = solve(s, (sc["iters"],))
        elif mode == "one_rank":    # against the single-GPU handle on the same matrix with the same preconditioner
            ref = pkg.Solver(ctx, n, len(vals_loc), vals_loc.astype(dtype), ip_loc, cols_glob.astype(np.int32), 1)
            for i, pre in enumerate(sc["pres"]):
                s.set_preconditioner(pre)
                out[f"x{i}"], out[f"h{i}"] = solve(s, (sc["iters"],))
                ref.set_preconditioner(pre)
                xr, hr = ref.solve(b.astype(dtype), None, sc["iters"])
                out[f"xr{i}"], out[f"hr{i}"] = xr, hr[:, 0]
            ref.close()
        elif mode == "removal":     # line, solve, None, solve: the bits of a handle that never had a preconditioner
            out["x_fresh"], out["h_fresh"] = solve(s, (30,))
            s.close()
            s = make()
            s.set_preconditioner(("line", 1))
            out["x_line"], out["h_line"] = solve(s, (30,))
            s.set_preconditioner(None)
            out["x_after"], out["h_after"] = solve(s, (30,))
        elif mode == "split":
            for i, pre in enumerate(sc["pres"]):
                s.set_preconditioner(pre)
                out[f"x{i}a"], out[f"h{i}a"] = solve(s, (30,))
                out[f"x{i}b"], out[f"h{i}b"] = solve(s, (10, 10, 10))
        elif mode == "fail":        # rank 1 fails locally; EVERY rank must raise, name rank 1 and the local row, and fall back to plain CG
            msgs = []
            for pre in ("jacobi", ("line", 1)):
                try:
                    s.set_preconditioner(pre)
                    msgs.append("no error")
                except pkg._lib.CgAmdError as e:
                    msgs.append(f"{e.status}|{e}")
            out["msgs"] = np.array(msgs)
            out["bad_local"] = bad_local
            out["launches"] = s.loop_launches()
            out["x"], out["h"] = solve(s, (12,))
        elif mode == "excluded_sr":  # single-reduction handle: the three setters return CGAMD_ERR_STATE
            m = torch.ones(plan.n_local, dtype=bl.dtype, device=dev)
            torch.cuda.synchronize()
            codes, texts = [], []
            for call in (lambda: lib.cgamd_dist_set_preconditioner(s.handle, pkg._lib.ptr(m)),
                         lambda: lib.cgamd_dist_set_preconditioner_jacobi(s.handle),
                         lambda: lib.cgamd_dist_set_preconditioner_line(s.handle, 1)):
                codes.append(call())
                texts.append(lib.cgamd_last_error().decode(errors="replace"))
            out["codes"], out["texts"] = np.array(codes), np.array(texts)
            out["x"], out["h"] = solve(s, (12,))          # the handle still runs its own loop
        elif mode == "resident":    # slab handle: with a preconditioner set it runs (and reports) a launched loop
            out["launches_before"] = s.loop_launches()
            s.set_preconditioner(sc["pres"][0])
            out["launches_pcg"] = s.loop_launches()
            out["x0"], out["h0"] = solve(s, (sc["iters"],))      # one call of >= 16 iterations: what the slab loop would take whole
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


def _spawn(tmp_path, world, sc):
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(world, _free_port(), sc, str(tmp_path)), nprocs=world, join=True)
    parts = [np.load(os.path.join(str(tmp_path), f"r{r}.npz")) for r in range(world)]
    assert all(int(p["err"]) == 0 for p in parts)
    return parts


def _hist_dev(h, ref, scale, keep):
    """max over the kept entries of |h - ref| / |scale| (not finite counts as infinite)"""
    with np.errstate(all="ignore"):
        d = np.abs(np.asarray(h) - ref) / np.abs(scale)
    return float(np.max(np.where(np.isfinite(d), d, np.inf)[keep]))


def _check(parts, key, A, b, M, iters, dtype, label):
    """x / history `key` of all ranks against the serial oracle with M; returns (oracle history, kept entries)"""
    import dist_pcg_oracle as dpo
    ht, xt, floor = _tols(dtype)
    xo, ho = dpo.oracle(A, b, M, iters)
    for p in parts[1:]:
        assert np.array_equal(p[f"h{key}"], parts[0][f"h{key}"]), label       # rank-ordered sums: bitwise identical on all ranks
    h = parts[0][f"h{key}"]
    assert len(h) == iters + 1, (label, len(h))
    keep = np.abs(ho) / np.abs(ho[0]) > floor
    eh = _hist_dev(h, ho, ho, keep)
    x = np.concatenate([p[f"x{key}"] for p in parts])
    ex = float(np.linalg.norm(x - xo) / np.linalg.norm(xo))
    print(f"  {label}: {int(keep.sum())} history entries compared, max rel dev {eh:.3e} (< {ht:g}), x rel err {ex:.3e} (< {xt:g})")
    assert eh < ht, (label, eh)
    assert ex < xt, (label, ex)
    return ho, keep


PRES = ["jacobi", ("line", 1), ("line", NX), ("line", NX * NY)]


# 1. parity with the serial oracle.  flags: 0 = four-launch loop, 8 = from a hipGraph, 128 = staged push / unpack / all-reduce launches
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("flags", [0, 8, 128, 128 | 8])
def test_parity_fp64(tmp_path, world, flags):
    import dist_pcg_oracle as dpo
    parts = _spawn(tmp_path, world, dict(mode="parity", kind="aniso", dtype="float64", flags=flags, pres=PRES, iters=30))
    A, b = _system("aniso")
    ranges = dpo.row_ranges(A.shape[0], world)
    for i, pre in enumerate(PRES):
        _check(parts, i, A, b, dpo.global_m(A, ranges, pre), 30, np.float64, f"world {world} flags {flags} {pre}")
        launches = [int(p[f"launches{i}"]) for p in parts]
        print(f"  launches per iteration {launches}")
        assert all(l == 7 for l in launches) if flags & 128 else all(l in (4, 7) for l in launches), launches


@pytest.mark.parametrize("world,kind,dtype,flags,pres", [(2, "aniso", "float32", 0, ["jacobi", ("line", NX * NY)]),
                                                         (3, "helm", "complex64", 0, ["jacobi", ("line", 1)]),
                                                         (2, "helm", "complex128", 8, ["jacobi", ("line", 1)])])
def test_parity_other_types(tmp_path, world, kind, dtype, flags, pres):
    import dist_pcg_oracle as dpo
    parts = _spawn(tmp_path, world, dict(mode="parity", kind=kind, dtype=dtype, flags=flags, pres=pres, iters=30))
    A, b = _system(kind)
    # the oracle works on the values the device holds: the matrix and b rounded to the handle's type
    A, b = A.astype(dtype).astype(A.dtype), b.astype(dtype).astype(b.dtype if np.dtype(dtype).kind == "c" else np.float64)
    ranges = dpo.row_ranges(A.shape[0], world)
    for i, pre in enumerate(pres):
        _check(parts, i, A, b, dpo.global_m(A, ranges, pre), 30, dtype, f"{dtype} world {world} {pre}")


# 2. a rank boundary inside a line, and the halo alias: row n_local - 1 coupled to halo slot 0 sits at column offset +1
@pytest.mark.parametrize("kind,iters,want_launches", [("chain", 3, 4), ("grid", 30, 4), ("chain_long", 3, 6)])
def test_lines_end_at_the_rank_boundary(tmp_path, kind, iters, want_launches):
    import dist_pcg_oracle as dpo
    world, pre = 3, ("line", 1)
    A, b = _system(kind)
    ranges = dpo.row_ranges(A.shape[0], world)
    assert all(rb % 11 for rb, _ in ranges[1:]) or kind != "grid"          # the row ranges fall mid-x-line
    M_cut, M_uncut = dpo.global_m(A, ranges, pre), dpo.global_m(A, ranges, pre, cut=False)
    assert (M_uncut - M_cut).nnz == 2 * (world - 1)
    ht = _tols(np.float64)[0]
    _, h_cut = dpo.oracle(A, b, M_cut, iters)
    _, h_uncut = dpo.oracle(A, b, M_uncut, iters)
    keep = np.abs(h_cut) / np.abs(h_cut[0]) > 1e-8
    apart = _hist_dev(h_uncut, h_cut, h_cut, keep)
    assert apart >= 100 * ht, apart            # on the CPU first: otherwise this test could not see the alias
    parts = _spawn(tmp_path, world, dict(mode="parity", kind=kind, dtype="float64", flags=0, pres=[pre], iters=iters))
    _check(parts, 0, A, b, M_cut, iters, np.float64, f"{kind} cut M")
    wrong = _hist_dev(parts[0]["h0"], h_uncut, h_cut, keep)
    print(f"  {kind}: the two oracles are {apart:.3e} apart; the device is {wrong:.3e} from the uncut one")
    assert wrong > ht
    launches = [int(p["launches0"]) for p in parts]
    assert all(l in (want_launches, want_launches + 3) for l in launches), launches      # (+3: the staged loop, where the SpMV grid cannot carry the push)


# 3. one rank, no peers: against the single-GPU handle with the same preconditioner, within the same tolerance
@pytest.mark.parametrize("comm", ["p2p", "rccl"])
def test_one_rank_matches_the_single_gpu_handle(tmp_path, comm):
    pres = ["jacobi", ("line", 1), ("line", NX * NY)]
    parts = _spawn(tmp_path, 1, dict(mode="one_rank", kind="aniso", dtype="float64", comm=comm, pres=pres, iters=30))
    ht, xt, floor = _tols(np.float64)
    p = parts[0]
    for i, pre in enumerate(pres):
        hr = p[f"hr{i}"]
        keep = np.abs(hr) / np.abs(hr[0]) > floor
        eh = _hist_dev(p[f"h{i}"], hr, hr, keep)
        ex = float(np.linalg.norm(p[f"x{i}"] - p[f"xr{i}"]) / np.linalg.norm(p[f"xr{i}"]))
        print(f"  {comm} {pre}: history {eh:.3e}, x {ex:.3e}")
        assert eh < ht and ex < xt, (comm, pre, eh, ex)


# 4. removal, 5. split calls
@pytest.mark.parametrize("flags", [0, 8])
def test_removal_gives_the_bits_of_a_fresh_handle(tmp_path, flags):
    parts = _spawn(tmp_path, 2, dict(mode="removal", kind="aniso", dtype="float64", flags=flags))
    for p in parts:
        assert np.array_equal(p["h_after"].view(np.uint8), p["h_fresh"].view(np.uint8))
        assert np.array_equal(p["x_after"].view(np.uint8), p["x_fresh"].view(np.uint8))
        assert not np.array_equal(p["h_line"], p["h_fresh"])          # (the preconditioner was in force in between)


@pytest.mark.parametrize("flags", [0, 128 | 8])
def test_split_calls(tmp_path, flags):
    pres = ["jacobi", ("line", NX * NY)]
    parts = _spawn(tmp_path, 3, dict(mode="split", kind="aniso", dtype="float64", flags=flags, pres=pres))
    for p in parts:
        for i in range(len(pres)):
            assert np.array_equal(p[f"h{i}a"].view(np.uint8), p[f"h{i}b"].view(np.uint8))
            assert np.array_equal(p[f"x{i}a"].view(np.uint8), p[f"x{i}b"].view(np.uint8))


# 6. iterations to 1e-6 ||b||: each count within one of the serial oracle's, cut z-lines need fewer than Jacobi
def test_iterations_to_tolerance(tmp_path):
    import dist_pcg_oracle as dpo
    world = 2
    A, b = _system("aniso")
    ranges = dpo.row_ranges(A.shape[0], world)
    ks = {}
    for pre in ("jacobi", ("line", NX * NY)):
        _, ho = dpo.oracle(A, b, dpo.global_m(A, ranges, pre), 200)
        k_oracle = dpo.first_below(ho, b)
        assert k_oracle is not None
        sub = tmp_path / str(pre[0] if isinstance(pre, tuple) else pre)
        sub.mkdir()
        parts = _spawn(sub, world, dict(mode="parity", kind="aniso", dtype="float64", flags=0, pres=[pre], iters=k_oracle + 3))
        k = dpo.first_below(parts[0]["h0"], b)
        print(f"  {pre}: first k with sqrt|r.r| < 1e-6 ||b||: device {k}, serial oracle {k_oracle}")
        assert k is not None and abs(k - k_oracle) <= 1, (pre, k, k_oracle)
        ks[pre] = k
    assert ks[("line", NX * NY)] < ks["jacobi"], ks


# 7. rank agreement on failure: an error return on one rank is raised on all of them; nothing faults
def test_all_ranks_raise_when_one_fails(tmp_path):
    import dist_pcg_oracle as dpo
    world = 3
    parts = _spawn(tmp_path, world, dict(mode="fail", kind="aniso", dtype="float64", flags=0))
    A, b = _system("aniso")
    A0, _, bad_local = _zeroed(A, world)
    for p in parts:
        assert int(p["bad_local"]) == bad_local
        for msg, who in zip(p["msgs"], ("dist_set_preconditioner_jacobi", "dist_set_preconditioner_line")):
            status, text = str(msg).split("|", 1)
            assert int(status) == ERR_INVALID, msg
            assert "rank 1" in text and who in text and f"row {bad_local}" in text, msg
    # afterwards the same handles run plain CG (the zeroed diagonal is part of the system: 12 iterations of plain CG on it)
    _check(parts, "", A0, b, None, 12, np.float64, "plain CG after the failure")
    assert all(int(p["launches"]) in (4, 7) for p in parts)


# 8. excluded flags
def test_single_reduction_handle_refuses(tmp_path):
    parts = _spawn(tmp_path, 2, dict(mode="excluded_sr", kind="aniso", dtype="float64", flags=256))
    for p in parts:
        assert list(p["codes"]) == [ERR_STATE] * 3, p["codes"]
        assert all("single-reduction loop" in str(t) and "no PCG form" in str(t) for t in p["texts"]), p["texts"]
        assert np.all(np.isfinite(p["h"])) and len(p["h"]) == 13


def test_resident_handle_runs_its_launched_loop(tmp_path):
    import dist_pcg_oracle as dpo
    world, pre = 2, ("line", 24 * 20)
    parts = _spawn(tmp_path, world, dict(mode="resident", kind="aniso_big", dtype="float64", flags=512, pres=[pre], iters=20))
    A, b = _system("aniso_big")
    print("  launches before / with / after the preconditioner:", [(int(p["launches_before"]), int(p["launches_pcg"]), int(p["launches_after"])) for p in parts])
    for p in parts:
        assert int(p["launches_before"]) == 0 and int(p["launches_after"]) == 0       # the slab loop: whole calls in one launch
        assert int(p["launches_pcg"]) in (4, 7)
    _check(parts, 0, A, b, dpo.global_m(A, dpo.row_ranges(A.shape[0], world), pre), 20, np.float64, "slab handle, cut z-lines")
