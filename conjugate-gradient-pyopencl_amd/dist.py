"""Row-partitioned multi-GPU CG: one process per GPU, torch.distributed for the plumbing, RCCL over xGMI
inside the C loop (csrc/dist.cpp).

The reference's only multi-GPU mode replicates the matrix on every device and splits the right-hand
sides over devices with no communication (p_h-PY_C-CL-multi-GPU.py:2123-2181, cl.py:203-360); that mode
is `cl.conjugate_gradient_multi_gpu`.  BASELINE.json's north star asks for the MATRIX to be row-
partitioned across the 8 GPUs with an all-reduce for the two dot products of every iteration and a
boundary exchange for A*d; this module is that (new design, no reference counterpart):

  1. `row_ranges`           contiguous row blocks [n*g//G, n*(g+1)//G)
  2. `build_halo_plan`      from the GLOBAL column indices of a rank's rows: which entries of d it needs
                            from which rank (halo), which of its own rows the others need (send lists),
                            and the columns renumbered to [0,n_local) U [n_local, n_local+n_halo)
  3. `DistSolver`           the C loop: pack -> ncclSend/ncclRecv -> SpMV(+d.q) -> ncclAllReduce ->
                            x/r update(+r.r) -> ncclAllReduce -> d update; no host sync inside
  4. `cg_loop`              the same recurrence written against two small interfaces (local ops, comm);
                            used by the CPU/gloo tests with the oracle's kernels, and usable on GPUs as a
                            slow cross-check of the C loop (per-iteration torch.distributed calls).
  5. `DistSolver.solve_until` / `iterate_until`: the C loop solved to a tolerance, the stop decided on the device from the
                            all-reduced r.r (cgamd_dist_iterate_until); `cg_loop_until` / `pcg_loop_until` are its host mirrors.

Everything in steps 1-2 is backend agnostic (CPU tensors + gloo, or CUDA tensors + nccl).
"""
import ctypes
import os
from dataclasses import dataclass, field
from typing import List

import numpy as np

from . import _lib
from ._lib import check, ptr


def row_ranges(n, world, indptr=None):
    """[(begin, end)] of the contiguous row block of every rank.

    Without `indptr`: equal row counts (what a stencil wants).  With the global row pointers (any array-like of n + 1
    non-decreasing integers): contiguous blocks of (nearly) equal NON-ZERO counts -- rank g ends at the first row whose
    pointer reaches g+1 shares of nnz -- for matrices whose rows differ in length (the SpMV streams non-zeros, so that is what
    balances the ranks); every rank keeps at least one row while there are rows left."""
    if indptr is None:
        return [(n * g // world, n * (g + 1) // world) for g in range(world)]
    ip = np.asarray(indptr.cpu() if hasattr(indptr, "cpu") else indptr, dtype=np.int64)
    if ip.shape[0] != n + 1:
        raise ValueError("indptr must have n + 1 entries")
    nnz = int(ip[-1])
    cuts = [0]
    for g in range(1, world):
        target = (nnz * g + world - 1) // world
        r = int(np.searchsorted(ip, target, side="left"))
        r = min(max(r, cuts[-1] + 1), n - (world - g))      # at least one row per rank on either side
        cuts.append(max(r, cuts[-1]))
    cuts.append(n)
    return [(cuts[g], cuts[g + 1]) for g in range(world)]


def local_grid_dims(dims, ranges, rank):
    """(nx, ny, nz) of the box a rank owns of a grid numbered x fastest, for DistSolver.set_preconditioner(("multigrid", ...)).
    dims: the global (nx, ny, nz), or (nx, ny) for nz = 1; ranges: `row_ranges`' blocks.  The rank's rows must be whole planes of
    nx * ny nodes (z-slabs), or whole x-lines of a grid with nz == 1; anything else is not a box and raises ValueError (the
    algebraic form, "amg", takes any row range)."""
    dims = tuple(int(v) for v in dims)
    if len(dims) not in (2, 3) or any(v < 1 for v in dims):
        raise ValueError(f"local_grid_dims: dims must be (nx, ny) or (nx, ny, nz) with positive entries, got {dims!r}")
    nx, ny, nz = dims + (1,) * (3 - len(dims))
    rb, re = (int(v) for v in ranges[rank])
    if not 0 <= rb < re <= nx * ny * nz:
        raise ValueError(f"local_grid_dims: rows [{rb}, {re}) of rank {rank} are not rows of a {nx} x {ny} x {nz} grid")
    unit, what = (nx * ny, "planes") if nz > 1 else (nx, "x-lines")
    if rb % unit or re % unit:
        raise ValueError(f"local_grid_dims: rows [{rb}, {re}) of rank {rank} are not whole {what} of {unit} nodes")
    return (nx, ny, (re - rb) // unit) if nz > 1 else (nx, (re - rb) // unit, 1)


@dataclass
class HaloPlan:
    rank: int
    world: int
    row_begin: int
    row_end: int
    n_local: int
    n_halo: int
    cols_local: object                 # torch int32, columns renumbered to local U halo
    halo_global: object                # torch int64 [n_halo], sorted global ids of the halo entries
    peers: List[int] = field(default_factory=list)         # ranks exchanged with, ascending
    send_counts: List[int] = field(default_factory=list)   # entries sent to each peer
    recv_counts: List[int] = field(default_factory=list)   # entries received from each peer (halo order)
    send_index: object = None          # torch int32: concatenated LOCAL row ids to send, peer by peer


def build_halo_plan(cols_global, ranges, rank, group=None):
    """Partition plan of one rank.  cols_global: 1-D torch integer tensor with the GLOBAL column index
    of every stored entry of this rank's rows (CPU or CUDA).  Collective over `group` when world > 1."""
    import torch
    import torch.distributed as dist
    world = len(ranges)
    rb, re = ranges[rank]
    n_local = re - rb
    c = cols_global.to(torch.int64)
    off = (c < rb) | (c >= re)
    halo_global = torch.unique(c[off])                      # sorted
    starts = torch.tensor([r[0] for r in ranges] + [ranges[-1][1]], dtype=torch.int64, device=c.device)
    owner = torch.searchsorted(starts, halo_global, right=True) - 1
    # columns -> local numbering
    cols_local = torch.where(off, n_local + torch.searchsorted(halo_global, c), c - rb).to(torch.int32)
    need = {}                                               # owner rank -> global ids wanted from it (sorted)
    if halo_global.numel():
        owners, counts = torch.unique_consecutive(owner, return_counts=True)
        pos = 0
        for o, k in zip(owners.tolist(), counts.tolist()):
            need[int(o)] = halo_global[pos:pos + k].cpu()
            pos += k
    # tell every owner which of its rows we need (setup only: object all-gather keeps this backend agnostic)
    if world > 1:
        gathered = [None] * world
        dist.all_gather_object(gathered, need, group=group)
    else:
        gathered = [need]
    wanted_from_me = {src: req[rank] for src, req in enumerate(gathered) if src != rank and rank in req}
    peers = sorted(set(need) | set(wanted_from_me))
    send_counts, recv_counts, send_lists = [], [], []
    for p in peers:
        s = wanted_from_me.get(p)
        send_counts.append(0 if s is None else int(s.numel()))
        if s is not None:
            send_lists.append((s - rb).to(torch.int32))
        recv_counts.append(int(need[p].numel()) if p in need else 0)
    send_index = (torch.cat(send_lists) if send_lists else torch.zeros(0, dtype=torch.int32)).to(c.device)
    return HaloPlan(rank, world, rb, re, n_local, int(halo_global.numel()), cols_local, halo_global, peers,
                    send_counts, recv_counts, send_index)


# ---------------------------------------------------------------------------------------------------
# generic distributed recurrence (reference clcg.c:250-430 with the two extra communication steps)
# ---------------------------------------------------------------------------------------------------
class TorchComm:
    """halo exchange + scalar all-reduce over torch.distributed (gloo on CPU, nccl = RCCL on GPUs)."""

    def __init__(self, plan, group=None):
        self.plan, self.group = plan, group

    def exchange(self, v_ext):
        """fill v_ext[n_local:] with the neighbours' entries; v_ext is a torch tensor"""
        import torch
        import torch.distributed as dist
        p = self.plan
        if not p.peers:
            return
        ops, so, ro = [], 0, p.n_local
        sendbuf = v_ext[p.send_index.long()]
        for peer, sc, rc in zip(p.peers, p.send_counts, p.recv_counts):
            if sc:
                ops.append(dist.P2POp(dist.isend, sendbuf[so:so + sc].contiguous(), peer, group=self.group))
            if rc:
                ops.append(dist.P2POp(dist.irecv, v_ext[ro:ro + rc], peer, group=self.group))
            so += sc
            ro += rc
        for w in dist.batch_isend_irecv(ops):
            w.wait()

    def allreduce(self, t):
        import torch.distributed as dist
        if self.plan.world > 1:
            dist.all_reduce(t, group=self.group)
        return t


def cg_loop(ops, comm, plan, b_local, x0_local, n_iterations):
    """Distributed fixed-iteration (CO)CG on torch tensors.

    ops: local kernels on this rank's rows --
         ops.spmv(v_ext) -> A_local @ v_ext, ops.dot(a, b) -> 0-d tensor (unconjugated, local part).
    Returns (x_local, history[n_iterations+1]) with history[k] = global r_k . r_k.
    """
    import torch
    n = plan.n_local
    x = x0_local.clone()
    d_ext = torch.zeros(n + plan.n_halo, dtype=b_local.dtype, device=b_local.device)
    d_ext[:n] = x
    comm.exchange(d_ext)
    r = b_local - ops.spmv(d_ext)                                   # clcg.c:255-260
    d_ext[:n] = r                                                   # :264
    delta_new = comm.allreduce(ops.dot(r, r).reshape(1).clone())    # :268-279 + all-reduce
    hist = [delta_new.clone()]
    for _ in range(n_iterations):                                   # :297
        comm.exchange(d_ext)                                        # boundary exchange of d
        q = ops.spmv(d_ext)                                         # :299-305
        dq = comm.allreduce(ops.dot(d_ext[:n], q).reshape(1).clone())   # :309-324 + all-reduce
        alpha = delta_new / dq                                      # :326-327
        x = x + alpha * d_ext[:n]                                   # :338-342
        r = r - alpha * q                                           # :345-349
        delta_old = delta_new
        delta_new = comm.allreduce(ops.dot(r, r).reshape(1).clone())    # :369-387 + all-reduce
        beta = delta_new / delta_old                                # :389-391
        d_ext[:n] = beta * d_ext[:n] + r                            # :415
        hist.append(delta_new.clone())
    return x, torch.cat(hist)


def pcg_loop(ops, comm, plan, b_local, x0_local, n_iterations, apply_m):
    """The preconditioned form of `cg_loop` (what csrc/dist.cpp runs once DistSolver.set_preconditioner is in force), with a
    RANK-LOCAL preconditioner: apply_m(r_local) -> z_local = M^-1 r_local needs no communication (a diagonal, or line solves cut at
    the rank's row range -- block-Jacobi over the ranks, symmetric and positive definite whenever A is).  rho = r.z drives alpha
    and beta; r.z and r.r travel in ONE all-reduce.  Returns (x_local, history[n_iterations+1]) with history[k] = global r_k . r_k,
    as cg_loop does.  With apply_m the identity the iterates are cg_loop's, bit for bit."""
    import torch
    n = plan.n_local
    x = x0_local.clone()
    d_ext = torch.zeros(n + plan.n_halo, dtype=b_local.dtype, device=b_local.device)
    d_ext[:n] = x
    comm.exchange(d_ext)
    r = b_local - ops.spmv(d_ext)
    z = apply_m(r)
    d_ext[:n] = z                                                   # d = z0
    red = comm.allreduce(torch.stack([ops.dot(r, z), ops.dot(r, r)]).clone())      # the one round: {r.z, r.r}
    rho = red[0:1].clone()
    hist = [red[1:2].clone()]
    for _ in range(n_iterations):
        comm.exchange(d_ext)
        q = ops.spmv(d_ext)
        dq = comm.allreduce(ops.dot(d_ext[:n], q).reshape(1).clone())
        alpha = rho / dq
        x = x + alpha * d_ext[:n]
        r = r - alpha * q
        z = apply_m(r)
        rho_old = rho
        red = comm.allreduce(torch.stack([ops.dot(r, z), ops.dot(r, r)]).clone())
        rho = red[0:1].clone()
        beta = rho / rho_old
        d_ext[:n] = beta * d_ext[:n] + z
        hist.append(red[1:2].clone())
    return x, torch.cat(hist)


def _stops(delta, tol):
    """the stopping rule of cgamd_dist_iterate_until on the all-reduced r.r (a 1-element tensor): !(sqrt|delta| >= tol), in double;
    NaN stops"""
    v = complex(delta.reshape(-1)[0].item())
    return not (np.sqrt(np.abs(v)) >= tol)


def cg_loop_until(ops, comm, plan, b_local, x0_local, tol, maxit):
    """`cg_loop` solved to a tolerance (host mirror of cgamd_dist_iterate_until): the same recurrence, line for line, left in the
    first iteration k >= 1 whose all-reduced r_k . r_k fails sqrt|r.r| >= tol (NaN fails it), after at most `maxit` iterations.
    The decision is taken from the all-reduced value, which every rank holds alike, so the ranks leave together.
    Returns (x_local, history[its + 1], its): the iterate and the history of exactly `its` iterations of `cg_loop`."""
    import torch
    n = plan.n_local
    x = x0_local.clone()
    d_ext = torch.zeros(n + plan.n_halo, dtype=b_local.dtype, device=b_local.device)
    d_ext[:n] = x
    comm.exchange(d_ext)
    r = b_local - ops.spmv(d_ext)                                   # clcg.c:255-260
    d_ext[:n] = r                                                   # :264
    delta_new = comm.allreduce(ops.dot(r, r).reshape(1).clone())    # :268-279 + all-reduce
    hist = [delta_new.clone()]
    its = 0
    for _ in range(maxit):                                          # :297
        comm.exchange(d_ext)                                        # boundary exchange of d
        q = ops.spmv(d_ext)                                         # :299-305
        dq = comm.allreduce(ops.dot(d_ext[:n], q).reshape(1).clone())   # :309-324 + all-reduce
        alpha = delta_new / dq                                      # :326-327
        x = x + alpha * d_ext[:n]                                   # :338-342
        r = r - alpha * q                                           # :345-349
        delta_old = delta_new
        delta_new = comm.allreduce(ops.dot(r, r).reshape(1).clone())    # :369-387 + all-reduce
        beta = delta_new / delta_old                                # :389-391
        d_ext[:n] = beta * d_ext[:n] + r                            # :415
        hist.append(delta_new.clone())
        its += 1
        if _stops(delta_new, tol):
            break
    return x, torch.cat(hist), its


def pcg_loop_until(ops, comm, plan, b_local, x0_local, tol, maxit, apply_m):
    """`pcg_loop` solved to a tolerance, by the rule of `cg_loop_until`: the test looks at r.r (what the history records), not at
    rho.  Returns (x_local, history[its + 1], its)."""
    import torch
    n = plan.n_local
    x = x0_local.clone()
    d_ext = torch.zeros(n + plan.n_halo, dtype=b_local.dtype, device=b_local.device)
    d_ext[:n] = x
    comm.exchange(d_ext)
    r = b_local - ops.spmv(d_ext)
    z = apply_m(r)
    d_ext[:n] = z                                                   # d = z0
    red = comm.allreduce(torch.stack([ops.dot(r, z), ops.dot(r, r)]).clone())      # the one round: {r.z, r.r}
    rho = red[0:1].clone()
    hist = [red[1:2].clone()]
    its = 0
    for _ in range(maxit):
        comm.exchange(d_ext)
        q = ops.spmv(d_ext)
        dq = comm.allreduce(ops.dot(d_ext[:n], q).reshape(1).clone())
        alpha = rho / dq
        x = x + alpha * d_ext[:n]
        r = r - alpha * q
        z = apply_m(r)
        rho_old = rho
        red = comm.allreduce(torch.stack([ops.dot(r, z), ops.dot(r, r)]).clone())
        rho = red[0:1].clone()
        beta = rho / rho_old
        d_ext[:n] = beta * d_ext[:n] + z
        hist.append(red[1:2].clone())
        its += 1
        if _stops(red[1:2], tol):
            break
    return x, torch.cat(hist), its


def cg_loop_single_reduction(ops, comm, plan, b_local, x0_local, n_iterations):
    """The single-reduction form of the same recurrence (Chronopoulos & Gear; csrc/cg1.hip is the device loop): w = A r, ONE
    all-reduce of {r.r, w.r} per iteration instead of two, the exchanged vector is r.  Same iterates in exact arithmetic; the
    rounding differs, so callers hold it to a stated tolerance, not to the bits of `cg_loop`.  history[k] = r_k . r_k."""
    import torch
    n = plan.n_local
    x = x0_local.clone()
    r_ext = torch.zeros(n + plan.n_halo, dtype=b_local.dtype, device=b_local.device)
    r_ext[:n] = x
    comm.exchange(r_ext)
    r_ext[:n] = b_local - ops.spmv(r_ext)                            # clcg.c:255-260
    p = torch.zeros_like(b_local)
    s = torch.zeros_like(b_local)
    hist, gamma_old, alpha_old = [], None, None
    for k in range(n_iterations + 1):
        comm.exchange(r_ext)                                        # boundary exchange of r
        w = ops.spmv(r_ext)
        red = comm.allreduce(torch.stack([ops.dot(r_ext[:n], r_ext[:n]), ops.dot(r_ext[:n], w)]).clone())   # the ONE reduction
        gamma, dl = red[0], red[1]
        hist.append(gamma.reshape(1).clone())
        if k == n_iterations:
            break
        if k == 0:
            beta = torch.zeros_like(gamma)
            alpha = gamma / dl
        else:
            beta = gamma / gamma_old
            alpha = gamma / (dl - beta * gamma / alpha_old)
        p = r_ext[:n] + beta * p
        s = w + beta * s
        x = x + alpha * p
        r_ext[:n] = r_ext[:n] - alpha * s
        gamma_old, alpha_old = gamma, alpha
    return x, torch.cat(hist)


# ---------------------------------------------------------------------------------------------------
# the C loop
# ---------------------------------------------------------------------------------------------------
def broadcast_unique_id(rank, group=None, device=None):
    """rank 0 creates the RCCL unique id through the C ABI; torch.distributed carries the 128 bytes."""
    import torch
    import torch.distributed as dist
    lib = _lib.load()
    buf = np.zeros(129, dtype=np.uint8)         # [128] = 1: rank 0 made an id (the broadcast runs either way)
    err = None
    if rank == 0:
        try:
            check(lib.cgamd_comm_unique_id(ptr(buf)))
            buf[128] = 1
        except Exception as e:      # noqa: BLE001 -- raised on every rank after the broadcast
            err = e
    t = torch.from_numpy(buf)
    if device is not None and dist.get_backend() == "nccl":
        t = t.to(device)
    dist.broadcast(t, src=0, group=group)
    out = t.cpu().numpy().copy()
    if out[128] != 1:
        raise err if err else RuntimeError("rank 0 could not create an RCCL unique id")
    return out[:128].copy()


class DistSolver:
    """Row-partitioned CG on this rank's GPU (csrc/dist.cpp).  All arrays are torch CUDA tensors that
    must outlive the solver; columns are plan.cols_local.

    comm="rccl": grouped ncclSend/ncclRecv + ncclAllReduce (needs `unique_id` from broadcast_unique_id).
    comm="p2p" : no RCCL -- every rank owns an uncached IPC mailbox its peers write over xGMI (collective over
                 `group` at construction: the 64-byte IPC handles and the landing offsets are all-gathered)."""

    def __init__(self, ctx, plan, indptr_local, values, dtype, unique_id=None, flags=0, comm="rccl", group=None):
        if int(flags) & _lib.HERMITIAN:     # (before anything touches a device; cgamd_dist_create refuses the flag as well)
            raise ValueError("the row-partitioned solver runs the unconjugated recurrence only: HERMITIAN is a flag of the single-GPU "
                             "Solver (Solver(..., hermitian=True))")
        import torch
        self.ctx, self.plan, self.dtype = ctx, plan, np.dtype(dtype)
        self._lib = _lib.load()
        self.mailbox = None
        peers = np.asarray(plan.peers, dtype=np.int32)
        sc = np.asarray(plan.send_counts, dtype=np.int32)
        rc = np.asarray(plan.recv_counts, dtype=np.int32)
        self._keep = (indptr_local, values, plan.cols_local, plan.send_index, peers, sc, rc)
        if comm == "p2p":
            flags |= _lib.DIST_P2P
            unique_id = None
        elif (plan.world > 1 or plan.peers) and unique_id is None:
            raise ValueError("unique_id is required when there are peers")
        idbuf = None if unique_id is None else np.ascontiguousarray(unique_id, dtype=np.uint8)
        torch.cuda.synchronize()
        h = ctypes.c_void_p()
        create_err = None
        try:
            self._create(ctx, plan, indptr_local, values, idbuf, peers, sc, rc, flags, h)
        except Exception as e:      # noqa: BLE001 -- with the peer-to-peer backend the failure is raised on every rank
            if comm != "p2p":
                raise
            create_err = e
        self.handle = h if create_err is None else None
        self.iterations = 0
        self._resident = bool(flags & _lib.DIST_RESIDENT)
        if comm == "p2p":
            self._attach_p2p(group, create_err)

    def _create(self, ctx, plan, indptr_local, values, idbuf, peers, sc, rc, flags, h):
        check(self._lib.cgamd_dist_create(
            ctx.handle, ptr(idbuf), plan.rank, plan.world, _lib.DTYPE_CODE[self.dtype], plan.n_local, plan.n_halo,
            int(plan.cols_local.numel()), ptr(values), ptr(indptr_local), ptr(plan.cols_local), len(plan.peers),
            ptr(peers) if len(peers) else None, ptr(sc) if len(sc) else None, ptr(rc) if len(rc) else None,
            ptr(plan.send_index) if plan.send_index.numel() else None, int(flags), ctypes.byref(h)))

    def _attach_p2p(self, group, create_err=None):
        """Collective over `group`.  A failure on any rank (allocation, IPC mapping) is raised on EVERY rank, so that the
        ranks keep executing the same sequence of collectives."""
        import torch.distributed as dist
        plan = self.plan
        err, handle = create_err, np.zeros(64, dtype=np.uint8)
        try:
            if err:
                raise err
            mb = ctypes.c_void_p()
            # CGAMD_DIST_RESIDENT: the slab loop's two published-d buffers (n_local + n_halo values each) live behind the halo area of
            # the same IPC allocation, so that the peers can write into their tails (include/cgamd.h: cgamd_dist_enable_resident)
            mb_values = plan.n_halo + (2 * (plan.n_local + plan.n_halo) + 256 if self._resident and (plan.peers or plan.world > 1) else 0)
            check(self._lib.cgamd_p2p_mailbox_alloc(self.ctx.handle, mb_values, _lib.DTYPE_CODE[self.dtype], ctypes.byref(mb), ptr(handle)))
            self.mailbox = mb
        except Exception as e:      # noqa: BLE001 -- reported collectively below
            err = e
        recv_off, off = {}, 0
        for peer, cnt in zip(plan.peers, plan.recv_counts):      # where each peer's entries land in MY halo area
            recv_off[int(peer)] = off
            off += int(cnt)
        mine = (None if err else handle.tobytes(), recv_off, int(plan.n_local), int(plan.n_halo))
        if plan.world > 1:
            everyone = [None] * plan.world
            dist.all_gather_object(everyone, mine, group=group)
        else:
            everyone = [mine]
        if any(e[0] is None for e in everyone):
            raise err if err else RuntimeError("peer-to-peer backend: a peer rank could not allocate its mailbox")
        try:
            if err:
                raise err
            handles = np.frombuffer(b"".join(e[0] for e in everyone), dtype=np.uint8).copy()
            dst = np.asarray([everyone[int(p)][1][plan.rank] for p in plan.peers], dtype=np.int32)
            check(self._lib.cgamd_dist_attach_p2p(self.handle, self.mailbox, ptr(handles), ptr(dst) if len(dst) else None))
            if self._resident and (plan.peers or plan.world > 1):
                nl = np.asarray([e[2] for e in everyone], dtype=np.int32)
                nh = np.asarray([e[3] for e in everyone], dtype=np.int32)
                check(self._lib.cgamd_dist_enable_resident(self.handle, int(mb_values), ptr(nl), ptr(nh)))
        except Exception as e:      # noqa: BLE001
            err = e
        if plan.world > 1:          # doubles as the barrier "every mailbox is mapped before anyone pushes"
            oks = [None] * plan.world
            dist.all_gather_object(oks, err is None, group=group)
            if not all(oks):
                raise err if err else RuntimeError("peer-to-peer backend: a peer rank could not map the mailboxes")
        elif err:
            raise err

    def p2p_error(self):
        return self._lib.cgamd_dist_p2p_error(self.handle)

    def index_codes(self):
        """distinct (column - row) offsets when this rank's SpMV reads one-byte column codes (include/cgamd.h), else 0"""
        return int(self._lib.cgamd_dist_index_codes(self.handle))

    def loop_launches(self):
        """stream operations per iteration of the loop this handle runs; 0 = the slab loop (whole calls in one launch)"""
        return int(self._lib.cgamd_dist_loop_launches(self.handle))

    def slab_plan(self):
        """what the slab loop of this handle runs on (cgamd_dist_slab_plan), as a dict: in_use, members, rows_m and steps of the largest
        member, unroll (5 / 7 / 8), budget (10 / 12 steps), value_coded, uniform, member_start (the members + 1 starts; [] when the
        loop is not in use)"""
        info = (ctypes.c_int * 8)()
        need = self._lib.cgamd_dist_slab_plan(self.handle, info, None, 0)
        if need < 0:
            raise _lib.CgAmdError(-need, "cgamd_dist_slab_plan")
        starts = (ctypes.c_int * max(need, 1))()
        if need > 0:
            assert self._lib.cgamd_dist_slab_plan(self.handle, info, starts, need) == need
        keys = ("in_use", "members", "rows_m", "steps", "unroll", "budget", "value_coded", "uniform")
        out = {k: int(v) for k, v in zip(keys, info)}
        out["member_start"] = [int(v) for v in starts[:need]]
        return out

    def comm_ranks(self):
        """ranks of the RCCL communicator, as RCCL reports them (0: no communicator)"""
        return int(self._lib.cgamd_dist_comm_ranks(self.handle))

    def set_preconditioner(self, m, group=None):
        """Preconditioned CG from the next set_rhs on.  m: None (remove), "jacobi" (1 / diag of the rank's matrix, built on the
        device), ("line", stride) (the local entries at column - row in {-stride, 0, +stride}; halo columns never count, so lines end
        at the rank's row range), ("multigrid", local_dims[, opts]) (one V-cycle of a hierarchy built from the rank's CUT matrix, its
        rows without their halo columns; local_dims is the rank's own box, `local_grid_dims`; opts as the single Solver's), "amg" or
        ("amg", opts) (the same on aggregates matched from the cut matrix: any row range) or a device tensor / buffer of n_local
        values (z = m .* r).  Collective over `group`: the C calls
        are local, so the ranks' statuses are all-gathered afterwards; if ANY rank failed, every rank removes its preconditioner and
        raises CgAmdError with the failing rank and its message -- ranks running different recurrences would wait for each
        other's sums until the peer-to-peer time-outs."""
        lib = self._lib
        if m is None:
            call = lambda: lib.cgamd_dist_set_preconditioner(self.handle, None)
        elif isinstance(m, str) and m == "jacobi":
            call = lambda: lib.cgamd_dist_set_preconditioner_jacobi(self.handle)
        elif (isinstance(m, (tuple, list)) and len(m) == 2 and isinstance(m[0], str) and m[0] == "line"
              and isinstance(m[1], (int, np.integer)) and not isinstance(m[1], bool)):
            call = lambda: lib.cgamd_dist_set_preconditioner_line(self.handle, int(m[1]))
        elif (isinstance(m, str) and m == "amg") or (isinstance(m, (tuple, list)) and len(m) == 2 and isinstance(m[0], str)
                                                     and m[0] == "amg" and isinstance(m[1], dict)):
            opts = {} if isinstance(m, str) else dict(m[1])
            if set(opts) - {"passes", "strength", "smooth_steps", "over_correction", "min_rows"}:
                raise ValueError('set_preconditioner: "amg" or ("amg", {"passes": 3, "strength": 0.25, "smooth_steps": 1, '
                                 '"over_correction": 1.6, "min_rows": 512})')
            args = (int(opts.get("passes", 0)), float(opts.get("strength", 0.0)), int(opts.get("smooth_steps", 0)),
                    float(opts.get("over_correction", 0.0)), int(opts.get("min_rows", 0)))
            call = lambda: lib.cgamd_dist_set_preconditioner_amg(self.handle, *args)
        elif (isinstance(m, (tuple, list)) and len(m) in (2, 3) and isinstance(m[0], str) and m[0] == "multigrid"
              and isinstance(m[1], (tuple, list)) and 1 <= len(m[1]) <= 3
              and all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in m[1])
              and (len(m) == 2 or isinstance(m[2], dict))):
            dims = tuple(int(v) for v in m[1]) + (1,) * (3 - len(m[1]))
            opts = dict(m[2]) if len(m) == 3 else {}
            if set(opts) - {"smooth_steps", "over_correction", "min_rows"}:
                raise ValueError('set_preconditioner: ("multigrid", (nx, ny, nz)[, {"smooth_steps": 1, "over_correction": 1.6, '
                                 '"min_rows": 512}]) with the dims of the rank\'s own box (local_grid_dims)')
            args = dims + (int(opts.get("smooth_steps", 0)), float(opts.get("over_correction", 0.0)), int(opts.get("min_rows", 0)))
            call = lambda: lib.cgamd_dist_set_preconditioner_multigrid(self.handle, *args)
        elif not isinstance(m, (str, tuple, list)) and (hasattr(m, "data_ptr") or hasattr(m, "ptr")):
            count = m.numel() if hasattr(m, "numel") else getattr(m, "size", self.plan.n_local)
            if int(count) != self.plan.n_local:
                raise ValueError(f"set_preconditioner: {int(count)} values, the rank has {self.plan.n_local} rows")
            if hasattr(m, "dtype") and hasattr(m, "data_ptr") and np.dtype(str(m.dtype).replace("torch.", "")) != self.dtype:
                raise ValueError(f"set_preconditioner: values of type {m.dtype}, the solver's is {self.dtype}")
            if hasattr(m, "is_cuda") and not m.is_cuda:
                raise ValueError("set_preconditioner: the values must be on the device")
            if hasattr(m, "is_cuda"):
                import torch
                torch.cuda.synchronize()        # torch filled the tensor on ITS stream; the library copies it on the context's
            call = lambda: lib.cgamd_dist_set_preconditioner(self.handle, ptr(m))
        else:
            raise ValueError('set_preconditioner: expected None, "jacobi", ("line", stride), ("multigrid", local_dims[, opts]), "amg", '
                             '("amg", opts) or n_local device values')
        status = call()
        mine = (int(status), lib.cgamd_last_error().decode(errors="replace") if status else "")
        if self.plan.world > 1:
            import torch.distributed as dist
            everyone = [None] * self.plan.world
            dist.all_gather_object(everyone, mine, group=group)
        else:
            everyone = [mine]
        bad = [(r, e) for r, e in enumerate(everyone) if e[0] != 0]
        if bad:
            lib.cgamd_dist_set_preconditioner(self.handle, None)     # (a failed call left this rank's earlier one in place)
            r, (code, text) = bad[0]
            raise _lib.CgAmdError(code, f"set_preconditioner failed on rank {r}: {text}")

    def mg_levels(self):
        """this rank's multigrid hierarchy in force: a list of dicts (rows, nnz, nx, ny, nz, lmax), level 0 (the cut matrix) first; []
        without one"""
        out = []
        for l in range(max(0, self._lib.cgamd_dist_mg_levels(self.handle))):
            info = (ctypes.c_longlong * 6)()
            check(self._lib.cgamd_dist_mg_level(self.handle, l, info))
            out.append({"rows": int(info[0]), "nnz": int(info[1]), "nx": int(info[2]), "ny": int(info[3]), "nz": int(info[4]),
                        "lmax": float(np.array([info[5]], dtype=np.int64).view(np.float64)[0])})
        return out

    def mg_level_matrix(self, level):
        """(indptr, indices, data) of a level of this rank's hierarchy, copied to the host (development accessor: tests)"""
        info = self.mg_levels()[level]
        ip, ix, da = np.empty(info["rows"] + 1, np.int32), np.empty(info["nnz"], np.int32), np.empty(info["nnz"], self.dtype)
        check(self._lib.cgamd_dist_mg_level_matrix(self.handle, int(level), ptr(ip), ptr(ix), ptr(da)))
        return ip, ix, da

    def mg_apply(self, r):
        """z = one V-cycle of this rank's hierarchy on r: a device tensor of n_local values in, a new one out (development
        accessor: tests)"""
        import torch
        if int(r.numel()) != self.plan.n_local or not r.is_cuda or np.dtype(str(r.dtype).replace("torch.", "")) != self.dtype:
            raise ValueError("mg_apply takes n_local device values of the solver's type")
        r = r.contiguous()
        z = torch.empty_like(r)
        torch.cuda.synchronize()        # torch filled r on ITS stream; the library reads it on the context's
        check(self._lib.cgamd_dist_mg_apply(self.handle, ptr(r), ptr(z)))
        return z

    def refresh_values(self, group=None):
        """The rank's matrix values (the borrowed tensor) were changed in place on the same pattern: the value codes and a "jacobi"
        / ("line", stride) / multigrid preconditioner follow them (cgamd_dist_refresh_values); the next call must be set_rhs.  Collective over
        `group` like set_preconditioner: the C call is local, the statuses are all-gathered; if ANY rank failed (a zero diagonal
        under the new values), every rank removes its preconditioner and raises CgAmdError with the failing rank and its message."""
        lib = self._lib
        if hasattr(self._keep[1], "is_cuda"):
            import torch
            torch.cuda.synchronize()        # torch wrote the values on ITS stream; the library reads them on the context's
        status = lib.cgamd_dist_refresh_values(self.handle)
        mine = (int(status), lib.cgamd_last_error().decode(errors="replace") if status else "")
        if self.plan.world > 1:
            import torch.distributed as dist
            everyone = [None] * self.plan.world
            dist.all_gather_object(everyone, mine, group=group)
        else:
            everyone = [mine]
        bad = [(r, e) for r, e in enumerate(everyone) if e[0] != 0]
        if bad:
            lib.cgamd_dist_set_preconditioner(self.handle, None)
            r, (code, text) = bad[0]
            raise _lib.CgAmdError(code, f"refresh_values failed on rank {r}: {text}")

    @property
    def last_refresh(self):
        """what this rank's last refresh_values did (cgamd_dist_last_refresh; ranks may differ)"""
        return int(self._lib.cgamd_dist_last_refresh(self.handle))

    def set_rhs(self, b_local, x0_local=None):
        check(self._lib.cgamd_dist_set_rhs(self.handle, ptr(b_local), ptr(x0_local)))
        self.iterations = 0

    def iterate(self, n):
        check(self._lib.cgamd_dist_iterate(self.handle, int(n)))
        self.iterations += int(n)

    @staticmethod
    def _until_args(tol, maxit, check_every):
        """ValueError before the library is touched"""
        for name, v in (("maxit", maxit), ("check_every", check_every)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"iterate_until: {name} must be an integer, got {v!r}")
            if v < 0:
                raise ValueError(f"iterate_until: {name} must be >= 0, got {v}")
        try:
            tol = float(tol)
        except (TypeError, ValueError):
            raise ValueError(f"iterate_until: tol must be a positive number, got {tol!r}") from None
        if not tol > 0.0:       # (NaN included)
            raise ValueError(f"iterate_until: tol must be > 0, got {tol}")
        return tol, int(maxit), int(check_every)

    def iterate_until(self, tol, maxit, check_every=8, group=None):
        """Up to `maxit` more iterations, stopped ON THE DEVICE in the first one whose global sqrt|r.r| fails >= tol
        (cgamd_dist_iterate_until, include/cgamd.h): x() is then the iterate of exactly that iteration and history() ends with it.
        Returns the iterations since set_rhs -- after a stop, the stopping iteration.  The call synchronises once per `check_every`
        iterations (0 = 8), never per iteration.  Collective over `group`: every rank makes the same call; the (status, iterations)
        pairs are all-gathered and CgAmdError names the first rank that failed or disagrees.  A stopped solver stays stopped until
        set_rhs: iterate raises, a further iterate_until returns the same count."""
        tol, maxit, check_every = self._until_args(tol, maxit, check_every)
        lib = self._lib
        its = ctypes.c_int(-1)
        status = lib.cgamd_dist_iterate_until(self.handle, maxit, tol, check_every, ctypes.byref(its))
        mine = (int(status), int(its.value), lib.cgamd_last_error().decode(errors="replace") if status else "")
        if self.plan.world > 1:
            import torch.distributed as dist
            everyone = [None] * self.plan.world
            dist.all_gather_object(everyone, mine, group=group)
        else:
            everyone = [mine]
        for r, (code, _, text) in enumerate(everyone):
            if code != 0:
                raise _lib.CgAmdError(code, f"iterate_until failed on rank {r}: {text}")
        for r, (_, k, _) in enumerate(everyone):
            if k != everyone[0][1]:
                raise _lib.CgAmdError(_lib.ERR_STATE, f"iterate_until: rank {r} is at iteration {k}, rank 0 at {everyone[0][1]}")
        self.iterations = int(its.value)
        return self.iterations

    def solve_until(self, b_local, x0_local=None, tol=1e-5, maxit=1000, check_every=8, group=None):
        """set_rhs, then iterate_until: solve to sqrt|r.r| < tol in at most `maxit` iterations.  Returns the iterations run."""
        tol, maxit, check_every = self._until_args(tol, maxit, check_every)
        self.set_rhs(b_local, x0_local)
        return self.iterate_until(tol, maxit, check_every, group=group)

    @property
    def iterations_done(self):
        """iterations since set_rhs as the library counts them; after a stop, the stopping iteration"""
        got = int(self._lib.cgamd_dist_iterations_done(self.handle))
        if got < 0:
            check(-got)
        return got

    def synchronize(self):
        check(self._lib.cgamd_dist_synchronize(self.handle))

    def x(self, out):
        check(self._lib.cgamd_dist_get_x(self.handle, ptr(out)))
        self.synchronize()
        return out

    def history(self):
        out = np.empty(self.iterations + 1, dtype=self.dtype)
        got = self._lib.cgamd_dist_history(self.handle, ptr(out), len(out))
        if got < 0:
            check(-got)
        return out[:got]

    def close(self):
        if getattr(self, "handle", None) and getattr(self.ctx, "handle", None):
            self._lib.cgamd_dist_destroy(self.handle)
            if getattr(self, "mailbox", None):
                self._lib.cgamd_p2p_mailbox_free(self.ctx.handle, self.mailbox)
                self.mailbox = None
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HipOps:
    """local kernels for cg_loop on torch CUDA tensors through the C ABI (cross-check of the C loop)."""

    def __init__(self, ctx, plan, indptr_local, values, dtype):
        from . import cl
        self.ctx, self.plan, self.dtype = ctx, plan, np.dtype(dtype)
        self.indptr, self.values = indptr_local, values
        self._lib = _lib.load()
        self.kern = cl.load_and_build_kernels(ctx, 1)
        self.queue = cl.CommandQueue(ctx)

    def spmv(self, v_ext):
        import torch
        p = self.plan
        # the stand-alone op takes a square system of size n_local + n_halo rows; pad the row pointers
        y = torch.zeros(p.n_local + p.n_halo, dtype=v_ext.dtype, device=v_ext.device)
        if not hasattr(self, "_ptr_ext"):
            last = self.indptr[-1:].expand(p.n_halo)
            self._ptr_ext = torch.cat([self.indptr, last]).contiguous()
        torch.cuda.synchronize()
        self.kern["spmv"](self.queue, p.n_local + p.n_halo, self.values, self._ptr_ext, p.cols_local, v_ext, y)
        self.ctx.synchronize()
        return y[:p.n_local]

    def dot(self, a, b):
        import torch
        res = torch.zeros(1, dtype=a.dtype, device=a.device)
        a, b = a.contiguous(), b.contiguous()
        torch.cuda.synchronize()
        self.kern["vdot"](self.queue, a, b, res, a.numel())
        self.ctx.synchronize()
        return res[0]


# ---------------------------------------------------------------------------------------------------
# bench.py --gpus N (N > 1): strong scaling of the N=10M system, z-slab row partition
# ---------------------------------------------------------------------------------------------------
def _cdev(dist, dev):
    """device for the small tensors of torch.distributed collectives: GPU with nccl, CPU with gloo (rehearsals)"""
    return dev if dist.get_backend() == "nccl" else "cpu"


def _all_ok(flag, dist, torch, dev):
    """logical AND of `flag` over all ranks (one all-reduce: every rank must call it the same number of times)"""
    t = torch.tensor([1.0 if flag else 0.0], device=_cdev(dist, dev))
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    return float(t.item()) == 1.0


def _run_dist(solver, b, warmup, steps, dist, torch, dev):
    """Time `steps` iterations after `warmup` untimed ones, bracketed by barrier + synchronize on both sides.
    -> (max over ranks of the wall time, every rank got through, local error text or None).
    A local failure (an exception of this rank's C loop) never skips a collective: the barriers and the final
    all-reduce run on every rank whatever happened in between, so one failing rank cannot leave the others hanging."""
    import time
    err = None
    try:
        solver.set_rhs(b, None)
        solver.iterate(warmup)
        solver.synchronize()
    except Exception as e:      # noqa: BLE001 -- reported collectively below
        err = f"{type(e).__name__}: {e}"
    dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if err is None:
        try:
            solver.iterate(steps)
            solver.synchronize()
        except Exception as e:  # noqa: BLE001
            err = f"{type(e).__name__}: {e}"
    torch.cuda.synchronize()
    dist.barrier()
    dt = time.perf_counter() - t0
    red = torch.tensor([dt, 0.0 if err is None else 1.0], dtype=torch.float64, device=_cdev(dist, dev))
    dist.all_reduce(red, op=dist.ReduceOp.MAX)
    return float(red[0].item()), float(red[1].item()) == 0.0, err


def _history_check(solver, ref_hist, entries=17):
    """(ok, text): no peer-to-peer time-out, finite history, first `entries` residuals equal to the single-GPU ones to 1e-9"""
    try:
        perr = solver.p2p_error()
        h = solver.history()
    except Exception as e:      # noqa: BLE001
        return False, f"{type(e).__name__}: {e}"
    if perr != 0:
        return False, f"peer-to-peer protocol time-out (error word {perr})"
    if not np.all(np.isfinite(h)):
        return False, "non-finite residual history"
    if ref_hist is not None:
        k = min(entries, len(ref_hist))
        if len(h) < k:
            return False, f"history has {len(h)} entries, expected >= {k}"
        dev_rel = float(np.max(np.abs(h[:k] - ref_hist[:k]) / np.abs(ref_hist[:k])))
        if not dev_rel < 1e-9:
            return False, f"residual history deviates from the single-GPU solver by {dev_rel:.3e} (> 1e-9)"
    return True, ""


DIST_MODES = ("slab", "p2p2-sr", "p2p4", "p2p4+graph", "p2p", "p2p+graph", "rccl-sr", "rccl-sr+graph", "rccl+graph", "rccl")


def bench_strong_scaling(args, pkg, ctx, torch, dist, dev, nx, ny, nz, dtype, rank, world):
    """bench.py --gpus N (N > 1): the SAME N=10M system, rows partitioned into N contiguous z-slabs.

    Candidate loops (all of them are built, validated and trialled; RCCL is always timed next to the peer-to-peer loops):
      slab        peer-to-peer, the WHOLE call in one launch per rank (csrc/slab.hip): vectors in registers, matrix streamed, halo
                  pushes, halo flags and the two rank-ordered scalar sums inside the launch
      p2p2-sr     peer-to-peer, single-reduction recurrence (csrc/cg1.hip): two launches, one scalar exchange per iteration
      rccl-sr(+graph)  the single-reduction recurrence over RCCL: one all-reduce of two scalars per iteration
      p2p4        peer-to-peer mailboxes over xGMI, FOUR launches per iteration: the halo push and the wait ride inside
                  the SpMV launch (halo read in place), the r.r all-reduce inside the aypx launch; plain launches
      p2p4+graph  the same, replayed from a hipGraph
      p2p         peer-to-peer with separate push / unpack / all-reduce launches (seven per iteration)
      p2p+graph   the same from a hipGraph
      rccl+graph  RCCL send/recv + all-reduce captured in a hipGraph
      rccl        RCCL, plain launches, exchange overlapped with the interior row blocks
    Validation before a loop may be timed: 16 iterations whose residual history must match, to 1e-9, the history of the SAME
    global system solved by the single-GPU solver, which every rank computes for itself (the whole system fits one GPU; no
    communication library is involved in the check).  The valid loops run a short trial; the fastest runs the timed
    region, AFTER which it is validated again (no protocol time-out on any rank, finite history, first residuals equal
    to the reference): a loop that fails that check is dropped and the next fastest runs the timed region instead, so
    `value` never comes from a run that went wrong.  If no C loop survives, the Python loop over torch.distributed
    drives the same HIP kernels."""
    import time
    n = nx * ny * nz
    ranges = row_ranges(n, world)
    rb, re = ranges[rank]
    indptr, cols_global, data = pkg.generators.laplace3d(ctx, nx, ny, nz, dtype=dtype, row_begin=rb, row_end=re)
    plan = build_halo_plan(cols_global, ranges, rank)
    del cols_global
    tdt = pkg.generators.torch_dtype(dtype)
    b = torch.full((plan.n_local,), 5.0, dtype=tdt, device=dev)          # main.c:44: b = (r+1)*5, x0 = 0
    torch.cuda.synchronize()
    notes, trials, rejected, solvers = [], {}, {}, {}
    skip = getattr(args, "dist_skip", "").split(",")
    have_rccl = dist.get_backend() == "nccl"
    want = [m for m in DIST_MODES if m not in skip and (have_rccl or not m.startswith("rccl"))]
    if not have_rccl:
        rejected["rccl+graph"] = rejected["rccl"] = "ranks bootstrap over gloo (they share a GPU): RCCL refuses duplicate devices"
    rccl_ranks = None

    def all_ok(flag):
        return _all_ok(flag, dist, torch, dev)

    def make(mode):
        flags = _lib.DIST_GRAPH if mode.endswith("+graph") else 0
        if "-sr" in mode:
            flags |= _lib.DIST_SINGLE_REDUCTION
        if mode == "slab":
            s = DistSolver(ctx, plan, indptr, data, dtype, flags=_lib.DIST_RESIDENT, comm="p2p")
            if s.loop_launches() != 0:      # (the flag is inert where the loop does not apply: that would time p2p4 twice)
                s.close()
                raise RuntimeError("the slab loop does not apply to this rank's slab")
            return s
        if mode.startswith("p2p"):
            if mode.startswith("p2p2"):
                pass
            elif not mode.startswith("p2p4"):
                flags |= _lib.DIST_P2P_STAGED | _lib.DIST_NO_OVERLAP
            return DistSolver(ctx, plan, indptr, data, dtype, flags=flags, comm="p2p")
        uid = broadcast_unique_id(rank, device=dev)      # collective; raises on every rank when rank 0 could not make one
        return DistSolver(ctx, plan, indptr, data, dtype, unique_id=uid, flags=flags)

    def drop(mode, solver, why):
        rejected[mode] = why
        notes.append(f"{mode}: {why}")
        if solver is not None:
            try:
                solver.close()
            except Exception:   # noqa: BLE001
                pass

    ref_hist = None
    try:    # reference history: the whole system on this rank's GPU with the single-GPU solver
        from . import cl
        ip_f, ix_f, da_f = pkg.generators.laplace3d(ctx, nx, ny, nz, dtype=dtype)
        ref = cl.Solver(ctx, n, int(ix_f.numel()), da_f, ip_f, ix_f, 1, flags=_lib.MATRIX_ON_DEVICE, dtype=dtype)
        b_f = torch.full((n,), 5.0, dtype=tdt, device=dev)
        torch.cuda.synchronize()                    # torch filled it on ITS stream; the solver reads it on the context's
        ref.set_rhs(b_f, None, on_device=True)
        ref.iterate(16)
        ref_hist = ref.history()[:, 0].copy()       # synchronises the solver's stream
        ref.close()
        del ip_f, ix_f, da_f, b_f, ref
        torch.cuda.empty_cache()
    except Exception as e:      # noqa: BLE001
        notes.append(f"single-GPU reference history unavailable: {type(e).__name__}: {e}")
    if not all_ok(ref_hist is not None):
        ref_hist = None         # every rank validates the same way or none does

    for mode in want:
        solver, err = None, None
        try:
            solver = make(mode)
        except Exception as e:  # noqa: BLE001
            err = f"{type(e).__name__}: {e}"
        if not all_ok(err is None):
            drop(mode, solver, "could not be created" + (f" ({err})" if err else " on another rank"))
            continue
        good, why = False, ""
        try:
            solver.set_rhs(b, None)
            solver.iterate(16)              # (one call of >= 16 iterations: what the slab loop takes whole)
            good, why = _history_check(solver, ref_hist, entries=17)
        except Exception as e:  # noqa: BLE001
            why = f"{type(e).__name__}: {e}"
        if not all_ok(good):
            drop(mode, solver, "validation run failed" + (f": {why}" if why else " on another rank"))
            continue
        t, ok, err = _run_dist(solver, b, 5, 30, dist, torch, dev)
        if not ok:
            drop(mode, solver, "trial run failed" + (f": {err}" if err else " on another rank"))
            continue
        trials[mode] = 30.0 / t
        solvers[mode] = solver
        if mode.startswith("rccl") and rccl_ranks is None:
            rccl_ranks = solver.comm_ranks()

    mode, dt, hist, index_codes_seen = None, None, None, 0
    for cand in sorted(trials, key=lambda m: -trials[m]):
        solver = solvers[cand]
        t, ok, err = _run_dist(solver, b, args.warmup, args.steps, dist, torch, dev)
        good, why = (False, err or "another rank failed") if not ok else _history_check(solver, ref_hist)
        if all_ok(good):
            mode, dt, hist = cand, t, solver.history()
            index_codes_seen = solver.index_codes()
            break
        rejected[cand] = "timed run failed its check" + (f": {why}" if why else " on another rank")
        notes.append(f"{cand}: {rejected[cand]}; falling through to the next candidate")
    for solver in solvers.values():
        try:
            solver.close()
        except Exception:       # noqa: BLE001
            pass
    validated = mode is not None
    if mode is None:   # still the HIP kernels through the C ABI, only the loop moves to Python
        notes.append("no C loop available; Python loop over torch.distributed")
        mode = "python-loop"
        ops = HipOps(ctx, plan, indptr, data, dtype)
        comm = TorchComm(plan)
        _, h8 = cg_loop(ops, comm, plan, b, torch.zeros_like(b), 8)
        if ref_hist is not None:
            dev8 = float(np.max(np.abs(h8.cpu().numpy() - ref_hist[:9]) / np.abs(ref_hist[:9])))
            validated = dev8 < 1e-9
            notes.append(f"python loop: max rel deviation from the single-GPU residual history over 8 iterations = {dev8:.3e}"
                         + ("" if validated else "  -- RESULT NOT VALIDATED"))
        dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, h = cg_loop(ops, comm, plan, b, torch.zeros_like(b), args.steps)
        torch.cuda.synchronize()
        dist.barrier()
        tmax = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=_cdev(dist, dev))
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax.item())
        hist = h.cpu().numpy()
    nnz_total = pkg.generators.laplace3d_nnz(nx, ny, nz)
    V = np.dtype(dtype).itemsize
    # what the ranks' kernels move per iteration (all ranks): one index byte per non-zero where the column codes apply; vector passes
    # of the loop that ran -- the slab loop keeps x, r, q in registers: it writes d once and gathers the off-member entries
    coded = index_codes_seen > 0
    passes = {"slab": 2, "p2p2-sr": 11, "rccl-sr": 11, "rccl-sr+graph": 11, "p2p4": 10, "p2p4+graph": 10}.get(mode, 11)
    iter_bytes = nnz_total * (V + (1 if coded else 4)) + (n + 1) * 4 + passes * n * V
    iter_bytes_csr = nnz_total * (V + 4) + (n + 1) * 4 + 14 * n * V
    it_s = args.steps / dt
    comm_desc = ("peer-to-peer mailboxes over xGMI (direct halo writes + rank-ordered scalar sums), one launch per call (slab loop)" if mode == "slab"
                 else "peer-to-peer mailboxes over xGMI (direct halo writes + rank-ordered scalar sums)"
                 + (", 4 launches/iteration" if mode.startswith("p2p4") else ", single-reduction recurrence, 2 launches/iteration" if mode.startswith("p2p2") else "")
                 if mode.startswith("p2p") else "RCCL send/recv + " + ("1 all-reduce of two scalars" if "-sr" in mode else "2 scalar all-reduces") + " per iteration")
    return {
        "metric": "CG iterations/sec + SpMV effective HBM GB/s (% of 8 TB/s peak), N=10M CSR",
        "value": it_s, "unit": "CG iterations/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": dt * 1e3 / args.steps, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
        "dtype": args.dtype, "data": "synthetic",
        "config": {"workload": f"3D 7-pt Laplacian {nx}x{ny}x{nz} CSR, N={n}, nnz={nnz_total}, {args.dtype}, 1 RHS, b=5, "
                               f"x0=0, fixed-iteration CG, rows partitioned in {world} contiguous z-slabs, "
                               f"halo {plan.n_halo} entries/rank, {comm_desc}",
                   "rows": n, "nnz": nnz_total, "parallelism": f"row-partition x{world} ({mode})"},
        "cg_iter_moved_bytes": iter_bytes, "cg_iter_gbs": iter_bytes * it_s / 1e9,
        "cg_iter_pct_of_aggregate_hbm_peak": 100.0 * iter_bytes * it_s / 1e9 / (8000.0 * world),
        "effective_csr": {"note": "reference CSR byte model (SURVEY 8d), an effective rate, not a fraction of the peak",
                          "cg_iter_bytes": iter_bytes_csr, "cg_iter_gbs": iter_bytes_csr * it_s / 1e9},
        "residual_check": {"delta_0": float(abs(hist[0])), "delta_last": float(abs(hist[-1])),
                           "iterations": int(len(hist) - 1)},
        "roofline": {"bound": "hbm", "kernel": "whole CG iteration (all ranks)", "achieved": iter_bytes * it_s / 1e9,
                     "peak": 8000.0 * world, "unit": "GB/s", "frac": iter_bytes * it_s / 1e9 / (8000.0 * world),
                     "traffic": None},
        "backend": mode, "backend_validated": bool(validated), "backend_rejected": rejected,
        "loop_trials_it_per_s": trials, "rccl_ranks": rccl_ranks, "notes": notes,
    }
