"""Preconditioned block CG on the host (numpy): the recurrence of include/cgamd.h "Preconditioned block CG" -- BCGrQ carried in the
M^-1 inner product, R = Q xi with Q^T M^-1 Q = I -- restated independently of csrc/block_pcg.hip, for tests/test_block_pcg_ref.py
(against separate PCG solves) and the GPU tests (tests/test_gpu_block_pcg_kernels.py bit for bit, tests/test_gpu_block_pcg.py).

What block CG and its preconditioned form share is block_ref's: the Gram partials and their sum, the Cholesky, L^-1, the G step
(small1) and the x / w update.  Restated here: the weighted Gram, the W step and the q / p update with Z.

    set_rhs      R0 = B - A X0; Z0 = M^-1 R0; C = R0^T Z0 = L L^T; xi = L^T; Q = R0 xi^-1; P = Z0 xi^-1; delta_0[j] = (R0^T R0)_jj
    iteration    G = P^T (A P) = L L^T; alpha = G^-1; M = alpha xi;  X += P M; W = Q - (A P) alpha
                 Z = M^-1 W; D = W^T W; delta_k[j] = (xi e_j)^T D (xi e_j) with the OLD xi (R_k+1 = W xi_k)
                 C = W^T Z = L L^T; tau = L^T; xi <- tau xi;  Q = W tau^-1; P = Z tau^-1 + P tau^T

Orders beyond block_ref's:
    weighted Gram   entry (i <= j) = w_i . (m w_j): m w_j rounded once in the value type, then gram_partials' order
    delta_k[j]      t_i = sum_m<=j D_im xi_mj (i <= j), then sum_i<=j xi_ij t_i, every sum from its first product on, ascending; at
                    set_rhs (xi = I) the diagonal entry D_jj itself
    vectors         qn_j = (..(w_0 ti_0j + w_1 ti_1j) .. + w_j ti_jj), y_j the same over z_k;
                    pn_j = (..((y_j + p_j tau_jj) + p_j+1 tau_j,j+1) ..); z_k = m w_k rounded once for a diagonal M
The history row is written before C is factored; a pivot of C = W^T Z failing block_ref's rule is status 2 (W_FAILED).
M^-1 is a callable on (s, n) blocks in the value type -- anything -- or a diagonal: an array m in the value type, z = m * w."""
import math

import numpy as np

import block_ref as B
from block_ref import chol, gram_partials, linv, small1, sum_partials, update_xw  # noqa: F401  (the shared steps, as the issue lists them)


def gram_weighted_partials(W, m, grid=None):
    """(s, n) and (n,) in the value type -> float64 [pairs][grid] of w_i . (m w_j)"""
    with np.errstate(all="ignore"):
        return gram_partials(W, (m[None, :] * W).astype(W.dtype), grid)


def small_w(dv, cv, xi, s, eps):
    """the W step from the summed entries of W^T W (dv) and W^T Z (cv) and the old xi (None at set_rhs: the identity):
    dict(D, C, delta, status, ratio[, tau, tau_inv, xi])"""
    D, C = B.sym(dv, s), B.sym(cv, s)
    delta = []
    for j in range(s):
        if xi is None:
            delta.append(D[j][j])
            continue
        acc = 0.0
        for i in range(j + 1):
            t = D[i][0] * xi[0][j]
            for m in range(1, j + 1):
                t = t + D[i][m] * xi[m][j]
            acc = xi[0][j] * t if i == 0 else acc + xi[i][j] * t
        delta.append(acc)
    L, st, ratio = chol(C, s, eps)
    out = {"D": np.array(D), "C": np.array(C), "delta": np.array(delta), "status": st if st != 1 else B.W_FAILED, "ratio": ratio}
    if st:
        return out
    X = linv(L, s)
    tau = [[L[j][i] for j in range(s)] for i in range(s)]
    ti = [[X[j][i] for j in range(s)] for i in range(s)]
    if xi is None:
        nx = tau
    else:
        nx = [[0.0] * s for _ in range(s)]
        for i in range(s):
            for j in range(i, s):
                acc = tau[i][i] * xi[i][j]
                for m in range(i + 1, j + 1):
                    acc = acc + tau[i][m] * xi[m][j]
                nx[i][j] = acc
    out.update(tau=np.array(tau), tau_inv=np.array(ti), xi=np.array(nx))
    return out


def update_qp_z(W, P, Z, ti, tau, init=False, m=None):
    """Q = W tau^-1, P = Z tau^-1 + P tau^T (init: P = Z tau^-1); Z the block, or None and z_k = m w_k rounded once.  Returns (Q, P)"""
    s = W.shape[0]
    Q, nP = np.empty_like(W), np.empty_like(P)
    with np.errstate(all="ignore"):
        if Z is None:
            Z = (m[None, :] * W).astype(W.dtype)
        for j in range(s):
            a, y = W[0] * ti[0, j], Z[0] * ti[0, j]
            for i in range(1, j + 1):
                a = a + W[i] * ti[i, j]
                y = y + Z[i] * ti[i, j]
            Q[j] = a
            if not init:
                for i in range(j, s):
                    y = y + P[i] * tau[j, i]
            nP[j] = y
    return Q, nP


def bpcg(A, Bm, M, tol=None, maxit=10, dtype=None, X0=None, grid=None, spmm=None):
    """Preconditioned block CG on the columns of Bm (n, s) in `dtype`.  M: an array (the diagonal of M^-1 in dtype: z = m * w, never
    stored as a block) or a callable Z = M(W) on (s, n) blocks in dtype.  tol, maxit, X0, grid as block_ref.bcg; spmm: the product
    on (s, n) blocks where it is not A @.  Returns block_ref.bcg's dict (history: r.r per column)."""
    dtype = np.dtype(dtype or Bm.dtype)
    eps = B.EPS[dtype]
    Bt = np.ascontiguousarray(Bm.T.astype(dtype))
    s, n = Bt.shape
    X = np.zeros_like(Bt) if X0 is None else np.ascontiguousarray(X0.T.astype(dtype))
    tl = None if tol is None else np.broadcast_to(np.asarray(tol, dtype=np.float64), (s,))
    if spmm is None:
        Ad = A.astype(dtype)
        spmm = lambda V: np.ascontiguousarray((Ad @ V.T).T.astype(dtype))
    diag = None if callable(M) else np.ascontiguousarray(np.asarray(M).reshape(-1).astype(dtype))

    def wz(W):
        """(Z or None, the summed entries of W^T Z)"""
        if diag is not None:
            return None, sum_partials(gram_weighted_partials(W, diag, grid))
        Z = np.ascontiguousarray(M(W)).astype(dtype)
        return Z, sum_partials(gram_partials(W, Z, grid))

    R = Bt - spmm(X)
    out = {"status": B.RUNNING, "event": 0, "min_ratio": math.inf, "iterations": 0}
    Z, cv = wz(R)
    st = small_w(sum_partials(gram_partials(R, R, grid)), cv, None, s, eps)
    out["min_ratio"] = min(out["min_ratio"], st["ratio"])
    hist = [st["delta"].astype(dtype)]
    if st["status"]:
        out.update(status=st["status"], X=X.T.copy(), history=np.array(hist))
        return out
    xi = st["xi"].tolist()
    Q, P = update_qp_z(R, R, Z, st["tau_inv"].astype(dtype), st["tau"].astype(dtype), init=True, m=diag)
    k = 0
    while k < maxit:
        AP = spmm(P)
        s1 = small1(sum_partials(gram_partials(P, AP, grid)), xi, s, eps)
        out["min_ratio"] = min(out["min_ratio"], s1["ratio"])
        out["G"] = s1["G"]
        if s1["status"]:
            out.update(status=s1["status"], event=k + 1)
            break
        out["alpha"] = s1["alpha"]
        k += 1
        X, W = update_xw(P, AP, X, Q, s1["M"].astype(dtype), s1["alpha"].astype(dtype))
        Z, cv = wz(W)
        s2 = small_w(sum_partials(gram_partials(W, W, grid)), cv, xi, s, eps)
        out["min_ratio"] = min(out["min_ratio"], s2["ratio"])
        hist.append(s2["delta"].astype(dtype))
        if s2["status"]:
            out.update(status=s2["status"], event=k)
            break
        xi = s2["xi"].tolist()
        out["tau"] = s2["tau"]
        Q, P = update_qp_z(W, P, Z, s2["tau_inv"].astype(dtype), s2["tau"].astype(dtype), m=diag)
        if tl is not None and not np.any(np.sqrt(np.abs(hist[-1].astype(np.float64))) >= tl):
            break
    out.update(X=X.T.copy(), history=np.array(hist), iterations=k, xi=np.array(xi), Q=Q, P=P)
    return out
