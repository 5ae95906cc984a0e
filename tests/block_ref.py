"""Block CG on the host (numpy): the residual-orthonormalised recurrence of include/cgamd.h "Block CG" (O'Leary's block CG in
Dubrulle's BCGrQ form), restated independently of csrc/block_cg.hip, for tests/test_block_ref.py (against separate CG solves) and the
GPU tests (tests/test_gpu_block_kernels.py bit for bit, tests/test_gpu_block.py).

The handle's vectors carry the block: x = X, r = Q (R = Q xi), d = P, q = A P; blocks here are (s, n) arrays, column j of the block
in row j, in the value type.  The s x s matrices are float64 (Python floats: IEEE double, one rounding per operation, math.sqrt
correctly rounded), each rounded ONCE to the value type before the vectors use it.

    set_rhs      R0 = B - A X0; C = R0^T R0 = L L^T; xi = L^T; Q = R0 xi^-1; P = Q; delta_0[j] = |xi e_j|^2
    iteration    G = P^T (A P) = L L^T; alpha = G^-1; M = alpha xi
                 X += P M; W = Q - (A P) alpha; C = W^T W = L L^T; tau = L^T; xi <- tau xi; delta_k[j] = |xi e_j|^2
                 Q = W tau^-1; P = Q + P tau^T

Orders (what "bit for bit" rests on):
    Gram partials   grid = gram_grid(n) work-groups of 256 threads; thread t of all adds, in float64, the products of its rows
                    t, t + 256 grid, ... in that order (acc = acc + a * b: product rounded, then the sum); cg_step_ref.block_sum per
                    work-group.  Entry p = j (j + 1) / 2 + i holds a_i . b_j, i <= j; layout [p][grid]
    their sum       lane l of one wave adds partials l, l + 64, ...; then the wave tree
    Cholesky        left-looking by columns: v = C_kk - sum_m<k L_km^2 (m ascending, one subtraction per term), the pivot rule,
                    L_kk = sqrt(v), L_ik = (C_ik - sum_m<k L_im L_km) / L_kk
    L^-1            X_jj = 1 / L_jj; X_ij = -(L_ij X_jj + ... + L_i,i-1 X_i-1,j) / L_ii
    alpha           alpha_ij = sum_m>=max(i,j) X_mi X_mj;  M_ij = sum_m<=j alpha_im xi_mj;  (tau xi)_ij = sum_i<=m<=j tau_im xi_mj;
                    delta_j = sum_i<=j xi_ij^2 -- every sum from its first product on, m ascending
    vectors         x_j = (..((x_j + p_0 M_0j) + p_1 M_1j) ..);  w_j = (..((q_j - ap_0 alpha_0j) - ap_1 alpha_1j) ..);
                    qn_j = (..(w_0 ti_0j + w_1 ti_1j) .. + w_j ti_jj);  pn_j = (..((qn_j + p_j tau_jj) + p_j+1 tau_j,j+1) ..)
A pivot v of a matrix C fails when not v > s eps_value max_j C_jj (eps_value 2^-23 / 2^-52); the pivot ratio is v / max_j C_jj."""
import math

import numpy as np

import cg_step_ref as S

MAX_BLOCK = 16
GRAM_GRID_MAX = 512
EPS = {np.dtype(np.float32): 2.0 ** -23, np.dtype(np.float64): 2.0 ** -52}
RUNNING, G_FAILED, W_FAILED, NAN = 0, 1, 2, 3


def pairs(s):
    return [(i, j) for j in range(s) for i in range(j + 1)]


def gram_grid(n):
    return max(1, min(-(-n // 256), GRAM_GRID_MAX))


def gram_partials(a, b, grid=None):
    """(s, n) x (s, n) in the value type -> float64 [pairs][grid]"""
    s, n = a.shape
    G = grid or gram_grid(n)
    T = G * 256
    ii = np.array([p[0] for p in pairs(s)]), np.array([p[1] for p in pairs(s)])
    J = -(-n // T)
    a64 = np.zeros((s, J * T)); a64[:, :n] = a
    b64 = np.zeros((s, J * T)); b64[:, :n] = b
    acc = np.zeros((len(ii[0]), T))
    for k in range(J):
        sl = slice(k * T, (k + 1) * T)
        acc = acc + a64[ii[0], sl] * b64[ii[1], sl]
    return S.block_sum(acc.reshape(-1, 256)).reshape(-1, G)


def sum_partials(p):
    """[pairs][grid] -> [pairs]: lane-strided, then the wave tree"""
    P, G = p.shape
    J = -(-G // 64)
    pad = np.zeros((P, J * 64)); pad[:, :G] = p
    acc = np.zeros((P, 64))
    for k in range(J):
        acc = acc + pad[:, k * 64:(k + 1) * 64]
    return S.block_sum(acc)


def sym(v, s):
    C = [[0.0] * s for _ in range(s)]
    for p, (i, j) in enumerate(pairs(s)):
        C[i][j] = C[j][i] = float(v[p])
    return C


def chol(C, s, eps):
    """(L, status, ratio): status 0 fine, 1 a pivot failed the rule, 3 NaN; ratio = the smallest pivot ratio seen (inf: none)"""
    L = [[0.0] * s for _ in range(s)]
    maxd = C[0][0]
    for k in range(1, s):
        maxd = C[k][k] if C[k][k] > maxd else maxd
    ratio = math.inf
    for k in range(s):
        if C[k][k] != C[k][k]:
            return L, NAN, ratio
    thr = s * eps * maxd
    for k in range(s):
        v = C[k][k]
        for m in range(k):
            v = v - L[k][m] * L[k][m]
        if v != v:
            return L, NAN, ratio
        if not v > thr:
            with np.errstate(all="ignore"):
                ratio = min(ratio, float(np.float64(v) / np.float64(maxd)))
            return L, 1, ratio
        ratio = min(ratio, v / maxd)
        L[k][k] = math.sqrt(v)
        for i in range(k + 1, s):
            w = C[i][k]
            for m in range(k):
                w = w - L[i][m] * L[k][m]
            L[i][k] = w / L[k][k]
    return L, 0, ratio


def linv(L, s):
    X = [[0.0] * s for _ in range(s)]
    for j in range(s):
        X[j][j] = 1.0 / L[j][j]
        for i in range(j + 1, s):
            acc = L[i][j] * X[j][j]
            for m in range(j + 1, i):
                acc = acc + L[i][m] * X[m][j]
            X[i][j] = -acc / L[i][i]
    return X


def small1(gv, xi, s, eps):
    """from the summed entries of P^T A P and xi: dict(G, status, ratio[, alpha, M])"""
    G = sym(gv, s)
    L, st, ratio = chol(G, s, eps)
    out = {"G": np.array(G), "status": st if st != 1 else G_FAILED, "ratio": ratio}
    if st:
        return out
    X = linv(L, s)
    al = [[0.0] * s for _ in range(s)]
    for i in range(s):
        for j in range(s):
            m0 = max(i, j)
            acc = X[m0][i] * X[m0][j]
            for m in range(m0 + 1, s):
                acc = acc + X[m][i] * X[m][j]
            al[i][j] = acc
    M = [[0.0] * s for _ in range(s)]
    for i in range(s):
        for j in range(s):
            acc = al[i][0] * xi[0][j]
            for m in range(1, j + 1):
                acc = acc + al[i][m] * xi[m][j]
            M[i][j] = acc
    out["alpha"], out["M"] = np.array(al), np.array(M)
    return out


def small2(cv, xi, s, eps):
    """from the summed entries of W^T W and xi (None at set_rhs: the identity): dict(C, status, ratio[, tau, tau_inv, xi, delta])"""
    C = sym(cv, s)
    L, st, ratio = chol(C, s, eps)
    out = {"C": np.array(C), "status": st if st != 1 else W_FAILED, "ratio": ratio}
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
    delta = []
    for j in range(s):
        acc = nx[0][j] * nx[0][j]
        for i in range(1, j + 1):
            acc = acc + nx[i][j] * nx[i][j]
        delta.append(acc)
    out.update(tau=np.array(tau), tau_inv=np.array(ti), xi=np.array(nx), delta=np.array(delta))
    return out


# ---- the vector steps, in the value type, one rounding per operation ------------------------------------------------------------------
def update_xw(P, AP, X, Q, M, al):
    """X += P M, W = Q - AP alpha (M, al: (s, s) in the value type).  Returns (X, W)"""
    s = P.shape[0]
    nX, W = np.empty_like(X), np.empty_like(Q)
    with np.errstate(all="ignore"):
        for j in range(s):
            a, w = X[j], Q[j]
            for i in range(s):
                a = a + P[i] * M[i, j]
                w = w - AP[i] * al[i, j]
            nX[j], W[j] = a, w
    return nX, W


def update_qp(W, P, ti, tau, init=False):
    """Q = W tau^-1, P = Q + P tau^T (init: P = Q); ti, tau: upper triangular (s, s) in the value type.  Returns (Q, P)"""
    s = W.shape[0]
    Q, nP = np.empty_like(W), np.empty_like(P)
    with np.errstate(all="ignore"):
        for j in range(s):
            a = W[0] * ti[0, j]
            for i in range(1, j + 1):
                a = a + W[i] * ti[i, j]
            Q[j] = a
            if not init:
                for i in range(j, s):
                    a = a + P[i] * tau[j, i]
            nP[j] = a
    return Q, nP


def bcg(A, B, tol=None, maxit=10, dtype=None, X0=None, grid=None):
    """Block CG on the columns of B (n, s) in `dtype`.  tol: None (run maxit iterations) or the absolute tolerances per column (a
    scalar or s values): all columns stop in the first iteration in which every sqrt|delta_k[j]| is not >= tol[j].  Returns a dict:
    X (n, s), history (its + 1, s) in dtype, iterations, status / event (the iteration of a breakdown), min_ratio, and the last
    xi, G, alpha, tau (float64)."""
    dtype = np.dtype(dtype or B.dtype)
    eps = EPS[dtype]
    A = A.astype(dtype)
    Bt = np.ascontiguousarray(B.T.astype(dtype))
    s, n = Bt.shape
    X = np.zeros_like(Bt) if X0 is None else np.ascontiguousarray(X0.T.astype(dtype))
    tl = None if tol is None else np.broadcast_to(np.asarray(tol, dtype=np.float64), (s,))
    spmm = lambda V: np.ascontiguousarray((A @ V.T).T.astype(dtype))
    R = Bt - spmm(X)
    out = {"status": RUNNING, "event": 0, "min_ratio": math.inf, "iterations": 0}
    st = small2(sum_partials(gram_partials(R, R, grid)), None, s, eps)
    out["min_ratio"] = min(out["min_ratio"], st["ratio"])
    hist = []
    if st["status"]:
        # (row 0 is then the diagonal of C: the squared norms of the residual columns themselves)
        out.update(status=st["status"], X=X.T.copy(), history=np.diag(st["C"]).astype(dtype)[None, :])
        return out
    xi = st["xi"].tolist()
    Q, P = update_qp(R, R, st["tau_inv"].astype(dtype), st["tau"].astype(dtype), init=True)
    hist.append(st["delta"].astype(dtype))
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
        s2 = small2(sum_partials(gram_partials(W, W, grid)), xi, s, eps)
        out["min_ratio"] = min(out["min_ratio"], s2["ratio"])
        if s2["status"]:
            out.update(status=s2["status"], event=k)
            break
        xi = s2["xi"].tolist()
        out["tau"] = s2["tau"]
        hist.append(s2["delta"].astype(dtype))
        Q, P = update_qp(W, P, s2["tau_inv"].astype(dtype), s2["tau"].astype(dtype))
        if tl is not None and not np.any(np.sqrt(np.abs(hist[-1].astype(np.float64))) >= tl):
            break
    out.update(X=X.T.copy(), history=np.array(hist), iterations=k, xi=np.array(xi))
    return out
