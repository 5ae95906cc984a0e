"""Multi-shift CG on the host (numpy): the recurrence of include/cgamd.h "Multi-shift CG" in its RATIO form, restated independently of
csrc/shifts.hip, for tests/test_shift_ref.py (against separate CG solves) and the GPU tests (tests/test_gpu_shifts.py,
tests/test_gpu_shift_kernel.py).

Seed, the handle's unconjugated (CO)CG:   q = A d; alpha = rho / d.q; x += alpha d; r -= alpha q; beta = rho' / rho; d = r + beta d
Shift j (theta = zeta_k / zeta_{k-1}; at the start theta = zeta = 1, x_j = 0, d_j = b, alpha_{-1} = 1, beta_{-1} = 0):
    theta' = alpha_{k-1} / (alpha_k beta_{k-1} (1 - theta) + alpha_{k-1} (1 + sigma_j alpha_k))
    zeta' = zeta theta'; alpha_j = alpha_k theta'; beta_j = beta_k theta' theta'
    x_j += alpha_j d_j; d_j = zeta' r_{k+1} + beta_j d_j
Scalars in float64 / complex128 from alpha_k, beta_k as rounded to the value type; alpha_j, beta_j, zeta' rounded once to the value
type before the vectors use them.  The vectors here are plain numpy arithmetic in `dtype`; update_bits is the type-true form of the
vector step (one rounding per operation, complex products by components) that the kernel test compares bit for bit."""
import numpy as np
import scipy.sparse as sp

import cg_step_ref as S


def acc_type(dtype):
    return np.complex128 if np.dtype(dtype).kind == "c" else np.float64


def laplace2d(nx, ny):
    """the 5-point Laplacian on an nx x ny grid, x fastest: 4 on the diagonal, -1 to the four neighbours"""
    ex = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(nx, nx))
    ey = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(ny, ny))
    A = (sp.kron(sp.eye(ny), ex) + sp.kron(ey, sp.eye(nx))).tocsr()
    A.sort_indices()
    return A


def shifted_laplace2d(nx, ny, shift):
    """L - shift I: complex symmetric (not Hermitian) for a complex shift, the reference's local_rect operator in the interior"""
    A = (laplace2d(nx, ny).astype(np.complex128) - shift * sp.eye(nx * ny)).tocsr()
    A.sort_indices()
    return A


def dot(a, b):
    return np.sum(a * b)        # unconjugated


def cg(A, b, iterations):
    """the seed recurrence alone, in the type of b: (x, history) with history[k] = r_k . r_k"""
    x, r = np.zeros_like(b), b.copy()
    d, rho = r.copy(), dot(r, r)
    hist = [rho]
    with np.errstate(all="ignore"):
        for _ in range(iterations):
            q = A @ d
            al = rho / dot(d, q)
            x = x + al * d
            r = r - al * q
            rn = dot(r, r)
            be = rn / rho
            d = r + be * d
            rho = rn
            hist.append(rho)
    return x, np.array(hist)


def theta_step(al, ap, bp, th, sigma):
    """theta' from alpha_k, alpha_{k-1}, beta_{k-1}, theta and sigma (accumulator type)"""
    return ap / (al * bp * (1 - th) + ap * (1 + sigma * al))


def mscg(A, b, sigmas, iterations, dtype=None):
    """the seed and every shifted system, vectors in `dtype` (default: the type of b).  Returns a dict: x (n), history (its + 1),
    xs (S, n), zeta (its + 1, S) and theta (S) in the accumulator type, alpha_s / beta_s (S) of the last iteration in dtype"""
    dtype = np.dtype(dtype or b.dtype)
    ct = acc_type(dtype)
    A = A.astype(dtype)
    b = b.astype(dtype)
    sig = np.asarray(sigmas).astype(dtype).astype(ct)       # as the handle receives them
    nS = sig.size
    x, r = np.zeros_like(b), b.copy()
    d, rho = r.copy(), dot(r, r)
    hist = [rho]
    xs = [np.zeros_like(b) for _ in range(nS)]
    ds = [b.copy() for _ in range(nS)]
    th, ze = np.ones(nS, ct), np.ones(nS, ct)
    ap, bp = ct(1), ct(0)
    zh = [ze.copy()]
    aj, bj = np.zeros(nS, dtype), np.zeros(nS, dtype)
    with np.errstate(all="ignore"):
        for _ in range(iterations):
            q = A @ d
            al = dtype.type(rho / dot(d, q))
            x = x + al * d
            r = r - al * q
            rn = dtype.type(dot(r, r))
            be = dtype.type(rn / rho)
            for j in range(nS):
                tn = theta_step(ct(al), ap, bp, th[j], sig[j])
                ze[j] = ze[j] * tn
                th[j] = tn
                aj[j] = dtype.type(ct(al) * tn)
                bj[j] = dtype.type(ct(be) * tn * tn)
                xs[j] = xs[j] + aj[j] * ds[j]
                ds[j] = dtype.type(ze[j]) * r + bj[j] * ds[j]
            d = r + be * d
            rho, ap, bp = rn, ct(al), ct(be)
            hist.append(rho)
            zh.append(ze.copy())
    return {"x": x, "history": np.array(hist), "xs": np.array(xs), "zeta": np.array(zh), "theta": th, "alpha_s": aj, "beta_s": bj}


def update_bits(r, xs, ds, al, be, ze):
    """the vector step in the value type, one rounding per operation (cg_step_ref.Ops: complex products by components):
    xs_j = vadd(xs_j, vmul(al_j, ds_j)); ds_j = vadd(vmul(ze_j, r), vmul(be_j, ds_j)).  r: (nrhs, n); xs, ds: (S, nrhs, n);
    al, be, ze: (S, nrhs).  Returns the new (xs, ds)"""
    ops = S.Ops(r.dtype)
    nx, nd = np.empty_like(xs), np.empty_like(ds)
    for j in range(xs.shape[0]):
        nx[j] = ops.axpy(xs[j], al[j], ds[j])
        zr = ops.mr(np.repeat(ze[j][:, None], r.shape[1], axis=1), r)
        nd[j] = ops.axpy(zr, be[j], ds[j])
    return nx, nd
