"""Host restatement of the recurrence CGAMD_HERMITIAN handles run (csrc/hermitian.hip), in complex128, and the Hermitian test systems.

CG for A = A^H positive definite with <a, b> = sum conj(a_i) b_i (numpy.vdot):

    r = b - A x0 ; z = m .* r (z = r without m) ; d = z ; rho = Re(r^H z) ; delta_0 = r^H r
    q = A d ; alpha = rho / Re(d^H q) ; x += alpha d ; r -= alpha q ; z = m .* r
    rho' = Re(r^H z) ; delta_k = r^H r ; beta = rho' / rho ; d = z + beta d

alpha and beta are real; the history is delta_k = r_k^H r_k whether or not a diagonal m is given.  With `tol` the run stops in the
first iteration whose sqrt(delta_k) fails >= tol (cgamd_solver_iterate_until's rule)."""
import numpy as np
import scipy.sparse as sp


def magnetic(nx, ny, flux, shift):
    """5-point "magnetic" Laplacian on an nx x ny grid numbered x fastest: diagonal 4 + shift, x couplings -1, y couplings
    -exp(+-2 pi i flux i) at column i.  Hermitian, not symmetric (flux not a multiple of 1/2), positive definite for shift > 0.
    scipy CSR, complex128, sorted columns."""
    n = nx * ny
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="xy")
    at = (j * nx + i).ravel()
    i, j = i.ravel(), j.ravel()
    rows, cols, vals = [at], [at], [np.full(n, 4.0 + shift, dtype=complex)]
    east = i + 1 < nx
    rows += [at[east], at[east] + 1]
    cols += [at[east] + 1, at[east]]
    vals += [np.full(east.sum(), -1.0 + 0j), np.full(east.sum(), -1.0 + 0j)]
    north = j + 1 < ny
    # the phase of column i from flux * i reduced to [0, 1) and folded onto [0, 1/2], so that equal phases are equal bit for bit and
    # conjugate ones exact conjugates: A is exactly Hermitian and has the few distinct values it has in exact arithmetic
    # (flux 0.1: 11, which the value codes of the SpMV take)
    frac = np.round((flux * i[north]) % 1.0, 12) % 1.0
    low = frac <= 0.5
    base = np.round(np.exp(2j * np.pi * np.where(low, frac, np.round(1.0 - frac, 12))), 15)
    ph = np.where(low, base, np.conj(base)) + 0.0
    rows += [at[north], at[north] + nx]
    cols += [at[north] + nx, at[north]]
    vals += [-ph + 0.0, -np.conj(ph) + 0.0]       # (+ 0.0: no negative zeros, which a bitwise count of the values would tell apart)
    A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    A.sort_indices()
    return A


def chain(n, diag=2.5, phase=0.3):
    """Hermitian tridiagonal chain: A[i][i] = diag, A[i][i + 1] = -exp(i phase), A[i + 1][i] = -exp(-i phase)"""
    up = np.full(n - 1, -np.exp(1j * phase))
    A = sp.diags([np.conj(up), np.full(n, diag + 0j), up], [-1, 0, 1], format="csr")
    A.sort_indices()
    return A


def cg(A, b, iters, m=None, x0=None, tol=None):
    """-> dict(x, history (its + 1 real values), alpha, beta (its values each), its).  iters: the cap.  m: the diagonal that
    multiplies r (1 / diag(A) for Jacobi), real and positive."""
    A = sp.csr_matrix(A).astype(np.complex128)
    b = np.asarray(b, dtype=np.complex128)
    x = np.zeros_like(b) if x0 is None else np.array(x0, dtype=np.complex128)
    r = b - A @ x
    z = r if m is None else np.asarray(m) * r
    d = z.copy()
    rho = np.vdot(r, z).real
    hist, alphas, betas = [np.vdot(r, r).real], [], []
    its = 0
    for _ in range(int(iters)):
        q = A @ d
        alpha = rho / np.vdot(d, q).real
        x = x + alpha * d
        r = r - alpha * q
        z = r if m is None else np.asarray(m) * r
        rho_new = np.vdot(r, z).real
        delta = np.vdot(r, r).real
        beta = rho_new / rho
        d = z + beta * d
        rho = rho_new
        its += 1
        hist.append(delta)
        alphas.append(alpha)
        betas.append(beta)
        if tol is not None and not (np.sqrt(delta) >= tol):
            break
    return {"x": x, "history": np.array(hist), "alpha": np.array(alphas), "beta": np.array(betas), "its": its}
