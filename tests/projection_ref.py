"""Solution projection (include/cgamd.h "Solution projection", csrc/projection.hip) restated in numpy -- no GPU.

Two modes of one algorithm, on (nrhs, n) arrays, every column with a basis of its own:
* type-true: one rounding per operation in the handle's type T (the element-wise expressions of cg_step_ref.Ops: vadd / vsub / vmul by
  components), the dots <w_j, v> in the order the header states -- the order of dot_partials_kernel on G = dots_grid(T, n) work-groups,
  then sum_partials_block -- accumulated in double / complex double and rounded once to T.  With the vectors of the device this gives
  the device's alpha, c, x0, e and e' BIT FOR BIT (the kernel tests compare them so); nu, s and what follows them go through the
  matrix product, whose row sums the device orders in its own way, so from there on the device is close, not equal.
* wide: the same steps in float64 / complex128 with plain sums.

Also here: the systems and the two sequences of right-hand sides of the tests, and CG with the handle's stopping rule.
"""
import numpy as np

import cg_step_ref as S
import mixed_ref as M

NX, NY = 33, 29                 # 957 rows: fp32, fp64 and complex64 handles carry padding rows
MOVE_STEP = 0.02               # the moving source advances by this much of the unit interval per solve
REL_TOL = {np.dtype(np.float32): 1e-4, np.dtype(np.complex64): 1e-4, np.dtype(np.float64): 1e-8, np.dtype(np.complex128): 1e-8}


def acc_type(dtype):
    return np.dtype(np.complex128 if np.dtype(dtype).kind == "c" else np.float64)


def drop_tol(dtype):
    """the span3 tests' drop_tol: 100 times the relative stop.  A solve stopped at a relative residual tau leaves an error of relative
    A-norm about tau (1.2 to 2.1 tau on these sequences), so a vector below 100 tau is mostly solver error: 1e-6 in the 64-bit types,
    1e-2 in the 32-bit types (1e-6 there would accept the fourth vector, 1.3e-4 of the solution, and fill the basis with noise)"""
    return 100.0 * REL_TOL[np.dtype(dtype)]


def eps(dtype):
    return float(np.finfo(np.dtype(dtype)).eps)


def ld_of(n, dtype):
    """cgamd_solver_ld: the size rounded up to whole 16-byte packs"""
    E = 16 // np.dtype(dtype).itemsize
    return -(-n // E) * E


def dots_grid(dtype, n):
    """cgamd_projection_dots_grid"""
    E = 16 // np.dtype(dtype).itemsize
    ppt = 1 if n <= 65536 else 2 if n <= 524288 else 4
    return int(max(1, min(1024, -(-n // (256 * E * ppt)))))


# ---- systems and sequences ---------------------------------------------------------------------------------------------------------
def system(dtype, scale=1.0):
    """5-point Poisson on 33 x 29 as (indptr, indices, data of `dtype`); the complex types use it times (1 + 0.05i)"""
    dtype = np.dtype(dtype)
    ip, ix, da = M.poisson2d_rect(NX, NY)
    da = da * scale
    if dtype.kind == "c":
        da = da * (1.0 + 0.05j)
    return ip, ix, da.astype(dtype)


def matvec(mat, v, dtype=None, acc=None):
    """(nrhs, n) -> (nrhs, n): products in `dtype`, every row summed in `acc`, rounded once.  mat: one (indptr, indices, data) for all
    columns, or a list of them, one per column (a batched handle)"""
    mats = mat if isinstance(mat, list) else [mat] * v.shape[0]
    dtype = np.dtype(dtype or v.dtype)
    return np.stack([M.csr_matvec(ip, ix, da.astype(dtype), np.ascontiguousarray(v[r], dtype=dtype), acc) for r, (ip, ix, da) in enumerate(mats)])


def _modes():
    n = NX * NY
    xs = np.linspace(0.0, 1.0, n)
    rng = np.random.default_rng(7)
    return xs, [np.sin(3 * (j + 1) * np.pi * xs) + 0.3 * rng.standard_normal(n) for j in range(3)]


def rhs(kind, t, dtype):
    """right-hand side t of a sequence, (n,) of `dtype`: "span3" b_t = A (u_0 + sin(2.2 t + 0.2) u_1 + cos(1.9 t) u_2) with A formed in
    float64 / complex128; "moving" b_t = exp(-(xs - 0.2 - 0.02 t)^2 / 0.01) + 1.
    (span3 with the frequencies 0.7 and 1.3 makes solutions 0 to 2 a poorly conditioned basis of the 3-dimensional space: solutions 6 to 8
    have coefficients of 1-norm 12.6, 15.6 and 11 in it, which multiplies the solves' own error -- every stored vector is a solution to
    the stop tolerance, no better -- so that those solves start at 6 to 7 times the tolerance instead of 1.3 to 2 times.  With 2.2 and
    1.9 the 1-norms stay below 1.4.)"""
    dtype = np.dtype(dtype)
    xs, u = _modes()
    if kind == "span3":
        wide = acc_type(dtype)
        v = (u[0] + np.sin(2.2 * t + 0.2) * u[1] + np.cos(1.9 * t) * u[2]).astype(wide)
        return matvec(system(wide), v[None, :])[0].astype(dtype)
    assert kind == "moving"
    return (np.exp(-((xs - 0.2 - MOVE_STEP * t) ** 2) / 0.01) + 1.0).astype(dtype)


def stop_tol(b, dtype):
    """the tests' stop: 1e-8 |b| in the 64-bit types, 1e-4 |b| in the 32-bit types"""
    return REL_TOL[np.dtype(dtype)] * float(np.linalg.norm(np.asarray(b).astype(acc_type(dtype))))


def _dot(a, b):
    acc = acc_type(a.dtype)
    return np.sum(a.astype(acc) * b.astype(acc), axis=-1)


def cg(mat, b, x0, tol, maxit=4000):
    """CG on one column in the type of b, sums in double, stopped like cgamd_solver_iterate_until: after the first iteration whose
    sqrt|r.r| is not >= tol.  Returns (x, iterations, r0.r0)"""
    dt = b.dtype
    acc = acc_type(dt)
    mv = lambda v: matvec(mat, v[None, :], dt, acc)[0]
    x = x0.astype(dt).copy()
    r = (b - mv(x)).astype(dt)
    d = r.copy()
    delta = dt.type(_dot(r, r))
    first = delta
    for k in range(1, maxit + 1):
        q = mv(d)
        alpha = dt.type(acc.type(delta) / _dot(d, q))
        x = (x + alpha * d).astype(dt)
        r = (r - alpha * q).astype(dt)
        dn = dt.type(_dot(r, r))
        if not float(np.sqrt(abs(dn))) >= tol:
            return x, k, first
        d = (r + dt.type(acc.type(dn) / acc.type(delta)) * d).astype(dt)
        delta = dn
    return x, maxit, first


# ---- the algorithm -------------------------------------------------------------------------------------------------------------------
class Projection:
    """The basis of nrhs columns.  dtype: the type the steps are rounded in (the handle's for type-true, float64 / complex128 for wide);
    exact_order: the dots in the order the header states (type-true) or plain sums (wide).  Vectors are carried at the padded length
    ld (zeros behind n), as the handle carries them, so that the packs of the stated order are the device's."""

    def __init__(self, mat, n, nrhs, dtype, capacity, drop_tol, exact_order=True, ld=None):
        self.mat, self.n, self.nrhs, self.dtype = mat, n, nrhs, np.dtype(dtype)
        self.acc = acc_type(dtype)
        self.K, self.drop_tol, self.exact = capacity, float(drop_tol), exact_order
        self.ld = ld if ld is not None else ld_of(n, dtype)
        self.G = dots_grid(self.dtype, self.ld)
        self.W = np.zeros((capacity, nrhs, self.ld), self.dtype)
        self.m = self.head = 0
        self.ops = S.Ops(self.dtype)
        self.alpha = np.zeros((capacity, nrhs), self.dtype)
        self.c = np.zeros((capacity, nrhs), self.dtype)
        self.x0 = np.zeros((nrhs, self.ld), self.dtype)
        self.nu = self.s = None
        self.last_slot = -1

    def _pad(self, v):
        out = np.zeros((self.nrhs, self.ld), self.dtype)
        out[:, :self.n] = np.asarray(v).reshape(self.nrhs, self.n)
        return out

    def dot_acc(self, a, b):
        """<a, b> per column in the accumulator type"""
        if not self.exact:
            return _dot(a, b)
        E = 16 // self.dtype.itemsize
        p = S.group_partials(self.ops.terms(a, b), self.G, E, True)
        return S.prologue_sum(p, 1024, 0)

    def dot(self, a, b):
        return S.from_acc(self.dot_acc(a, b), self.dtype)

    def spmv(self, v):
        out = np.zeros_like(v)
        out[:, :self.n] = matvec(self.mat, v[:, :self.n], self.dtype, self.acc)
        return out

    def held(self):
        return list(range(self.m))

    def guess(self, b):
        """alpha_j = <w_j, b>, x0 = sum_j alpha_j w_j (slots ascending, from +0); returns x0 (nrhs, n)"""
        b = self._pad(b)
        x0 = np.zeros((self.nrhs, self.ld), self.dtype)
        for j in self.held():
            self.alpha[j] = self.dot(self.W[j], b)
        for j in self.held():
            x0 = self.ops.axpy(x0, self.alpha[j], self.W[j])
        self.x0 = x0
        return x0[:, :self.n].copy()

    def update(self, x):
        """from the solve's x (nrhs, n); returns the added flags"""
        x = self._pad(x)
        retired = self.head if self.m == self.K else -1
        live = [j for j in self.held() if j != retired]
        e = self.ops.sub(x, self.x0)
        if retired >= 0:        # what the retired vector carried of the guess stays in what is added
            e = self.ops.axpy(e, self.alpha[retired], self.W[retired])
        q = self.spmv(e)
        for j in live:
            self.c[j] = self.dot(self.W[j], q)
        eq = self.dot_acc(e, q)
        e1 = e
        for j in live:
            e1 = self.ops.axmy(e1, self.c[j], self.W[j])
        nu = self.dot_acc(e1, self.spmv(e1))
        aa = np.zeros(self.nrhs, self.acc)
        ac = np.zeros(self.nrhs, self.acc)
        for j in live:
            aj = self.alpha[j].astype(self.acc)
            aa = aa + aj * aj
            ac = ac + aj * self.c[j].astype(self.acc)
        s = (aa + (ac + ac)) + eq
        with np.errstate(all="ignore"):
            ok = np.isfinite(nu) & (np.abs(nu) > self.drop_tol * self.drop_tol * np.abs(s))
            if self.dtype.kind != "c":
                ok = ok & (nu > 0)
            t = np.where(ok, S.from_acc(1.0 / np.sqrt(np.where(ok, nu, 1.0)), self.dtype), self.dtype.type(0))
        self.nu, self.s, self.e, self.e1 = nu, s, e, e1
        self.last_slot = -1
        if ok.any():
            slot = retired if retired >= 0 else self.m
            w = self.ops.mr(np.broadcast_to(t[:, None], e1.shape), e1)
            w[~ok] = 0
            self.W[slot] = w
            self.last_slot = slot
            if retired >= 0:
                self.head = (self.head + 1) % self.K
            else:
                self.m += 1
        return ok

    def gram_defect(self, W=None):
        """max |W^T A W - I| over the held slots of every column, formed in float64 / complex128 (columns of zeros -- refused -- left out)"""
        W = self.W[:self.m] if W is None else W
        wide = self.acc
        worst = 0.0
        for r in range(self.nrhs):
            cols = [W[j, r, :self.n].astype(wide) for j in range(W.shape[0]) if np.any(W[j, r] != 0)]
            if not cols:
                continue
            V = np.stack(cols)
            mat_r = self.mat[r] if isinstance(self.mat, list) else self.mat
            AV = matvec([mat_r] * len(cols), V, wide)
            worst = max(worst, float(np.abs(V @ AV.T - np.eye(len(cols))).max()))
        return worst


def run_sequence(kind, dtype, capacity, drop_tol, solves, exact_order=True, work_dtype=None, feed=None):
    """One column through `solves` right-hand sides: guess, CG to the tests' tolerance from the guess (and from zero, for the count),
    update.  work_dtype: the type of the projection steps (default `dtype`; the wide mode passes float64 / complex128 and keeps the CG
    iterates it is fed).  feed: the x of every solve (skips CG).  Returns a list of dicts per solve."""
    dtype = np.dtype(dtype)
    work = np.dtype(work_dtype or dtype)
    mat = system(dtype)
    n = NX * NY
    P = Projection((mat[0], mat[1], mat[2].astype(work)), n, 1, work, capacity, drop_tol, exact_order, ld=ld_of(n, dtype))
    out = []
    for t in range(solves):
        b = rhs(kind, t, dtype)
        tol = stop_tol(b, dtype)
        x0 = P.guess(b.astype(work)[None, :])
        rec = {"t": t, "tol": tol, "x0": x0[0].copy(), "alpha": P.alpha[:, 0].copy(), "count_before": P.m}
        if feed is None:
            x, its, r0 = cg(mat, b, x0[0].astype(dtype), tol)
            _, its0, _ = cg(mat, b, np.zeros(n, dtype), tol)
            rec.update(x=x, its=its, its_zero=its0, start=float(np.sqrt(abs(r0))))
        else:
            x = feed[t]
            rec.update(x=x)
        added = P.update(np.asarray(x).astype(work)[None, :])
        rec.update(added=bool(added[0]), count=P.m, slot=P.last_slot, c=P.c[:, 0].copy(), nu=P.nu[0], s=P.s[0], W=P.W[:, 0, :n].copy(),
                   defect=P.gram_defect())
        out.append(rec)
    return out


def distance(a, b):
    """how far two runs of one sequence are apart: the largest of |dW| / max|W| per stored vector, |d alpha| / sqrt|s| and
    |d c| / sqrt|s| (the scalars are A-inner products with x and with x - x0: sqrt|s| = the A-norm of x is their scale)"""
    worst = 0.0
    for ra, rb in zip(a, b):
        scale = float(np.sqrt(abs(rb["s"]))) or 1.0
        worst = max(worst, float(np.abs(ra["alpha"].astype(np.complex128) - rb["alpha"]).max()) / scale,
                    float(np.abs(ra["c"].astype(np.complex128) - rb["c"]).max()) / scale)
        for wa, wb in zip(ra["W"], rb["W"]):
            top = float(np.abs(wb).max())
            if top > 0:
                worst = max(worst, float(np.abs(wa.astype(np.complex128) - wb).max()) / top)
    return worst
