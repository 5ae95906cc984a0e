"""Host restatement of the vector and scalar steps of a CG / Jacobi-PCG iteration (csrc/vector.hip, csrc/reduce_device.h) -- pure
numpy, no GPU -- built on the helpers of spmv_ref.py.

Why it can be exact
-------------------
The library is compiled with -ffp-contract=off: every expression is evaluated as written, one rounding per multiply and per add in
the value type T, complex values by components (device_types.h vadd / vsub / vmul / vaypx).  Sums are formed in the accumulator type
(double; two doubles for the complex types) in an order that does not depend on timing.  numpy's float32 / float64 array operations
are single IEEE operations, so every value below can be compared with the device's BIT FOR BIT.

Rules restated (file:line of the rule)
--------------------------------------
element-wise, in T (vector.hip):
    r   = vsub(r, vmul(al, q))                 axpy_dot_body :137,:145; ewise OP 1 :235; pcg_axpy2_dot2 :521,:538
    x   = vadd(x, vmul(al, d))                 aypx_beta_x :350,:360; ewise OP 0 :234; pcg_aypx_beta :613,:624; xlag :462,:475
    d   = vaypx(bt, d, r) = vadd(vmul(bt, d), r)      aypx_beta_x :351,:361; ewise OP 2 :236; aypx_beta_out :415; xlag :463,:478
    r0  = vsub(b, q)                           ewise OP 3 :237 (launch_sub(b, q, r), solver.cpp set_rhs)
    z   = vmul(m, r)                           pcg_axpy2_dot2 :527,:541
    p   = vadd(vmul(bt, p), vmul(m, r))        pcg_aypx_beta :614,:626
a work-group's partial (dot_partials :203-218, axpy_dot_body :126-150, pcg_axpy2_dot2 :509-549): grid G work-groups of 256 threads,
E = 16 / sizeof(T) values per pack.  Thread (b, t) starts from +0 and adds to_acc(product) -- the product rounded in T, then widened --
of the packs b 256 + t + j G 256, j = 0, 1, ..., the E values of a pack in order; then the scalar tail, value npack E + b 256 + t
(+ j G 256); then block_sum<256> (device_types.h :189-202): the wave tree v[l] += v[l + off], off = 32 .. 1, and ((w0 + w1) + w2) + w3.
The scalar form (VEC = false) is the same with E = 1.  The two PCG sums keep accumulators of their own.
prologue sums (reduce_device.h): thread_partials<BLOCK>(P, K) :16-27 -- K = 0: thread t adds p[t], p[t + BLOCK], ...; K > 0: thread
t < 256 adds p[t K .. t K + K - 1], the others hold 0 -- then block_sum<BLOCK>.  BLOCK = 256 in the folded prologues (vector.hip :98,
:180, :270, :320, :377, :569), 1024 in sum_partials_block :29-49 (cg_delta0, cg_alpha, cg_beta, pcg_delta0), whose 16 wave sums are
added in order and whose 8-loads-in-flight branch :36-42 adds in the same order.  cg_alpha2 (vector.hip :704-740): 32 parts of
ceil(P / 32) partials, each a sum_partials_block, added in part order from +0, real and imaginary parts separately.
scalar steps: dqT = T(dq); alpha = T(acc_div(double(delta), double(dqT))) (:101-102, :183-184, :692-693, :735-736);
dnT = T(r.r); beta = T(acc_div(double(dnT), double(delta_old))) (:274-276, :324-326, :750-751); PCG: rho, the parity buffer rho2 and
history = T(r.r) (:578-586, :654-658).  acc_div of complex values is Smith's algorithm by components (device_types.h :92-99).

Padding with zeros: the restatement pads every strided pass to whole rounds with +0.  acc + (+0) == acc in every bit unless acc is -0,
and an accumulator that starts from +0 never becomes -0 under round-to-nearest (x + (-x) = +0; +0 + (-0) = +0); `valid_inputs`
asserts that no accumulator or partial of the chosen inputs is -0.

The bounds
----------
u_T = 2^-24 / 2^-53, u_D = 2^-53, gamma_k(u) = k u / (1 - k u), u_ext the unit roundoff of np.longdouble.
* A partial of m terms against the exact products summed in longdouble (`check_partials`).  Real: each product is rounded once in T
  (relative u_T), widened exactly, and passes through at most m - 1 double additions in any order (a tree of m leaves has depth
  <= m - 1; the first addition to +0 is exact), so  |got - ref| <= (u_T + gamma_m(u_D) (1 + u_T)) * S,  S = sum |a_i||b_i|, plus the
  reference's own gamma_{m+1}(u_ext) S.  Complex, per component: a component of vmul is two products and one subtraction in T,
  gamma_2(u_T) relative to |ar||br| + |ai||bi| <= |a||b|, so (gamma_2(u_T) + gamma_m(u_D)(1 + gamma_2(u_T))) S + gamma_{m+2}(u_ext) S.
* The same partial against the T-rounded products summed in longdouble: the product roundings cancel and only
  (gamma_m(u_D) + gamma_m(u_ext)) * sum |t_i| remains.  For the 32-bit types this is 2^29 times tighter than u_T S: it is what shows
  that accumulation is in double -- the bits alone could not if the restatement shared the mistake.
* A full sum of P partials (`check_sum`): depth <= P - 1 in double, then one rounding to T where T is narrower:
  |T(sum) - sum_ext| <= (gamma_P(u_D) + gamma_P(u_ext)) sum |p_j| + u_T |sum| (the last term for the 32-bit types only), per component.
* alpha of a real type (`check_alpha`): alpha = T(delta / T(dq)) carries the factors (1 + e) of the sum (|e| <= gamma_P(u_D) c,
  c = sum |p_j| / |sum p_j|), of two roundings to T and of one double division: |alpha / alpha_ext - 1| <= D / (1 - D),
  D = gamma_P(u_D) c + 2 u_T + u_D + gamma_{P+2}(u_ext) c (Higham, Accuracy and Stability, lemma 3.1).  Complex alpha and beta are
  compared bit for bit only.

Mutations (`Rules`): each switch replaces one rule by a plausible wrong one; tests/test_cg_step_ref.py proves on the CPU that every
one of them changes a compared bit on the inputs the device module uses.
"""
import zlib

import numpy as np

import spmv_ref as R

LD = R.LD
U_D = LD(2) ** -53


class Rules:
    """the rules of the module docstring; a mutation is a Rules with one switch changed"""
    def __init__(self, **kw):
        self.waves = "inorder"          # "pairwise": wave sums added (w0 + w1) + (w2 + w3) ...
        self.tree = "tree"              # "sequential": lanes added 0, 1, 2, ... instead of the wave tree
        self.swap_blocked = False       # member-blocked order where strided is due and the other way round
        self.pack_after = False         # value k of every pack of the strided pass, then value k + 1, ...
        self.tail_first = False         # the scalar tail before the packs
        self.acc_in_T = False           # partials accumulated in T instead of double
        self.dq_unrounded = False       # d.q not rounded to T before the division
        self.textbook_div = False       # (a conj b) / |b|^2 instead of Smith's algorithm
        self.alpha2_onepass = False     # cg_alpha2's partials summed as one sum_partials_block
        self.contract = None            # one expression evaluated with a fused multiply-add (emulated in longdouble)
        for k, v in kw.items():
            assert k in self.__dict__, k
            setattr(self, k, v)


EXACT = Rules()
CONTRACTIBLE = ("axpy", "axmy", "aypx", "mr", "pcg_dir", "dot")


def acc_type(dtype):
    return np.complex128 if R.is_complex(dtype) else np.float64


def pack_values(dtype):
    return 16 // np.dtype(dtype).itemsize


# ---- element-wise operations in T -----------------------------------------------------------------------------------------------------
def _ld(v):
    return np.asarray(v).astype(LD)


def _mul(a, x, dtype, fused=False, watch=None):
    """vmul on (re, im) pairs; fused: the second product of each component contracted into the subtraction / addition.  watch: the
    products formed on the way (a real product; the four of a complex one) are noted too"""
    if watch is not None:
        for u in a:
            for v in x:
                if u is not None and v is not None:
                    watch.note_T(np.asarray(u * v))
    if a[1] is None or not fused:
        return R.vmul_t(a, x, dtype)
    Rt = R.real_type(dtype)
    ar, ai = a
    xr, xi = x
    return (_ld(ar) * _ld(xr) - _ld(ai * xi)).astype(Rt), (_ld(ar) * _ld(xi) + _ld(ai * xr)).astype(Rt)


def _muladd(a, x, y, dtype, sign, fused, watch=None):
    """y + sign * (a * x): vadd / vsub of vmul"""
    if a[1] is None:
        if watch is not None:
            watch.note_T(np.asarray(a[0] * x[0]))
        if fused:
            return (_ld(y[0]) + sign * (_ld(a[0]) * _ld(x[0]))).astype(R.real_type(dtype)), None
        p = a[0] * x[0]
        return (y[0] + p if sign > 0 else y[0] - p), None
    pr, pi = _mul(a, x, dtype, fused, watch)
    if sign > 0:
        return y[0] + pr, y[1] + pi
    return y[0] - pr, y[1] - pi


def _col(s, dtype):
    """per-right-hand-side scalars (nrhs,) as (nrhs, 1) parts"""
    re, im = R._parts(s, dtype)
    return re[:, None], (im[:, None] if im is not None else None)


class Ops:
    """the element-wise expressions and the products of the dots under a set of rules, on (nrhs, n) arrays of `dtype`"""
    def __init__(self, dtype, rules=EXACT, watch=None):
        self.dtype, self.rules, self.watch = np.dtype(dtype), rules, watch

    def _out(self, re, im):
        v = R._join(re, im, self.dtype)
        if self.watch is not None:
            self.watch.note_T(v)
        return v

    def _f(self, name):
        return self.rules.contract == name

    def axpy(self, y, a, x):       # vadd(y, vmul(a, x))
        with np.errstate(all="ignore"):
            return self._out(*_muladd(_col(a, self.dtype), R._parts(x, self.dtype), R._parts(y, self.dtype), self.dtype, +1, self._f("axpy"), self.watch))

    def axmy(self, y, a, x):       # vsub(y, vmul(a, x))
        with np.errstate(all="ignore"):
            return self._out(*_muladd(_col(a, self.dtype), R._parts(x, self.dtype), R._parts(y, self.dtype), self.dtype, -1, self._f("axmy"), self.watch))

    def aypx(self, a, y, x):       # vadd(vmul(a, y), x)
        with np.errstate(all="ignore"):
            return self._out(*_muladd(_col(a, self.dtype), R._parts(y, self.dtype), R._parts(x, self.dtype), self.dtype, +1, self._f("aypx"), self.watch))

    def sub(self, x, b):           # vsub(x, b)
        xr, xi = R._parts(x, self.dtype)
        br, bi = R._parts(b, self.dtype)
        with np.errstate(all="ignore"):
            return self._out(xr - br, xi - bi if xi is not None else None)

    def mr(self, m, r):            # vmul(m, r)
        with np.errstate(all="ignore"):
            return self._out(*_mul(R._parts(m, self.dtype), R._parts(r, self.dtype), self.dtype, self._f("mr"), self.watch))

    def pcg_dir(self, bt, p, m, r):    # vadd(vmul(bt, p), vmul(m, r))
        with np.errstate(all="ignore"):
            z = _mul(R._parts(m, self.dtype), R._parts(r, self.dtype), self.dtype, False, self.watch)
            return self._out(*_muladd(_col(bt, self.dtype), R._parts(p, self.dtype), z, self.dtype, +1, self._f("pcg_dir"), self.watch))

    def terms(self, a, b):
        """to_acc(vmul(a_i, b_i)): (nrhs, n) in the accumulator type (in T under acc_in_T)"""
        with np.errstate(all="ignore"):
            pr, pi = _mul(R._parts(a, self.dtype), R._parts(b, self.dtype), self.dtype, self._f("dot"), self.watch)
        t = R._join(pr, pi, self.dtype)
        if self.watch is not None:
            self.watch.note_T(t)
        return t if self.rules.acc_in_T else t.astype(acc_type(self.dtype))


# ---- sums ---------------------------------------------------------------------------------------------------------------------------------
def block_sum(v, rules=EXACT):
    """block_sum<BLOCK> on (nb, BLOCK): the wave tree per 64 lanes, then the wave sums in order"""
    with np.errstate(all="ignore"):
        w = v.reshape(v.shape[0], -1, 64)
        if rules.tree == "tree":
            off = 32
            while off > 0:
                w = w[..., :off] + w[..., off:2 * off]
                off //= 2
            w = w[..., 0]
        else:
            s = w[..., 0]
            for l in range(1, 64):
                s = s + w[..., l]
            w = s
        if rules.waves == "inorder":
            s = w[:, 0]
            for i in range(1, w.shape[1]):
                s = s + w[:, i]
            return s
        while w.shape[1] > 1:
            w = w[:, 0::2] + w[:, 1::2]
        return w[:, 0]


def group_partials(t, G, E, vec, rules=EXACT):
    """the partial of every work-group: t (nrhs, n) terms -> (nrhs, G)"""
    nrhs, n = t.shape
    S = G * 256
    if not vec:
        E = 1
    npack = n // E
    J = -(-npack // S)
    body = np.zeros((nrhs, J * S * E), t.dtype)
    body[:, :npack * E] = t[:, :npack * E]
    body = body.reshape(nrhs, J, S, E)
    tail = np.zeros((nrhs, S), t.dtype)
    assert n - npack * E <= S
    tail[:, :n - npack * E] = t[:, npack * E:]
    acc = np.zeros((nrhs, S), t.dtype)
    with np.errstate(all="ignore"):
        if rules.tail_first:
            acc = acc + tail
        if rules.pack_after:
            for k in range(E):
                for j in range(J):
                    acc = acc + body[:, j, :, k]
        else:
            for j in range(J):
                for k in range(E):
                    acc = acc + body[:, j, :, k]
        if not rules.tail_first:
            acc = acc + tail
    return block_sum(acc.reshape(nrhs * G, 256), rules).reshape(nrhs, G)


def thread_partials(p, BLOCK, K, rules=EXACT):
    """reduce_device.h thread_partials<BLOCK>: p (nrhs, P) -> (nrhs, BLOCK)"""
    nrhs, P = p.shape
    if rules.swap_blocked:
        K = 0 if K > 0 else max(1, -(-P // 256))
    acc = np.zeros((nrhs, BLOCK), p.dtype)
    with np.errstate(all="ignore"):
        if K > 0:
            assert P <= 256 * K, "member-blocked order: the partials beyond 256 K would be dropped"
            pad = np.zeros((nrhs, 256 * K), p.dtype)
            pad[:, :P] = p
            pad = pad.reshape(nrhs, 256, K)
            a = np.zeros((nrhs, 256), p.dtype)
            for k in range(K):
                a = a + pad[:, :, k]
            acc[:, :256] = a
        else:
            J = -(-P // BLOCK)
            pad = np.zeros((nrhs, J * BLOCK), p.dtype)
            pad[:, :P] = p
            pad = pad.reshape(nrhs, J, BLOCK)
            for j in range(J):
                acc = acc + pad[:, j]
    return acc


def prologue_sum(p, BLOCK, K, rules=EXACT):
    """thread_partials<BLOCK>(P, K) then block_sum<BLOCK>: (nrhs,).  BLOCK = 1024 is sum_partials_block (its unrolled branch adds in
    the same order)"""
    return block_sum(thread_partials(p, BLOCK, K, rules), rules)


def alpha2_sum(p, rules=EXACT):
    """cg_alpha2_kernel: 32 contiguous parts, each a sum_partials_block, added in part order from +0"""
    if rules.alpha2_onepass:
        return prologue_sum(p, 1024, 0, rules)
    nrhs, P = p.shape
    per = (P + 31) // 32
    tot = np.zeros(nrhs, p.dtype)
    with np.errstate(all="ignore"):
        for k in range(32):
            lo = min(k * per, P)
            hi = min(lo + per, P)
            tot = tot + prologue_sum(p[:, lo:hi], 1024, 0, rules)
    return tot


# ---- scalar steps -------------------------------------------------------------------------------------------------------------------------
def acc_div(a, b, rules=EXACT):
    """device_types.h acc_div on double / (double, double) arrays"""
    with np.errstate(all="ignore"):
        if not np.iscomplexobj(a):
            return a / b
        ax, ay, bx, by = (np.ascontiguousarray(v, np.float64) for v in (a.real, a.imag, b.real, b.imag))
        out = np.empty(a.shape, np.complex128)
        if rules.textbook_div:
            den = bx * bx + by * by
            out.real, out.imag = (ax * bx + ay * by) / den, (ay * bx - ax * by) / den
            return out
        r1 = by / bx
        d1 = bx + by * r1
        r2 = bx / by
        d2 = bx * r2 + by
        big = np.abs(bx) >= np.abs(by)
        out.real = np.where(big, (ax + ay * r1) / d1, (ax * r2 + ay) / d2)
        out.imag = np.where(big, (ay - ax * r1) / d1, (ay * r2 - ax) / d2)
        return out


def from_acc(a, dtype):
    with np.errstate(all="ignore"):
        return np.asarray(a).astype(dtype)          # by components for the complex types


def to_acc(v):
    return np.asarray(v).astype(acc_type(v.dtype))


def quotient(num, den, dtype, rules=EXACT):
    """T(acc_div(double(num), double(den)))"""
    return from_acc(acc_div(to_acc(num), to_acc(den), rules), dtype)


# ---- validity of the inputs -----------------------------------------------------------------------------------------------------------------
class Watch:
    """collects what `valid_inputs` asserts: no value formed in T is subnormal, infinite or NaN; no accumulator is -0"""
    def __init__(self):
        self.bad_T = 0
        self.neg_zero = 0
        self.seen = 0

    def note_T(self, v):
        a = np.abs(np.asarray(v).view(R.real_type(v.dtype)))
        tiny = np.finfo(a.dtype).tiny
        self.bad_T += int(np.count_nonzero(~np.isfinite(a) | ((a > 0) & (a < tiny))))
        self.seen += a.size

    def note_acc(self, v):
        a = np.asarray(v)
        a = a.view(np.float64) if a.dtype.kind == "c" else a
        self.neg_zero += int(np.count_nonzero((a == 0) & np.signbit(a)))
        self.bad_T += int(np.count_nonzero(~np.isfinite(a)))
        self.seen += a.size


# ---- whole steps --------------------------------------------------------------------------------------------------------------------------
class Steps:
    """set_rhs and iterations of one handle.  ip, ix, da: the CSR WITH the appended empty rows (n = plan["n"] rows); da (nnz,) or,
    for a batched handle, (nrhs, nnz).  plan: Solver.step_plan().  m: None, (n,) shared or (nrhs, n) per system.  State: x, r, d, q
    (nrhs, n); part_dq (nrhs, n_partials), part_rr / part_rz (nrhs, vgrid) in the accumulator type; alpha, beta, delta (nrhs,),
    rho2 (2, nrhs) in T; it; history (list of (nrhs,))."""
    def __init__(self, ip, ix, da, dtype, nrhs, plan, m=None, unfused=False, rules=EXACT, watch=None, spmv_cache=None, two=False):
        self.two = two
        self.ip, self.ix, self.da = ip, ix, np.asarray(da)
        self.dtype, self.nrhs, self.plan = np.dtype(dtype), nrhs, dict(plan)
        self.n = len(ip) - 1
        assert self.n == plan["n"], (self.n, plan["n"])
        self.m = None if m is None else np.broadcast_to(np.asarray(m, dtype=dtype).reshape(-1, self.n), (nrhs, self.n))
        self.unfused, self.rules, self.watch = unfused, rules, watch
        self.ops = Ops(dtype, rules, watch)
        self.E = pack_values(dtype)
        self.cache = spmv_cache if spmv_cache is not None else {}
        self.part_dq = self.part_rz = None
        self.rho2 = None

    # -- pieces
    def spmv(self, v):
        key = zlib.crc32(v.tobytes()), v.shape
        if key not in self.cache:
            if self.da.ndim == 2:
                q = np.concatenate([R.spmv_in_type(self.ip, self.ix, self.da[r], v[r], self.dtype, 1) for r in range(self.nrhs)])
            else:
                q = R.spmv_in_type(self.ip, self.ix, self.da, v, self.dtype, self.nrhs)
            self.cache[key] = (v.copy(), q)
        v0, q = self.cache[key]
        assert R.bit_equal(v0, v)
        return q.copy()

    def dq_partials(self, d, q):
        p = np.stack([R.block_partials_in_type(d[r], q[r], self.dtype) for r in range(self.nrhs)])
        assert p.shape[1] == self.plan["n_partials"], (p.shape, self.plan["n_partials"])
        return self._acc(p)

    def _acc(self, p):
        p = p.astype(acc_type(self.dtype))
        if self.watch is not None:
            self.watch.note_acc(p)
        return p

    def dot(self, a, b):
        return self._acc(group_partials(self.ops.terms(a, b), self.plan["vgrid"], self.E, bool(self.plan["vec"]), self.rules))

    def total(self, p, BLOCK, K):
        return self._acc(prologue_sum(p, BLOCK, K, self.rules))

    def alpha_step(self, p):
        """alpha from the d.q partials p by the launch the plan names (alpha_value), and the counter"""
        al = alpha_value(p, self.delta, self.plan, self.dtype, self.rules, self.watch)
        if self.watch is not None:
            self.watch.note_T(al)
        self.alpha = al
        self.it += 1

    # -- set_rhs (solver.cpp cgamd_solver_set_rhs)
    def set_rhs(self, b, x0=None):
        n, nrhs, dt = self.n, self.nrhs, self.dtype
        self.b = np.asarray(b, dtype=dt).reshape(nrhs, n)
        self.x = np.zeros((nrhs, n), dt) if x0 is None else np.array(x0, dtype=dt).reshape(nrhs, n)
        self.q = self.spmv(self.x)
        self.r = self.ops.sub(self.b, self.q)
        self.it = 0
        if self.m is not None:         # INIT form of pcg_axpy2_dot2, then pcg_delta0
            z = self.ops.mr(self.m, self.r)
            self.d = z
            self.part_rz = self.dot(self.r, z)
            self.part_rr = self.dot(self.r, self.r)
            rho = from_acc(self.total(self.part_rz, 1024, 0), dt)
            self.delta = rho
            self.rho2 = np.zeros((2, nrhs), dt)
            self.rho2[0] = rho
            self.history = [from_acc(self.total(self.part_rr, 1024, 0), dt)]
        else:                          # d = r, dot_partials, cg_delta0
            self.d = self.r.copy()
            self.part_rr = self.dot(self.r, self.r)
            self.delta = from_acc(self.total(self.part_rr, 1024, 0), dt)
            self.history = [self.delta.copy()]
        self.alpha = self.beta = None
        return self

    # -- one iteration (solver.cpp enqueue_iteration)
    def iterate(self, count=1):
        for _ in range(count):
            if self.m is not None:
                self._pcg()
            elif self.unfused:
                self._unfused()
            elif self.two:
                self._two_launch()
            else:
                self._fused()
        return self

    def _beta_from(self, new, old):
        bt = quotient(new, old, self.dtype, self.rules)
        if self.watch is not None:
            self.watch.note_T(bt)
            self.watch.note_T(new)
        return bt

    def _fused(self):
        """SpMV + d.q partials; alpha (folded, cg_alpha or cg_alpha2); axpy_dot(_alpha); aypx_beta_x (or the steps of a group of the
        deferred x update, which apply the same operations to every element in the same order)"""
        pl, dt = self.plan, self.dtype
        self.q = self.spmv(self.d)
        self.part_dq = self.dq_partials(self.d, self.q)
        self.alpha_step(self.part_dq)
        self.r = self.ops.axmy(self.r, self.alpha, self.q)
        self.part_rr = self.dot(self.r, self.r)
        dn = from_acc(self.total(self.part_rr, 256, pl["krr"]), dt)
        self.beta = self._beta_from(dn, self.history[self.it - 1])
        self.delta = dn
        self.history.append(dn)
        self.x = self.ops.axpy(self.x, self.alpha, self.d)
        self.d = self.ops.aypx(self.beta, self.d, self.r)

    def _two_launch(self):
        """spmv.hip spmv_fused_kernel: beta of the PREVIOUS iteration (0 in the first) and d = vaypx(beta, d, r) at the head of the SpMV
        launch, q = A d, d.q partials; vector.hip axpy2_dot_alpha: alpha in the prologue, x += alpha d, r -= alpha q, r.r partials;
        cg_tail_kernel at the end of the call: delta, beta, history -- the sums in the order of the three-launch loop's prologues"""
        pl, dt = self.plan, self.dtype
        bt = np.zeros(self.nrhs, dt) if self.it == 0 else self.beta
        self.d = self.ops.aypx(bt, self.d, self.r)
        self.q = self.spmv(self.d)
        self.part_dq = self.dq_partials(self.d, self.q)
        self.alpha_step(self.part_dq)
        self.x = self.ops.axpy(self.x, self.alpha, self.d)
        self.r = self.ops.axmy(self.r, self.alpha, self.q)
        self.part_rr = self.dot(self.r, self.r)
        dn = from_acc(self.total(self.part_rr, 256, pl["krr"]), dt)
        self.beta = self._beta_from(dn, self.history[self.it - 1])
        self.delta = dn
        self.history.append(dn)

    def _unfused(self):
        """the eight launches: SpMV, dot_partials(d, q), cg_alpha, axpy +, axpy -, dot_partials(r, r), cg_beta, aypx"""
        dt = self.dtype
        self.q = self.spmv(self.d)
        self.part_rr = self.dot(self.d, self.q)
        self.alpha_step(self.part_rr)
        self.x = self.ops.axpy(self.x, self.alpha, self.d)
        self.r = self.ops.axmy(self.r, self.alpha, self.q)
        self.part_rr = self.dot(self.r, self.r)
        dn = from_acc(self.total(self.part_rr, 1024, 0), dt)
        self.beta = self._beta_from(dn, self.delta)
        self.delta = dn
        self.history.append(dn)
        self.d = self.ops.aypx(self.beta, self.d, self.r)

    def _pcg(self):
        """SpMV + p.q partials; cg_alpha on delta = rho; pcg_axpy2_dot2; pcg_aypx_beta"""
        pl, dt = self.plan, self.dtype
        self.q = self.spmv(self.d)
        self.part_dq = self.dq_partials(self.d, self.q)
        self.alpha_step(self.part_dq)
        self.r = self.ops.axmy(self.r, self.alpha, self.q)
        z = self.ops.mr(self.m, self.r)
        self.part_rz = self.dot(self.r, z)
        self.part_rr = self.dot(self.r, self.r)
        rho = from_acc(self.total(self.part_rz, 256, pl["krr"]), dt)
        rr = from_acc(self.total(self.part_rr, 256, pl["krr"]), dt)
        self.beta = self._beta_from(rho, self.rho2[(self.it - 1) & 1])
        self.delta = rho
        self.rho2[self.it & 1] = rho
        self.history.append(rr)
        self.x = self.ops.axpy(self.x, self.alpha, self.d)
        self.d = self.ops.pcg_dir(self.beta, self.d, self.m, self.r)

    def state(self):
        """what the device module compares, by name"""
        out = {"x": self.x, "r": self.r, "d": self.d, "q": self.q, "part_rr": self.part_rr, "delta": self.delta,
               "iter": np.array([self.it]), "history": np.stack(self.history)}
        if self.part_dq is not None:
            out["part_dq"] = self.part_dq
        if self.part_rz is not None:
            out["part_rz"], out["rho2"] = self.part_rz, self.rho2.copy()
        if self.alpha is not None:
            out["alpha"], out["beta"] = self.alpha, self.beta
        return out


# ---- longdouble references and the bounds ---------------------------------------------------------------------------------------------------
def element_groups(n, G, E, vec):
    """the work-group whose partial element i is added to"""
    S = G * 256
    if not vec:
        E = 1
    npack = n // E
    i = np.arange(n)
    return np.where(i < npack * E, ((i // E) % S) // 256, (i - npack * E) // 256)


def _group_sum(v, g, G):
    out = np.zeros(G, LD)
    np.add.at(out, g, v)
    return out


def check_partials(got, a, b, dtype, G, E, vec, label=""):
    """got (nrhs, G) partials of a.b against both references of the module docstring; returns the largest error / bound ratios
    (exact products, T-rounded products) and asserts both <= 1"""
    dtype = np.dtype(dtype)
    a, b = np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype)
    nrhs, n = a.shape
    cplx = R.is_complex(dtype)
    uT = R.unit_roundoff(dtype)
    g = element_groups(n, G, E, vec)
    m = np.bincount(g, minlength=G).astype(LD)
    worst = [0.0, 0.0]
    for r in range(nrhs):
        ar, ai = (_ld(v) for v in (a[r].real, a[r].imag))
        br, bi = (_ld(v) for v in (b[r].real, b[r].imag))
        S = _group_sum(np.hypot(ar, ai) * np.hypot(br, bi), g, G)
        with np.errstate(all="ignore"):
            tr, ti = R.vmul_t(R._parts(a[r], dtype), R._parts(b[r], dtype), dtype)
        comps = [(ar * br - ai * bi, tr, got[r].real)]
        if cplx:
            comps.append((ar * bi + ai * br, ti, got[r].imag))
        for exact, t, gv in comps:
            gv = _ld(gv)
            if cplx:
                bound1 = (R.gamma(2, uT) + R.gamma(m, U_D) * (1 + R.gamma(2, uT)) + R.gamma(m + 2, R.U_EXT)) * S
            else:
                bound1 = (uT + R.gamma(m, U_D) * (1 + uT) + R.gamma(m + 1, R.U_EXT)) * S
            err1 = np.abs(gv - _group_sum(exact, g, G))
            tl = _ld(t)
            bound2 = (R.gamma(m, U_D) + R.gamma(m, R.U_EXT)) * _group_sum(np.abs(tl), g, G)
            err2 = np.abs(gv - _group_sum(tl, g, G))
            for k, (e, bd) in enumerate(((err1, bound1), (err2, bound2))):
                ok = (e <= bd)
                assert np.all(ok), f"{label}: partial {np.nonzero(~ok)[0][:4].tolist()} of right-hand side {r} outside bound {k + 1}"
                with np.errstate(all="ignore"):
                    ratio = np.where(bd > 0, e / np.where(bd > 0, bd, 1), 0)
                worst[k] = max(worst[k], float(ratio.max()))
    return tuple(worst)


def check_sum(got_T, p, dtype, label=""):
    """got_T (nrhs,) = T(sum of the partials p (nrhs, P)) against their longdouble sum; returns the largest error / bound"""
    dtype = np.dtype(dtype)
    P = p.shape[1]
    narrow = R.real_type(dtype) is np.float32
    uT = R.unit_roundoff(dtype)
    worst = 0.0
    comps = [(got_T.real, p.real)] + ([(got_T.imag, p.imag)] if R.is_complex(dtype) else [])
    for gv, pv in comps:
        pv = _ld(pv)
        ref = pv.sum(axis=1)
        bound = (R.gamma(P, U_D) + R.gamma(P, R.U_EXT)) * np.abs(pv).sum(axis=1) + (uT * np.abs(ref) * (1 + R.gamma(P, U_D)) if narrow else 0)
        err = np.abs(_ld(gv) - ref)
        assert np.all(err <= bound), f"{label}: sum outside the bound: {err} > {bound}"
        with np.errstate(all="ignore"):
            worst = max(worst, float(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0).max()))
    return worst


def check_alpha(alpha, delta, p, dtype, label=""):
    """real types: alpha (nrhs,) = T(delta / T(sum p)) against delta / sum_ext(p); returns the largest error / bound"""
    dtype = np.dtype(dtype)
    assert not R.is_complex(dtype)
    P = p.shape[1]
    uT = R.unit_roundoff(dtype)
    pv = _ld(p)
    ref_sum = pv.sum(axis=1)
    c = np.abs(pv).sum(axis=1) / np.abs(ref_sum)
    D = R.gamma(P, U_D) * c + 2 * uT + U_D + R.gamma(P + 2, R.U_EXT) * c
    bound = D / (1 - D)
    err = np.abs(_ld(alpha) / (_ld(delta) / ref_sum) - 1)
    assert np.all(err <= bound), f"{label}: alpha outside the bound: {err} > {bound}"
    return float((err / bound).max())


# ---- inputs shared by the host test and the device module ---------------------------------------------------------------------------------
def spread(rng, n, dtype, half=16):
    """magnitudes spread over 2^-half .. 2^half, random signs and mantissas (in the spirit of spmv_ref.adversarial_d)"""
    Rt = R.real_type(dtype)

    def one():
        return (rng.uniform(1.0, 2.0, n) * np.exp2(rng.integers(-half, half + 1, n)) * rng.choice([-1.0, 1.0], n)).astype(Rt)
    if R.is_complex(dtype):
        return R._join(one(), one(), dtype)
    return one().astype(dtype)


def chain_matrix(n, dtype, far=0):
    """SPD Toeplitz chain: 2.5 (+ 2 * 0.7 with `far`) on the diagonal, -1 at distance 1, -0.7 at distance `far`; complex types: times
    (1 + 0.05j), complex symmetric.  Entries in the order (-far, -1, 0, 1, far) inside a row."""
    offs = (-1, 0, 1) if not far else (-far, -1, 0, 1, far)
    vals = {0: 2.5 + (1.4 if far else 0.0), -1: -1.0, 1: -1.0}
    if far:
        vals.update({far: -0.7, -far: -0.7})
    rows = np.repeat(np.arange(n, dtype=np.int64), len(offs))
    o = np.tile(np.asarray(offs, dtype=np.int64), n)
    cols = rows + o
    keep = (cols >= 0) & (cols < n)
    ip = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows[keep], minlength=n), out=ip[1:])
    da = np.array([vals[int(k)] for k in offs])[np.tile(np.arange(len(offs)), n)][keep]
    if R.is_complex(dtype):
        da = da * (1.0 + 0.05j)
    return ip, cols[keep].astype(np.int32), da.astype(dtype)


def pad_system(ip, n_to):
    """the row pointers with the appended empty rows of a handle whose working size is n_to"""
    n = len(ip) - 1
    assert n_to >= n
    return np.concatenate([ip, np.full(n_to - n, ip[-1], dtype=ip.dtype)])


def pad_vectors(v, nrhs, n, n_to):
    out = np.zeros((nrhs, n_to), dtype=v.dtype)
    out[:, :n] = np.asarray(v).reshape(nrhs, n)
    return out


def case_inputs(n, dtype, nrhs, seed, x0=True, jacobi=None, far=0):
    """matrix, right-hand sides, first guess and (jacobi: "shared" / "systems") the inverse diagonals of one case, from its seed"""
    rng = np.random.default_rng(seed)
    ip, ix, da = chain_matrix(n, dtype, far)
    # (every 256-row block scaled by a power of two of its own: the partial ARRAYS spread as well, so the order of the prologue sums
    # shows in their bits)
    block = np.repeat(np.exp2(rng.integers(-8, 9, -(-n // 256))), 256)[:n].astype(R.real_type(dtype))
    B = np.stack([spread(rng, n, dtype) * block for _ in range(nrhs)])
    X0 = np.stack([spread(rng, n, dtype, half=8) for _ in range(nrhs)]) if x0 else None
    out = {"ip": ip, "ix": ix, "da": da, "B": B, "X0": X0, "m": None, "n": n}
    if jacobi:
        # inverse diagonals with magnitudes of their own (a diagonal preconditioner need not be 1 / diag(A) to be SPD)
        k = nrhs if jacobi == "systems" else 1
        m = np.stack([np.abs(spread(rng, n, np.float64, half=6)) for _ in range(k)])
        out["m"] = (m * ((1.0 + 0.03j) if R.is_complex(dtype) else 1.0)).astype(dtype)
        if jacobi == "systems":          # a batched handle: values of their own per system on the one pattern
            scale = 1.0 + 0.25 * np.arange(nrhs)
            out["da"] = np.stack([(da * s).astype(dtype) for s in scale])
    return out


# ---- the cases of tests/test_gpu_cg_steps.py, and the plan each must report (host copy of vector.hip vec_grid and of the rules of
# solver.cpp that Solver.step_plan() reads; the device module asserts the record against it before anything else) ----------------------
DT = {"f32": np.float32, "f64": np.float64, "c64": np.complex64, "c128": np.complex128}
# launched loops only, three / four launches: no resident loop, no two-launch loop
LAUNCHED = {"resident": 0, "resident_wide": 0, "two_launch": 0}
TUNE_DEFAULTS = {"resident": 1, "resident_wide": 1, "two_launch": 1, "pad_rows": 1, "vec_grid": 0, "dev.vec_ppt": 0,
                 "dev.no_fold_alpha": 0, "dev.x_lag": -1}
NO_GRAPH, UNFUSED = "NO_GRAPH", "UNFUSED"


def host_vec_grid(n, dtype, nrhs, knobs):
    total = n * max(nrhs, 1)
    ppt = knobs.get("dev.vec_ppt", 0) or (1 if (total <= 262144 or n <= 65536) else 2 if total <= 524288 else 4)
    per_block = 256 * pack_values(dtype) * ppt
    g = min(-(-n // per_block), knobs.get("vec_grid", 0) or 2048)
    if nrhs <= 1 and not knobs.get("vec_grid", 0) and g > 512:
        g = 512
    return max(g, 1)


def host_plan(case):
    """the fields of Solver.step_plan() a case is written for (vec_nt is a streaming hint without influence on any bit: not predicted)"""
    dtype, nrhs, knobs = DT[case["dt"]], case["nrhs"], case["knobs"]
    E = pack_values(dtype)
    n = case["n"] if not knobs.get("pad_rows", 1) else -(-case["n"] // E) * E
    P = -(-n // 256)
    wide = case.get("wide", False)
    unfused = UNFUSED in case["flags"]
    pcg = bool(case.get("jacobi"))
    fold = (not unfused and not pcg and not knobs.get("dev.no_fold_alpha", 0) and P <= 2048)
    alpha_grid = host_vec_grid(n, dtype, nrhs, knobs) if unfused else P
    kdq = 8 if wide else 0
    # solver.cpp setup_x_lag / x_lag_now: the default rule defers x by 4 iterations in captured runs of the four-launch loop
    knob = knobs.get("dev.x_lag", -1)
    lag = max(knob, 1) if knob >= 0 else (1 if fold or wide else 4)
    if pcg or unfused or NO_GRAPH in case["flags"] or case.get("two"):
        lag = 1
    return {"n": n, "ld": n, "vgrid": -(-(n // E) // 256) if wide else host_vec_grid(n, dtype, nrhs, knobs), "n_partials": P,
            "kdq": kdq, "krr": kdq // E, "fold": int(fold), "alpha2": int(not fold and alpha_grid >= 16384),
            "vec": int(nrhs == 1 or (n * np.dtype(dtype).itemsize) % 16 == 0), "x_lag": lag}


def host_launches(case):
    """cgamd_solver_loop_launches of the case"""
    if case.get("jacobi"):
        return 4
    if UNFUSED in case["flags"]:
        return 8
    if case.get("two"):
        return 2
    return 3 if host_plan(case)["fold"] else 4


# cases whose seed was advanced until the mutation table of tests/test_cg_step_ref.py is all-detected (a mutation that shows in about
# a fifth of the draws of a one-thread sum needs a draw in which it shows)
SALT = {'edges-f32-5-x1-pad_rows0': '+21', 'edges-f64-3-x1-pad_rows0': '+1', 'edges-c64-3-x1-pad_rows0': '+1',
        'unrolled-c64-2360476-x1-nox0': '+1'}


def _case(group, dt, n, nrhs=1, knobs=None, flags=(), iters=2, x0=True, **kw):
    k = dict(LAUNCHED)
    k.update(knobs or {})
    c = {"group": group, "dt": dt, "n": n, "nrhs": nrhs, "knobs": k, "flags": tuple(flags), "iters": iters, "x0": x0}
    c.update(kw)
    tag = "-".join(f"{a.replace('dev.', '')}{b}" for a, b in sorted((knobs or {}).items()))
    c["id"] = "-".join(str(v) for v in (group, dt, n, f"x{nrhs}", tag, "".join(f[0] for f in flags), kw.get("jacobi", ""), "" if x0 else "nox0",
                                        f"lag{kw['lag']}" if "lag" in kw else "") if v != "")
    c["seed"] = zlib.crc32((c["id"] + SALT.get(c["id"], "")).encode())
    return c


def cases():
    out = []
    ALL = list(DT)
    for dt in ALL:
        E = pack_values(DT[dt])
        # pack and tail edges: default padding (appended rows), pad_rows = 0 (the VEC tail; odd n x 3: the scalar form)
        sizes = sorted({1, max(E - 1, 1), E, E + 1, 255, 256 * E - 1, 256 * E, 256 * E + 1} | {1000 + k for k in range(E)})
        for n in sizes:
            for nrhs in (1, 3):
                # (a system of one row is solved exactly by its first iteration: a second one would divide 0 by 0)
                it = 1 if n == 1 else 2
                out.append(_case("edges", dt, n, nrhs, iters=it))
                if n % E or nrhs == 1:
                    out.append(_case("edges", dt, n, nrhs, {"pad_rows": 0}, iters=it))
        # grid-stride rounds: 3 to 10 packs per thread; packs per thread the grid is sized for
        for vg in (1, 2, 3):
            out.append(_case("stride", dt, 5003, 1, {"vec_grid": vg, "pad_rows": 0}))
        for ppt in (1, 2, 4):
            out.append(_case("stride", dt, 5003, 3, {"dev.vec_ppt": ppt}))
        # loop kernels
        for n in (3001, 70001):
            out.append(_case("loops", dt, n, 1))                                             # folded, three launches (captured)
            out.append(_case("loops", dt, n, 3, {"dev.no_fold_alpha": 1}))                    # cg_alpha + axpy_dot
            out.append(_case("loops", dt, n, 1, flags=(UNFUSED,)))                            # the eight launches
            out.append(_case("loops", dt, n, 3, flags=(NO_GRAPH,)))                           # plain launches
            out.append(_case("loops", dt, n, 1, {"two_launch": 1}, two=True))                 # the two-launch loop
        for n in (3001, 70001):                                                               # a captured group of the deferred x update
            for lag in (4, 2):
                out.append(_case("lag", dt, n, 1, {"dev.x_lag": lag, "dev.no_fold_alpha": 1}, iters=8, lag=lag, at_end=True))
        # Jacobi PCG: shared M, and a batched handle with M per system
        for n in (3001, 70001):
            for nrhs in (1, 3):
                out.append(_case("pcg", dt, n, nrhs, jacobi="shared", x0=(nrhs == 1)))
            out.append(_case("pcg", dt, n, 3, jacobi="systems", x0=(n < 10000)))
    # member-blocked order: handles the chip-wide resident loop can take over, launched loop forced
    for dt in ("f64", "c64"):
        out.append(_case("wide", dt, 50000, 1, {"resident_wide": 1, "resident": 1}, flags=(NO_GRAPH,), wide=True))
        out.append(_case("wide", dt, 50000, 1, {"resident_wide": 1, "resident": 1}, flags=(NO_GRAPH,), wide=True, jacobi="shared"))
    # fold threshold
    out.append(_case("fold", "f64", 524288, 1, iters=1, x0=False))
    out.append(_case("fold", "f64", 524289, 1, {"pad_rows": 0}, iters=1, x0=False))
    # the 8-loads-in-flight branch of sum_partials_block: 9221 partials
    for dt in ("f64", "c64"):
        out.append(_case("unrolled", dt, 2360476, 1, iters=1, x0=False))
    # cg_alpha2: 16384 partials (per = 512) and 16391 (per = 513, a short last part of 488)
    for dt in ("f32", "f64", "c64"):
        out.append(_case("alpha2", dt, 16384 * 256, 1, iters=1, x0=False))
        out.append(_case("alpha2", dt, 16390 * 256 + 17, 1, {"pad_rows": 0}, iters=1, x0=False))
    return out


LARGE_GROUPS = ("fold", "unrolled", "alpha2")


def alpha_value(p, delta, plan, dtype, rules=EXACT, watch=None):
    """the alpha launch alone, on given partials: folded prologue (256 threads), cg_alpha2, or cg_alpha (sum_partials_block); then
    dqT = T(dq), alpha = T(acc_div(double(delta), double(dqT))).  Steps.alpha_step stores its result"""
    if plan["fold"]:
        dq = prologue_sum(p, 256, plan["kdq"], rules)
    elif plan["alpha2"]:
        dq = alpha2_sum(p, rules)
    else:
        dq = prologue_sum(p, 1024, plan["kdq"], rules)
    if watch is not None:
        watch.note_acc(dq)
    dqT = dq if rules.dq_unrounded else from_acc(dq, dtype)
    return from_acc(acc_div(to_acc(delta), to_acc(dqT), rules), dtype)


def build_steps(case, plan=None, rules=EXACT, watch=None, cache=None, inputs=None):
    """(Steps, inputs) of a case on the host; plan: the device's record (default: host_plan)"""
    dtype = DT[case["dt"]]
    plan = dict(plan or host_plan(case))
    inp = inputs or case_inputs(case["n"], dtype, case["nrhs"], case["seed"], x0=case["x0"], jacobi=case.get("jacobi"))
    n, nt, nrhs = case["n"], plan["n"], case["nrhs"]
    m = None if inp["m"] is None else pad_vectors(inp["m"], inp["m"].shape[0], n, nt)
    st = Steps(pad_system(inp["ip"], nt), inp["ix"], inp["da"], dtype, nrhs, plan, m=m, unfused=UNFUSED in case["flags"], rules=rules,
               watch=watch, spmv_cache=cache, two=bool(case.get("two")))
    st.set_rhs(pad_vectors(inp["B"], nrhs, n, nt), None if inp["X0"] is None else pad_vectors(inp["X0"], nrhs, n, nt))
    return st, inp
