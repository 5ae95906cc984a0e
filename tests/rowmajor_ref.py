"""Host restatement of the row-major CG loop (csrc/rowmajor.hip; the row-major branches of csrc/solver.cpp) -- pure numpy, no GPU --
on the helpers of cg_step_ref.py and spmv_ref.py.

The loop: set_rhs = spmm_rm_kernel (q = A x0), launch_sub (r = b - q), d = r, rm_dot_kernel (r.r partials), cg_delta0; an iteration =
spmm_rm_kernel with the fused d.q partials, cg_alpha, rm_axpy_dot_kernel, cg_beta, rm_aypx_x_kernel.  The handle keeps its block as
[n][R]; the host state here is (R, n) like cg_step_ref.Steps -- the element-wise expressions do not see the layout, the sums get it
through index maps.

Restated exactly (rowmajor.hip)
-------------------------------
strips: a strip is 16 rows and belongs to one wave.  Work-group wg sweeps for XCD xcd = wg & 7 the strips [sb, se) =
[xcd strips / 8, (xcd + 1) strips / 8) (integer division); its wave `wave` is wave wl = (wg >> 3) 4 + wave of the XCD's W = (nwg >> 3) 4
and takes strips sb + wl, sb + wl + W, ... below se (`strips_of`).
d.q partial of a work-group, from the DEVICE's q: lane (kq, m) of a wave holds the real columns NH m .. NH m + NH - 1; over its strips in
order and the output slots i = 0..3 -- row 4 i + kq of the strip for fp64 (v_mfma_f64_4x4x4 D[b][i][j] @ 16 i + 4 b + j), row 4 kq + i
for fp32 / complex64 (the 16 x 16 tile) -- rows >= n skipped, it adds (double)(x * q rounded in T) per column from +0.  The four kq
meet by xor 16 then xor 32: (v0 + v1) + (v2 + v3); the waves as ((w0 + w1) + w2) + w3.  Complex: per real column the sums
tot(c) of x_c q_c and cross(c) of x_c q_(c ^ 1); re = tot(2t) - tot(2t + 1), im = cross(2t) + cross(2t + 1), unconjugated.  The buffer is
[c][nwg].
rm_dot / rm_axpy_dot / rm_aypx_x: E = 16 / sizeof(T) values per pack; thread g = b 256 + t of G work-groups walks the packs g, g + 256 G,
...; value k of pack i is element i E + k of the [n][R] block (row (i E + k) / R, column (i E + k) % R: always the same column for a thread);
acc[k] += to_acc(vmul(.,.)) from +0.  rm_column_partials: off = R / E, 2 R / E, ... 32: acc += acc of lane ^ off; lanes < R / E hold
columns lane E + k; waves in order; buffer [c][G].  Element-wise: r = vsub(r, vmul(alpha_c, q)); x = vadd(x, vmul(alpha_c, d)) with the
OLD d, d = vadd(vmul(beta_c, d), r) -- cg_step_ref.Ops (uncontracted, complex by components).
scalar launches on those partial counts: cg_delta0 and cg_beta sum with sum_partials_block (thread-strided), cg_alpha with K = plan kdq;
cg_beta divides by the delta the previous step stored.

NOT restated: q
---------------
The rounding inside v_mfma_f64_4x4x4 / v_mfma_f32_16x16x4 is not something the project has measured; a guessed model would make the
test a test of the guess.  q is held (a) EXACTLY where every product and partial sum is an integer the format holds (matrix and x in
{+-1 .. +-8}; `check_q_exact`: any correct order gives the same bits, and a sum that cancels is +0 under round-to-nearest); (b) on random
values within  |q - q_exact| <= gamma_L(u) S + L 2^-63 S,  S = sum_k |a_k||x_k|, L the row's entry count, u = 2^-53 / 2^-24, q_exact in
np.longdouble from the T-rounded inputs (`check_q_bound`).  complex64, per component: 2 L terms, S_re = sum |ar||xr| + |ai||xi|,
S_im = sum |ar||xi| + |ai||xr|.  A row without entries must be exactly +0.  Magnitudes lie in [2^-4, 2^4]: nothing is subnormal.
After that check the restatement continues from the device's q, and everything downstream is bit for bit.

`spmm_model` is NOT a model of the kernel's rounding: it is the longdouble product rounded once to T, with a switch for three mistakes
(`fault`), and exists for tests/test_rowmajor_ref.py alone -- the proof that the two q checks reject those mistakes.
"""
import zlib

import numpy as np

import cg_step_ref as C
import spmv_ref as R

LD = R.LD
DT = {"f32": np.float32, "f64": np.float64, "c64": np.complex64}
WIDTHS = (("f64", 16), ("f64", 32), ("f32", 16), ("f32", 32), ("f32", 64), ("c64", 16), ("c64", 32))
PLAN_KEYS = ("n", "rc", "nh", "tq_fused", "tq_plain", "strips", "nwg_fused", "nwg_plain", "vgrid", "nt_axpy_dot", "nt_aypx_x", "kdq", "krr",
             "paced_fused", "paced_plain", "lead", "n_partials")
TUNE_DEFAULTS = {"spmm_rowmajor": 1, "dev.spmm_wgs": 0, "dev.spmm_lead": 0, "dev.spmm_ynt": -1, "vec_grid": 0, "vec_nt": -1}


class Rules(C.Rules):
    """cg_step_ref.Rules (waves, acc_in_T, contract, ...) and the rules of this loop; a mutation is a Rules with one switch changed"""
    def __init__(self, **kw):
        C.Rules.__init__(self)
        self.row_map_swapped = False    # fp64 lanes walk rows 4 kq + i, fp32 lanes 4 i + kq
        self.round_robin = False        # strip s belongs to wave s % (4 nwg) of the whole grid
        self.partial_wg_major = False   # partials stored at [wg][c]
        self.tree_from_1 = False        # the column shuffle tree starts at off = 1
        self.re_plus = False            # complex d.q: re = tot(2t) + tot(2t + 1)
        self.next_column = False        # the vector kernels take alpha / beta of column c + 1
        self.x_new_d = False            # x += alpha d after d = beta d + r
        for k, v in kw.items():
            assert k in self.__dict__, k
            setattr(self, k, v)


EXACT = Rules()


# ---- the plan a case is written for (host copy of rm_instance / rm_grid_for / rm_vec_grid / the vec_nt rule) -----------------------------
def max_quad(ip):
    ip = np.asarray(ip, dtype=np.int64)
    n = len(ip) - 1
    starts = np.arange(0, n, 4)
    return int((ip[np.minimum(starts + 4, n)] - ip[starts]).max())


def host_plan(ip, dtype, nrhs, knobs=None):
    """the fields of Solver.rowmajor_plan() below the resident capacity of the chip (at most 32 work-groups per XCD: the occupancy
    query, which the host cannot make, does not bind)"""
    knobs = knobs or {}
    dtype = np.dtype(dtype)
    n = len(ip) - 1
    rc = nrhs * (2 if R.is_complex(dtype) else 1)
    mq = max_quad(ip)
    tq = 5 if 0 < mq <= 20 else 8
    strips = -(-n // 16)
    per_xcd = max(1, min(((strips + 7) // 8 + 3) // 4, knobs.get("dev.spmm_wgs", 0) or 32))
    assert per_xcd < 32 or knobs.get("dev.spmm_wgs", 0), "the host cannot predict a grid at the resident capacity"
    nwg = 8 * per_xcd
    W = 4 * per_xcd
    lead_knob = knobs.get("dev.spmm_lead", 0)
    paced = 0 if lead_knob < 0 else sum(1 for x in range(8) if W <= 256 and (x + 1) * strips // 8 - x * strips // 8 >= W)
    E = C.pack_values(dtype)
    vgrid = max(1, min(-(-(n * nrhs) // (256 * E * 4)), knobs.get("vec_grid", 0) or 16 * 2048))
    vnt = knobs.get("vec_nt", -1)
    big = n * nrhs * dtype.itemsize > (96 << 20)
    return {"n": n, "rc": rc, "nh": rc // 16, "tq_fused": tq, "tq_plain": tq, "strips": strips, "nwg_fused": nwg, "nwg_plain": nwg,
            "vgrid": vgrid, "nt_axpy_dot": int((vnt & 2) != 0 if vnt >= 0 else big), "nt_aypx_x": int((vnt & 1) != 0 if vnt >= 0 else big),
            "kdq": 0, "krr": 0, "paced_fused": paced, "paced_plain": paced, "lead": lead_knob if lead_knob > 0 else 3, "n_partials": nwg}


# ---- strips and the d.q partials -------------------------------------------------------------------------------------------------------------
def strips_of(wg, wave, nwg, strips, rules=EXACT):
    if rules.round_robin:
        return list(range(wg * 4 + wave, strips, 4 * nwg))
    xcd = wg & 7
    sb, se = xcd * strips // 8, (xcd + 1) * strips // 8
    W = (nwg >> 3) * 4
    return list(range(sb + (wg >> 3) * 4 + wave, se, W))


def wave_steps(nwg, strips):
    """strips per wave, (nwg, 4)"""
    return np.array([[len(strips_of(wg, w, nwg, strips)) for w in range(4)] for wg in range(nwg)])


def lane_rows(n, nwg, f64, rules=EXACT):
    """rows in the order lane (kq, .) of (wg, wave) adds them: (idx, mask), each (nwg * 16, L); unit = (wg * 4 + wave) * 4 + kq"""
    strips = -(-n // 16)
    quad_major = f64 != rules.row_map_swapped          # slot i is row 4 i + kq
    seqs = []
    for wg in range(nwg):
        for wave in range(4):
            ss = strips_of(wg, wave, nwg, strips, rules)
            for kq in range(4):
                rows = [16 * s + (4 * i + kq if quad_major else 4 * kq + i) for s in ss for i in range(4)]
                seqs.append([r for r in rows if r < n])
    L = max(1, max(len(s) for s in seqs))
    idx = np.zeros((len(seqs), L), dtype=np.int64)
    mask = np.zeros((len(seqs), L), dtype=bool)
    for u, s in enumerate(seqs):
        idx[u, :len(s)] = s
        mask[u, :len(s)] = True
    return idx, mask


def _waves(w, rules):
    """w (..., 4) wave sums -> (...)"""
    if rules.waves == "inorder":
        return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def _stored(p, rules):
    """p (columns, groups) as the launches that READ the buffer see it ([c][groups]) when it was written under `rules`"""
    if rules.partial_wg_major:
        return np.ascontiguousarray(p.T).reshape(p.shape)
    return p


def dq_terms(d, q, dtype, rules=EXACT):
    """per real column the products a lane adds: (tot, cross or None), each (RC, n), double (T under acc_in_T)"""
    dtype = np.dtype(dtype)
    nrhs, n = d.shape
    with np.errstate(all="ignore"):
        if not R.is_complex(dtype):
            t = d * q
            return (t if rules.acc_in_T else t.astype(np.float64)), None
        dr, di = R._parts(d, dtype)
        qr, qi = R._parts(q, dtype)
        tot = np.empty((2 * nrhs, n), np.float32)
        cross = np.empty((2 * nrhs, n), np.float32)
        tot[0::2], tot[1::2] = dr * qr, di * qi
        cross[0::2], cross[1::2] = dr * qi, di * qr
    if rules.acc_in_T:
        return tot, cross
    return tot.astype(np.float64), cross.astype(np.float64)


def dq_partials(d, q, dtype, nwg, rules=EXACT):
    """the fused d.q partials of spmm_rm_kernel: d, q (nrhs, n) -> (nrhs, nwg) in the accumulator type"""
    dtype = np.dtype(dtype)
    nrhs, n = d.shape
    idx, mask = lane_rows(n, nwg, dtype == np.float64, rules)
    tot, cross = dq_terms(d, q, dtype, rules)

    def sweep(t):
        acc = np.zeros((t.shape[0], idx.shape[0]), t.dtype)
        with np.errstate(all="ignore"):
            for j in range(idx.shape[1]):
                acc = np.where(mask[:, j], acc + t[:, idx[:, j]], acc)
            a = acc.reshape(t.shape[0], nwg, 4, 4)
            w = (a[..., 0] + a[..., 1]) + (a[..., 2] + a[..., 3])          # xor 16, then xor 32
            return _waves(w, rules).astype(np.float64)
    with np.errstate(all="ignore"):
        if cross is None:
            return _stored(sweep(tot), rules)
        T_, X_ = sweep(tot), sweep(cross)
        out = np.empty((nrhs, nwg), np.complex128)
        out.real = (T_[0::2] + T_[1::2]) if rules.re_plus else (T_[0::2] - T_[1::2])
        out.imag = X_[0::2] + X_[1::2]
    return _stored(out, rules)


def row_groups(n, nwg):
    """the work-group whose d.q partial row i is added to"""
    strips = -(-n // 16)
    g = np.empty(n, dtype=np.int64)
    for wg in range(nwg):
        for wave in range(4):
            for s in strips_of(wg, wave, nwg, strips):
                g[16 * s:min(16 * s + 16, n)] = wg
    return g


def dq_integer(d, q, dtype, nwg):
    """the d.q partials of integer-valued d and q in integer arithmetic (no order to restate: the rows of a work-group, nothing else)"""
    dtype = np.dtype(dtype)
    nrhs, n = d.shape
    g = row_groups(n, nwg)
    dr, di, qr, qi = (np.rint(v).astype(np.int64) for v in (np.real(d), np.imag(d), np.real(q), np.imag(q)))
    assert np.array_equal(dr + 1j * di, d.astype(np.complex128)) and np.array_equal(qr + 1j * qi, q.astype(np.complex128))
    re, im = np.zeros((nrhs, nwg), np.int64), np.zeros((nrhs, nwg), np.int64)
    for r in range(nrhs):
        np.add.at(re[r], g, dr[r] * qr[r] - di[r] * qi[r])
        np.add.at(im[r], g, dr[r] * qi[r] + di[r] * qr[r])
    big = max(np.abs(dr * qr).max(initial=0), np.abs(di * qi).max(initial=0), np.abs(dr * qi).max(initial=0), np.abs(di * qr).max(initial=0))
    assert big < 2 ** (24 if R.real_type(dtype) is np.float32 else 53), "a product of d and q is rounded in T"
    if R.is_complex(dtype):
        out = np.empty((nrhs, nwg), np.complex128)
        out.real, out.imag = re, im
        return out
    return re.astype(np.float64)


# ---- the partials of the rm_* vector kernels --------------------------------------------------------------------------------------------------
def rm_partials(t, dtype, G, rules=EXACT):
    """rm_column_partials over the terms t (nrhs, n) of the [n][nrhs] block: (nrhs, G)"""
    nrhs, n = t.shape
    E = C.pack_values(dtype)
    S = G * 256
    flat = np.ascontiguousarray(t.T).reshape(-1)          # element (i, c) at i nrhs + c
    npack = flat.size // E
    assert npack * E == flat.size and nrhs % E == 0 and (256 * E) % nrhs == 0
    J = max(1, -(-npack // S))
    body = np.zeros(J * S * E, t.dtype)
    body[:flat.size] = flat
    live = (np.arange(J * S) < npack).reshape(J, S)
    body = body.reshape(J, S, E)
    acc = np.zeros((S, E), t.dtype)
    with np.errstate(all="ignore"):
        for j in range(J):
            acc = np.where(live[j][:, None], acc + body[j], acc)
        acc = acc.reshape(G, 4, 64, E)
        lane = np.arange(64)
        groups = nrhs // E
        off = 1 if rules.tree_from_1 else groups
        while off < 64:
            acc = acc + acc[:, :, lane ^ off, :]
            off *= 2
        red = acc[:, :, :groups, :].reshape(G, 4, nrhs)
        tot = _waves(np.moveaxis(red, 1, -1), rules)      # (G, nrhs)
    acct = C.acc_type(dtype)
    return _stored(np.ascontiguousarray(tot.T).astype(acct), rules)


# ---- the loop ---------------------------------------------------------------------------------------------------------------------------------
class RmSteps:
    """set_rhs and iterations of one row-major handle.  plan: Solver.rowmajor_plan().  q is GIVEN (the device's, or a model's): the
    restatement starts behind the SpMM.  State as cg_step_ref.Steps: x, r, d, q (nrhs, n); part_dq (nrhs, nwg_fused), part_rr
    (nrhs, vgrid); alpha, beta, delta (nrhs,); it; history"""
    def __init__(self, dtype, nrhs, plan, rules=EXACT):
        self.dtype, self.nrhs, self.plan, self.rules = np.dtype(dtype), nrhs, dict(plan), rules
        self.n = plan["n"]
        self.ops = C.Ops(dtype, rules)
        self.alpha = self.beta = self.part_dq = None

    def _rr(self):
        return rm_partials(self.ops.terms(self.r, self.r), self.dtype, self.plan["vgrid"], self.rules)

    def _col(self, s):
        return np.roll(s, -1) if self.rules.next_column else s

    def set_rhs(self, b, x0, q):
        n, nrhs, dt = self.n, self.nrhs, self.dtype
        self.b = np.asarray(b, dtype=dt).reshape(nrhs, n)
        self.x = np.zeros((nrhs, n), dt) if x0 is None else np.array(x0, dtype=dt).reshape(nrhs, n)
        self.q = np.array(q, dtype=dt).reshape(nrhs, n)
        self.r = self.ops.sub(self.b, self.q)
        self.d = self.r.copy()
        self.part_rr = self._rr()
        self.delta = C.from_acc(C.prologue_sum(self.part_rr, 1024, 0, self.rules), dt)
        self.history = [self.delta.copy()]
        self.it = 0
        return self

    def iterate(self, q):
        dt = self.dtype
        self.q = np.array(q, dtype=dt).reshape(self.nrhs, self.n)
        self.part_dq = dq_partials(self.d, self.q, dt, self.plan["nwg_fused"], self.rules)
        self.alpha = C.alpha_value(self.part_dq, self.delta, {"fold": 0, "alpha2": 0, "kdq": self.plan["kdq"]}, dt, self.rules)
        self.it += 1
        al = self._col(self.alpha)
        self.r = self.ops.axmy(self.r, al, self.q)
        self.part_rr = self._rr()
        dn = C.from_acc(C.prologue_sum(self.part_rr, 1024, 0, self.rules), dt)
        self.beta = C.quotient(dn, self.delta, dt, self.rules)
        self.delta = dn
        self.history.append(dn)
        bt = self._col(self.beta)
        if self.rules.x_new_d:
            self.d = self.ops.aypx(bt, self.d, self.r)
            self.x = self.ops.axpy(self.x, al, self.d)
        else:
            self.x = self.ops.axpy(self.x, al, self.d)
            self.d = self.ops.aypx(bt, self.d, self.r)
        return self

    def state(self):
        out = {"x": self.x, "r": self.r, "d": self.d, "q": self.q, "part_rr": self.part_rr, "delta": self.delta,
               "iter": np.array([self.it]), "history": np.stack(self.history)}
        if self.alpha is not None:
            out.update(part_dq=self.part_dq, alpha=self.alpha, beta=self.beta)
        return out


def differing(a, b):
    """names of the state entries whose bits differ"""
    return [k for k in a if not R.bit_equal(np.asarray(a[k]), np.asarray(b[k]))]


# ---- q: the two checks ------------------------------------------------------------------------------------------------------------------------
def _rows(ip):
    return np.repeat(np.arange(len(ip) - 1), np.diff(np.asarray(ip, dtype=np.int64)))


def q_integer(ip, ix, da, x, dtype):
    """A x in integer arithmetic for integer-valued inputs: x (nrhs, n) -> (nrhs, n) of dtype"""
    dtype = np.dtype(dtype)
    rows = _rows(ip)
    nrhs, n = x.shape
    ar, ai = (np.rint(v).astype(np.int64) for v in (np.real(da), np.imag(da)))
    xr, xi = (np.rint(v).astype(np.int64) for v in (np.real(x), np.imag(x)))
    assert np.array_equal(ar + 1j * ai, np.asarray(da, dtype=np.complex128)) and np.array_equal(xr + 1j * xi, np.asarray(x, dtype=np.complex128))
    re = np.zeros((nrhs, n), np.int64)
    im = np.zeros((nrhs, n), np.int64)
    for r in range(nrhs):
        np.add.at(re[r], rows, ar * xr[r, ix] - ai * xi[r, ix])
        np.add.at(im[r], rows, ar * xi[r, ix] + ai * xr[r, ix])
    # every partial sum of moduli below the format's integer range: any order is exact
    absum = np.zeros(n, np.int64)
    np.add.at(absum, rows, np.abs(ar) + np.abs(ai))
    assert int(absum.max(initial=0)) * int(max(np.abs(xr).max(initial=0), np.abs(xi).max(initial=0))) * 2 < 2 ** (24 if R.real_type(dtype) is np.float32 else 53)
    if R.is_complex(dtype):
        return R._join(re.astype(np.float32), im.astype(np.float32), dtype)
    assert not im.any()
    return re.astype(dtype)


def check_q_exact(got, ip, ix, da, x, dtype, label=""):
    want = q_integer(ip, ix, da, x, dtype)
    got = np.asarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape, (label, got.dtype, got.shape)
    bad = np.argwhere((R.bits(got) != R.bits(want)).reshape(want.shape + (-1,)).any(axis=-1))
    assert not len(bad), f"{label}: {len(bad)} of {want.size} values of q differ from integer arithmetic, first (rhs, row) {bad[0].tolist()}: " \
                         f"{got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}"


def q_reference(ip, ix, da, x, dtype):
    """components of A x in longdouble from the T-rounded inputs, the sums S of the moduli and the terms per row: [(exact, S, terms)]"""
    dtype = np.dtype(dtype)
    rows = _rows(ip)
    nrhs, n = x.shape
    da, x = np.asarray(da, dtype=dtype), np.asarray(x, dtype=dtype)
    L = np.diff(np.asarray(ip, dtype=np.int64)).astype(LD)
    ar, xr = np.real(da).astype(LD), np.real(x).astype(LD)
    if not R.is_complex(dtype):
        ex, S = np.zeros((nrhs, n), LD), np.zeros((nrhs, n), LD)
        for r in range(nrhs):
            np.add.at(ex[r], rows, ar * xr[r, ix])
            np.add.at(S[r], rows, np.abs(ar * xr[r, ix]))
        return [(ex, S, L)]
    ai, xi = np.imag(da).astype(LD), np.imag(x).astype(LD)
    re, im, Sr, Si = (np.zeros((nrhs, n), LD) for _ in range(4))
    for r in range(nrhs):
        a, b = xr[r, ix], xi[r, ix]
        np.add.at(re[r], rows, ar * a - ai * b)
        np.add.at(im[r], rows, ar * b + ai * a)
        np.add.at(Sr[r], rows, np.abs(ar * a) + np.abs(ai * b))
        np.add.at(Si[r], rows, np.abs(ar * b) + np.abs(ai * a))
    return [(re, Sr, 2 * L), (im, Si, 2 * L)]


def check_q_bound(got, ip, ix, da, x, dtype, label=""):
    """every value of q inside gamma_L(u) S + L 2^-63 S of the longdouble product (module docstring); rows without entries exactly +0.
    Returns the largest error / bound"""
    dtype = np.dtype(dtype)
    assert np.finfo(LD).nmant >= 63
    got = np.asarray(got)
    assert got.dtype == dtype, (label, got.dtype)
    u = R.unit_roundoff(dtype)
    comps = [np.real(got), np.imag(got)] if R.is_complex(dtype) else [got]
    empty = np.diff(np.asarray(ip, dtype=np.int64)) == 0
    z = got[:, empty]
    assert not R.bits(z).any(), f"{label}: a row without entries is not +0"
    worst = 0.0
    for g, (ex, S, L) in zip(comps, q_reference(ip, ix, da, x, dtype)):
        bound = (R.gamma(L, u) + L * LD(2) ** -63) * S
        err = np.abs(g.astype(LD) - ex)
        with np.errstate(all="ignore"):
            ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))
        worst = max(worst, float(ratio.max(initial=0)))
    print(f"{label}: largest |q - q_exact| / bound = {worst:.3g}")
    assert worst <= 1.0, f"{label}: q outside the format's bound: error / bound = {worst:.3g}"
    return worst


def spmm_model(ip, ix, da, x, dtype, tq=8, fault=None):
    """the longdouble product rounded once to T -- a stand-in for the device's q on the host (module docstring) -- or that product with
    one mistake: "neighbour_row" (the last entry of the first row of every quad credited to the quad's next row), "drop_round" (the
    entries of a quad beyond the 4 tq slots of its first round dropped), "row_map" (rows 4 a + b and 4 b + a of a strip exchanged)"""
    dtype = np.dtype(dtype)
    ip = np.asarray(ip, dtype=np.int64)
    n = len(ip) - 1
    rows = _rows(ip)
    keep = np.ones(len(ix), dtype=bool)
    if fault == "neighbour_row":
        rows = rows.copy()
        for r0 in range(0, n - 1, 4):
            if ip[r0 + 1] > ip[r0]:
                rows[ip[r0 + 1] - 1] = r0 + 1
    if fault == "drop_round":
        for r0 in range(0, n, 4):
            keep[ip[r0] + 4 * tq:ip[min(r0 + 4, n)]] = False
    ip2 = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows[keep], minlength=n), out=ip2[1:])
    order = np.argsort(rows[keep], kind="stable")
    ix2, da2 = np.asarray(ix)[keep][order], np.asarray(da, dtype=dtype)[keep][order]
    ref = q_reference(ip2, ix2, da2, np.asarray(x, dtype=dtype), dtype)
    Rt = R.real_type(dtype)
    out = R._join(ref[0][0].astype(Rt), ref[1][0].astype(Rt) if len(ref) > 1 else None, dtype)
    if fault == "row_map":
        i = np.arange(n)
        l = i % 16
        j = i - l + 4 * (l % 4) + l // 4
        j = np.where(j < n, j, i)
        out = out[:, j]
    return out


# ---- inputs shared by the host proof and the device module --------------------------------------------------------------------------------
def values(rng, shape, dtype, kind):
    """kind "int": {+-1 .. +-8}; "rand": magnitudes 2^[-4, 4], random signs (both components of a complex value)"""
    Rt = R.real_type(dtype)

    def one():
        if kind == "int":
            return (rng.integers(1, 9, shape) * rng.choice([-1, 1], shape)).astype(Rt)
        return (np.exp2(rng.uniform(-4.0, 4.0, shape)) * rng.choice([-1.0, 1.0], shape)).astype(Rt)
    if R.is_complex(dtype):
        return R._join(one(), one(), dtype)
    return one().astype(dtype)


def _csr(n, rows, cols):
    ip = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows, minlength=n), out=ip[1:])
    return ip, np.asarray(cols, dtype=np.int32)


def grid_pattern(N, nine):
    """5- or 9-point stencil on an N x N grid, the entries of a row in stencil order"""
    offs = [(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1) if nine or a == 0 or b == 0]
    rows, cols = [], []
    for i in range(N):
        for j in range(N):
            for a, b in offs:
                if 0 <= i + a < N and 0 <= j + b < N:
                    rows.append(i * N + j)
                    cols.append((i + a) * N + j + b)
    return _csr(N * N, np.asarray(rows), cols)


def counted_pattern(rng, counts):
    """rows of the given entry counts, distinct columns in random (unsorted) order"""
    n = len(counts)
    cols = np.concatenate([rng.choice(n, size=int(c), replace=False) for c in counts] + [np.zeros(0, dtype=np.int64)])
    return _csr(n, np.repeat(np.arange(n), counts), cols)


def random_pattern():
    """1543 rows: unsorted columns, empty rows, an empty quad (rows 40-43), an empty strip (rows 160-175), a quad of exactly 32 entries
    (rows 200-203) and one of 33 (rows 300-303), one row of 77 entries (row 777)"""
    rng = np.random.default_rng(1543)
    n = 1543
    counts = np.minimum(rng.poisson(5, n), 7)          # (a quad of 4 x 7 = 28 entries stays inside one round of TQ 8)
    counts[rng.choice(n, n // 7, replace=False)] = 0
    counts[40:44] = 0
    counts[160:176] = 0
    counts[200:204] = 8
    counts[300:304] = (9, 8, 8, 8)
    counts[777] = 77
    return counted_pattern(rng, counts)


def small_pattern(n):
    rng = np.random.default_rng(n)
    return counted_pattern(rng, np.minimum(rng.integers(0, 5, n) + (np.arange(n) == 0), n))


SYSTEMS = {"grid5": lambda: grid_pattern(39, False), "grid9": lambda: grid_pattern(39, True), "random": random_pattern}
SMALL_N = (1, 15, 16, 17, 100, 129)
_PATTERNS = {}


def pattern(name):
    if name not in _PATTERNS:
        _PATTERNS[name] = SYSTEMS[name]() if name in SYSTEMS else small_pattern(int(name))
    return _PATTERNS[name]


def case_seed(*parts):
    return zlib.crc32("-".join(str(p) for p in parts).encode())


def spmm_inputs(name, dt, nrhs, kind):
    """(ip, ix, da, X (nrhs, n)) of an SpMM case"""
    ip, ix = pattern(name)
    rng = np.random.default_rng(case_seed("spmm", name, dt, nrhs, kind))
    return ip, ix, values(rng, len(ix), DT[dt], kind), values(rng, (nrhs, len(ip) - 1), DT[dt], kind)


def loop_inputs(name, dt, nrhs, kind):
    """(ip, ix, da, B, X0 or None) of a loop case: "int" -- integer matrix and B, no first guess; "rand" -- random matrix, B and X0"""
    ip, ix = pattern(name)
    n = len(ip) - 1
    rng = np.random.default_rng(case_seed("loop", name, dt, nrhs, kind))
    da = values(rng, len(ix), DT[dt], kind)
    B = values(rng, (nrhs, n), DT[dt], kind)
    return ip, ix, da, B, (values(rng, (nrhs, n), DT[dt], "rand") if kind == "rand" else None)
