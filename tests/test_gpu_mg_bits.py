"""What a handle's multigrid hierarchy holds, and its whole V-cycle, BIT FOR BIT (csrc/multigrid.hip, csrc/amg.hip,
csrc/multigrid_setup.cpp; include/cgamd.h states the orders).  Every comparison starts from what the DEVICE holds one step earlier --
the level matrix above, the device's own dinv, lmax, coefficients and maps -- so each piece is held on its own:

  * dinv = T(1 / the diagonal summed in stored order in double), Smith's division for the complex types; +0 on the padding rows;
  * lmax, for the real types, = max_i |dinv_i| * (sum_j |a_ij| in stored order in double) (complex: 1e-13, hypot is not specified to
    the bit); c0, c1 = mg_ref.chebyshev_coefficients of that lmax;
  * the member lists = the ascending preimages of the map, -1 behind the last;
  * every level's matrix = mg_ref.galerkin / amg_ref.galerkin of the device's matrix of the level above;
  * the product of every level as the cycle launches it = the spmv_ref restatement of the family cgamd_last_spmv_form reports;
  * z = mg_apply(r) = mg_kernel_ref.cycle_bits fed with all of the above."""
import numpy as np
import pytest
import scipy.sparse as sp

import amg_ref
import mg_kernel_ref as K
import mg_ref
import spmv_ref as R
from canary_buffers import Embedded

pytestmark = pytest.mark.gpu
ALL = [np.float32, np.float64, np.complex64, np.complex128]
LANE_FAMILIES = ("rowblock", "vc", "vcp", "spmm", "rowcode", "rowpair")       # one lane per row: a row is added up in stored order


def parts(A, dtype):
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(dtype)


def solver(pkg, ctx, A, dtype, nrhs=1):
    ip, ix, da = parts(A, dtype)
    return pkg.Solver(ctx, A.shape[0], len(ix), da, ip, ix, nrhs)


def as_type(A, dtype):
    return sp.csr_matrix(A * (1.0 + 0.05j)) if np.dtype(dtype).kind == "c" else sp.csr_matrix(A)


def rhs(n, dtype, nrhs, seed=11):
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((nrhs, n))
    if np.dtype(dtype).kind == "c":
        B = B + 1j * rng.standard_normal((nrhs, n))
    return B.astype(dtype)


def level_form(pkg, ctx, s, l, st, dtype, x=None):
    """run the level's product on x (zeros by default) inside canary buffers: (what last_spmv_form reports, w as (nrhs, n))"""
    nrhs, n, ld = s.n_rhs, st["n"], st["ld"]
    xs = Embedded(pkg, ctx, np.zeros((nrhs, n), dtype) if x is None else x, ld)
    ws = Embedded(pkg, ctx, np.empty((nrhs, n), dtype), ld, blank=True)
    s.mg_level_spmv(l, xs.ptr, ws.ptr)
    form = s.last_spmv_form()
    got = ws.buf.get()
    lanes = got[ws.start:ws.start + nrhs * ld * np.dtype(dtype).itemsize].view(dtype).reshape(nrhs, ld)[:, :n].copy()
    ws.check(f"level {l}: w (nothing at or behind row {n} of a column, nothing around the array)", lanes)
    xs.check(f"level {l}: x is only read")
    return form, lanes


def spmv_rule(form, l):
    assert form["family"] in LANE_FAMILIES + ("chunked",), f"level {l} runs the {form['family']} kernel, which has no restatement to the bit"
    return ("chunked", form["width"]) if form["family"] == "chunked" else ("lane",)


def device_hierarchy(pkg, ctx, s, dtype):
    """everything the cycle uses, read back from the device, as mg_kernel_ref.cycle_bits takes it; (levels, infos, forms)"""
    infos = s.mg_levels()
    out, forms = [], []
    for l, info in enumerate(infos):
        st = s.mg_level_state(l, 0)
        assert st["nu"] == info["rows"] and st["n"] >= st["nu"] and st["ld"] >= st["n"]
        ip, ix, da = s.mg_level_matrix(l)
        last = l == len(infos) - 1
        agg = members = None
        if not last:
            agg, nc = s.mg_aggregates(l)
            assert nc == infos[l + 1]["rows"]
            members = s.mg_level_state(l, 4) if st["algebraic"] else K.members_of(agg, nc)
        form, _ = level_form(pkg, ctx, s, l, st, dtype)
        forms.append(form)
        c0, c1 = s.mg_level_state(l, 2), s.mg_level_state(l, 3)
        assert len(c0) == len(c1) == st["steps"]
        out.append(K.level(ip, ix, da, s.mg_level_state(l, 1), c0, c1, n=st["n"], nu=st["nu"], ld=st["ld"], members=members, agg=agg,
                           spmv=spmv_rule(form, l)))
    return out, infos, forms


def describe(forms):
    return ", ".join(f"level {l}: {f['family']}" + (f" x{f['width']}" if f["family"] in ("chunked", "spmm") else "") for l, f in enumerate(forms))


# ---- per-level state ------------------------------------------------------------------------------------------------------------------------
def check_level_state(s, levels, infos, dtype, smooth_steps):
    nl = len(levels)
    for l, (L, info) in enumerate(zip(levels, infos)):
        last = l == nl - 1
        nu = L["nu"]
        ip, ix, da = L["ip"][:nu + 1], L["ix"], L["da"]
        st = s.mg_level_state(l, 0)
        assert st["steps"] == (mg_ref.COARSEST_STEPS if last else smooth_steps)
        assert l == 0 or st["n"] == nu                                            # only level 0 carries padding rows
        want = K.dinv_bits(ip, ix, da, dtype)
        assert L["dinv"].dtype == np.dtype(dtype) and L["dinv"].size == L["n"]
        assert R.bit_equal(L["dinv"][:nu], want), f"level {l}: dinv"
        assert not R.bits(L["dinv"][nu:]).any(), "the padding rows of dinv are +0"
        if np.dtype(dtype).kind == "c":
            W = np.complex128
            absA = sp.csr_matrix((np.abs(da.astype(W)), ix, ip), shape=(nu, nu))
            lm = float(np.max(np.abs(L["dinv"][:nu].astype(W)) * np.asarray(absA @ np.ones(nu))))
            assert abs(info["lmax"] - lm) <= 1e-13 * lm
        else:
            assert info["lmax"] == K.lmax_real(ip, da, L["dinv"]), f"level {l}: lmax"
        c0, c1 = mg_ref.chebyshev_coefficients(info["lmax"], mg_ref.KAPPA_COARSEST if last else mg_ref.KAPPA_SMOOTH, st["steps"])
        assert R.bit_equal(np.asarray(L["c0"], np.float64), np.asarray(c0)) and R.bit_equal(np.asarray(L["c1"], np.float64), np.asarray(c1)), l
        if not last:
            nc = levels[l + 1]["nu"]
            assert L["members"].shape == (nc, 8)
            assert np.array_equal(L["members"], K.members_of(L["agg"], nc)), f"level {l}: member lists"


STATE_CASES = [("grid", (13, 11, 9)), ("grid", (9, 7, 1)), ("amg", (13, 11, 9))]


@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("kind,dims", STATE_CASES, ids=[f"{k}-{'x'.join(map(str, d))}" for k, d in STATE_CASES])
def test_level_state(pkg, gpu, kind, dims, dtype):
    ctx = gpu[0]
    A = as_type(mg_ref.variable7(*dims), dtype)
    s = solver(pkg, ctx, A, dtype, 2)
    for steps in (1, 3):
        opts = {"min_rows": 8, "smooth_steps": steps}
        s.set_preconditioner(("multigrid", dims, opts) if kind == "grid" else ("amg", opts))
        levels, infos, forms = device_hierarchy(pkg, ctx, s, dtype)
        assert len(levels) >= 3
        check_level_state(s, levels, infos, dtype, steps)
        last = len(levels) - 1
        with pytest.raises(pkg.CgAmdError):
            s.mg_level_state(last, 4)                  # the coarsest level has no aggregates
        if kind == "grid":
            with pytest.raises(pkg.CgAmdError):
                s.mg_level_state(0, 4)                 # a grid hierarchy stores no member lists
        for bad in ((len(levels), 0), (-1, 1), (0, 5)):
            with pytest.raises(pkg.CgAmdError):
                s.mg_level_state(*bad)
    s.set_preconditioner(None)
    with pytest.raises(pkg.CgAmdError):
        s.mg_level_state(0, 0)
    s.close()


# ---- Galerkin values ------------------------------------------------------------------------------------------------------------------------
def same_matrix(got, want, label):
    ip, ix, da = got
    assert np.array_equal(ip, want.indptr) and np.array_equal(ix, want.indices), f"{label}: pattern"
    assert R.bit_equal(da, want.data), f"{label}: {int(np.count_nonzero(R.bits(da) != R.bits(want.data)))} value lanes differ"


def system(kind, dims, dtype):
    A = mg_ref.variable7(*dims) if kind == "var7" else mg_ref.stencil27(*dims)
    return as_type(A, dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.complex64])
@pytest.mark.parametrize("kind", ["var7", "stencil27"])
@pytest.mark.parametrize("dims", [(7, 6, 5), (9, 7, 1), (13, 1, 1)])
def test_galerkin_bits_grid(pkg, gpu, dims, kind, dtype):
    ctx = gpu[0]
    s = solver(pkg, ctx, system(kind, dims, dtype), dtype)
    s.set_preconditioner(("multigrid", dims, {"min_rows": 2}))
    infos = s.mg_levels()
    assert len(infos) >= 3
    above, d = s.mg_level_matrix(0), dims
    for l in range(1, len(infos)):
        fine = sp.csr_matrix((above[2], above[1], above[0]), shape=(infos[l - 1]["rows"],) * 2)
        want, _ = mg_ref.galerkin(fine, d, dtype)
        above, d = s.mg_level_matrix(l), mg_ref.coarse_dims(d)
        same_matrix(above, want, f"level {l} {dims} {kind}")
    s.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.complex64])
def test_galerkin_bits_more_than_1024_coarse_rows(pkg, gpu, dtype):
    """24 x 22 x 20: 1320 coarse rows, so the scan's threads sum chunks of two counts and the last chunks are ragged or empty; the
    pointers and columns are compared as well as the values"""
    ctx = gpu[0]
    dims = (24, 22, 20)
    s = solver(pkg, ctx, system("var7", dims, dtype), dtype)
    s.set_preconditioner(("multigrid", dims, {"min_rows": 1000}))
    infos = s.mg_levels()
    assert [L["rows"] for L in infos] == [10560, 1320, 180]
    above, d = s.mg_level_matrix(0), dims
    for l in (1, 2):
        fine = sp.csr_matrix((above[2], above[1], above[0]), shape=(infos[l - 1]["rows"],) * 2)
        want, _ = mg_ref.galerkin(fine, d, dtype)
        above, d = s.mg_level_matrix(l), mg_ref.coarse_dims(d)
        same_matrix(above, want, f"level {l}")
    s.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.complex64])
@pytest.mark.parametrize("dims", [(7, 6, 5), (9, 7, 1), (13, 1, 1)])
def test_galerkin_bits_algebraic_one_pass(pkg, gpu, dims, dtype):
    """passes = 1: a level is one product through the device's own map"""
    ctx = gpu[0]
    s = solver(pkg, ctx, system("var7", dims, dtype), dtype)
    s.set_preconditioner(("amg", {"passes": 1, "min_rows": 2}))
    infos = s.mg_levels()
    assert len(infos) >= 2
    above = s.mg_level_matrix(0)
    for l in range(1, len(infos)):
        fine = sp.csr_matrix((above[2], above[1], above[0]), shape=(infos[l - 1]["rows"],) * 2)
        agg, nc = s.mg_aggregates(l - 1)
        want, _ = amg_ref.galerkin(fine, agg, nc, dtype)
        above = s.mg_level_matrix(l)
        same_matrix(above, want, f"level {l} {dims}")
    s.close()


INTEGER_SYSTEMS = {"lap": lambda: mg_ref.laplace3d(7, 6, 5), "stencil27": lambda: mg_ref.stencil27(7, 6, 5), "z100": lambda: amg_ref.zaniso(9, 7, 6)}


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.complex64])
@pytest.mark.parametrize("passes", [2, 3])
@pytest.mark.parametrize("kind", list(INTEGER_SYSTEMS))
def test_galerkin_bits_algebraic_more_passes(pkg, gpu, kind, passes, dtype):
    """2 and 3 passes on the integer systems of test_maps_exact, level by level from the DEVICE's matrix: the restated passes compose
    to the device's map, and the last kept product, rounded once per pass, is the device's next level"""
    ctx = gpu[0]
    A = as_type(INTEGER_SYSTEMS[kind](), dtype)
    s = solver(pkg, ctx, A, dtype)
    s.set_preconditioner(("amg", {"passes": passes, "min_rows": 2}))
    infos = s.mg_levels()
    assert len(infos) >= 3
    above = s.mg_level_matrix(0)
    for l in range(1, len(infos)):
        fine = sp.csr_matrix((above[2], above[1], above[0]), shape=(infos[l - 1]["rows"],) * 2)
        built = amg_ref.coarsen(fine, np.dtype(dtype), passes, 0.25)
        assert built is not None
        agg, nc = s.mg_aggregates(l - 1)
        assert nc == built[1].shape[0] and np.array_equal(agg, built[0]), f"level {l}: the restated passes do not compose to the device's map"
        above = s.mg_level_matrix(l)
        same_matrix(above, built[1], f"level {l} {kind} passes {passes}")
    s.close()


# ---- the product of every level ---------------------------------------------------------------------------------------------------------------
PRODUCT_CASES = [("grid", (13, 11, 9)), ("grid", (16, 16, 16)), ("amg", (13, 11, 9))]


@pytest.mark.parametrize("nrhs", [1, 3])
@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("kind,dims", PRODUCT_CASES, ids=[f"{k}-{'x'.join(map(str, d))}" for k, d in PRODUCT_CASES])
def test_level_product(pkg, gpu, kind, dims, dtype, nrhs):
    ctx = gpu[0]
    s = solver(pkg, ctx, system("var7", dims, dtype), dtype, nrhs)
    s.set_preconditioner(("multigrid", dims, {"min_rows": 32}) if kind == "grid" else ("amg", {"min_rows": 32}))
    levels, infos, _ = device_hierarchy(pkg, ctx, s, dtype)
    forms = []
    for l, L in enumerate(levels):
        x = rhs(L["n"], dtype, nrhs, seed=3 + l)
        form, w = level_form(pkg, ctx, s, l, s.mg_level_state(l, 0), dtype, x)
        forms.append(form)
        L = dict(L, spmv=spmv_rule(form, l))
        want = K.product(L, x, dtype)
        bad = np.argwhere(R.bits(w).reshape(nrhs, L["n"], -1) != R.bits(want).reshape(nrhs, L["n"], -1))
        assert bad.size == 0, f"level {l} ({form['family']}): {len(bad)} lanes differ, the first in (column, row) {bad[0][:2].tolist()}"
    print(f"  {kind} {dims} {np.dtype(dtype).name} x{nrhs}: {describe(forms)}")
    s.close()


# ---- the whole cycle --------------------------------------------------------------------------------------------------------------------------
def check_cycle_bits(pkg, ctx, s, dtype, omega, label):
    levels, infos, forms = device_hierarchy(pkg, ctx, s, dtype)
    n, n0, nrhs = infos[0]["rows"], levels[0]["n"], s.n_rhs
    B = rhs(n, dtype, nrhs)
    z = s.mg_apply(B.reshape(-1)).reshape(nrhs, n)
    r = np.zeros((nrhs, n0), dtype)
    r[:, :n] = B
    want = K.cycle_bits(levels, r, omega, dtype)
    assert not R.bits(want[:, n:]).any(), "z is +0 on the padding rows"
    bad = np.argwhere(R.bits(z).reshape(nrhs, n, -1) != R.bits(want[:, :n]).reshape(nrhs, n, -1))
    print(f"  {label} {np.dtype(dtype).name} x{nrhs}: {len(levels)} levels; {describe(forms)}")
    assert bad.size == 0, f"{label}: {len(bad)} lanes of z differ from the restated chain, the first in (column, row) {bad[0][:2].tolist()}"


GRID_OPTS = [{"min_rows": 32}, {"min_rows": 32, "smooth_steps": 2, "over_correction": 1.0}, {"min_rows": 32, "smooth_steps": 3},
             {"min_rows": 5000}, {"min_rows": 5000, "over_correction": 1.0}]


def set_mg(s, m):
    """set the preconditioner; returns the over-correction it was given (0 or absent: 1.6)"""
    s.set_preconditioner(m)
    return float(m[-1].get("over_correction", 0.0) or 1.6)


@pytest.mark.parametrize("nrhs", [1, 3])
@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("dims", [(13, 11, 9), (16, 16, 16), (9, 7, 1)])
def test_cycle_bits_grid(pkg, gpu, dims, dtype, nrhs):
    ctx = gpu[0]
    s = solver(pkg, ctx, system("var7", dims, dtype), dtype, nrhs)
    for opts in GRID_OPTS:
        omega = set_mg(s, ("multigrid", dims, opts))
        want_levels = 1 if opts["min_rows"] == 5000 else (4 if dims != (9, 7, 1) else 2)
        assert len(s.mg_levels()) == want_levels
        check_cycle_bits(pkg, ctx, s, dtype, omega, f"grid {dims} {opts}")
    s.close()


AMG_SYSTEMS = {"var7": lambda: mg_ref.variable7(13, 11, 9), "permuted16": lambda: amg_ref.permuted(mg_ref.laplace3d(16, 16, 16))}
AMG_OPTS = [{"min_rows": 32}, {"min_rows": 32, "smooth_steps": 2, "over_correction": 1.0}, {"min_rows": 32, "smooth_steps": 3}]


@pytest.mark.parametrize("nrhs", [1, 3])
@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("kind", list(AMG_SYSTEMS))
def test_cycle_bits_algebraic(pkg, gpu, kind, dtype, nrhs):
    ctx = gpu[0]
    s = solver(pkg, ctx, as_type(AMG_SYSTEMS[kind](), dtype), dtype, nrhs)
    for opts in AMG_OPTS:
        omega = set_mg(s, ("amg", opts))
        assert len(s.mg_levels()) >= 3
        check_cycle_bits(pkg, ctx, s, dtype, omega, f"algebraic {kind} {opts}")
    s.close()
