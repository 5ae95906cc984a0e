"""The three kernels of the multigrid V-cycle and the scan of the setup (csrc/multigrid.hip, csrc/amg.hip) through their stateless
entries, element by element and BIT FOR BIT against the host restatement (tests/mg_kernel_ref.py), in all four value types.

As in test_gpu_mixed_kernels.py, every array of a call lies inside a larger device buffer filled with 0xFF bytes -- a NaN in every
value type, -1 as an int -- and the WHOLE buffer is compared afterwards with what the contract says it holds: the results where the
kernel writes, the bytes of before everywhere else (the lanes between size and the leading dimension, the bytes around the arrays,
every array that is only read).  An array the contract says is not read (w in mode 0, d outside mode 2) is left as canary throughout,
so a kernel that read it would return NaNs; one it says is not written (d with store_d = 0) must come back as canary.  The padding
lanes of b and w are NaN canaries as well: no sum may take them in.

Which NaN an operation returns (sign, payload) is the one thing IEEE leaves open: where the restatement has a NaN the device must
have one, every other lane is compared in all its bits."""
import numpy as np
import pytest

import mg_kernel_ref as K
from canary_buffers import Embedded

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def env(pkg, gpu):
    return pkg, gpu[0], pkg._lib.load()


def blank(shape, dtype):
    return np.empty(shape, dtype)


# ---- the smoothing step -------------------------------------------------------------------------------------------------------------------
SMOOTH = K.smooth_cases()


@pytest.mark.parametrize("c", SMOOTH, ids=[c["id"] for c in SMOOTH])
def test_smooth_step(env, c):
    pkg, ctx, lib = env
    P = pkg._lib.ptr
    dtype, inp = K.DTYPES[c["dt"]], K.smooth_inputs(c)
    mode, store_d, n, nrhs, ld, off = c["mode"], c["store_d"], c["size"], c["nrhs"], c["ld"], c["off"]
    dinv = Embedded(pkg, ctx, inp["dinv"][None, :], n, off)
    b = Embedded(pkg, ctx, inp["b"], ld, off)
    w = Embedded(pkg, ctx, inp["w"], ld, off, blank=mode == 0)
    d = Embedded(pkg, ctx, inp["d"], ld, off, blank=mode != 2)
    x = Embedded(pkg, ctx, inp["x"], ld, off, blank=mode == 0)
    pkg._lib.check(lib.cgamd_mg_smooth_step(ctx.handle, K.CODE[c["dt"]], mode, n, ld, nrhs, P(dinv.ptr), P(b.ptr), P(w.ptr), P(d.ptr), P(x.ptr),
                                            inp["c0"], inp["c1"], store_d))
    want_x, want_d = K.smooth_step(dtype, mode, inp["dinv"], inp["b"], inp["w"], inp["d"], inp["x"], inp["c0"], inp["c1"], store_d)
    x.check("x", want_x)
    d.check("d" if store_d else "d is not written without store_d", want_d)
    dinv.check("dinv is only read")
    b.check("b is only read")
    w.check("w is only read" if mode else "w is neither read nor written in mode 0")


def test_smooth_step_takes_null_for_what_it_does_not_touch(env):
    """mode 0 without w and d, mode 1 without d; and a size of 0 launches nothing"""
    pkg, ctx, lib = env
    P = pkg._lib.ptr
    c = [c for c in SMOOTH if c["dt"] == "f64" and c["size"] == 257 and c["store_d"] == 0][0]
    inp = K.smooth_inputs(c)
    for mode in (0, 1):
        dinv = Embedded(pkg, ctx, inp["dinv"][None, :], 257)
        b, w = Embedded(pkg, ctx, inp["b"], 260), Embedded(pkg, ctx, inp["w"], 260)
        x = Embedded(pkg, ctx, inp["x"], 260, blank=mode == 0)
        pkg._lib.check(lib.cgamd_mg_smooth_step(ctx.handle, 1, mode, 257, 260, 3, P(dinv.ptr), P(b.ptr), P(w.ptr) if mode else None, None, P(x.ptr),
                                                0.0, inp["c1"], 0))
        x.check(f"x, mode {mode}", K.smooth_step(np.float64, mode, inp["dinv"], inp["b"], inp["w"], None, inp["x"], 0.0, inp["c1"], 0)[0])
        pkg._lib.check(lib.cgamd_mg_smooth_step(ctx.handle, 1, 2, 0, 260, 3, P(dinv.ptr), P(b.ptr), P(w.ptr), P(w.ptr), P(b.ptr), 0.5, 0.5, 1))
        b.check("size 0: b")
        w.check("size 0: w")


# ---- restriction and prolongation ---------------------------------------------------------------------------------------------------------
TRANSFER = K.transfer_cases()
_INPUTS = {}


def transfer_inputs(c):
    if c["id"] not in _INPUTS:
        _INPUTS[c["id"]] = K.transfer_inputs(c)
    return _INPUTS[c["id"]]


def map_arguments(pkg, ctx, c, inp, lists):
    """(nx, ny, nz, the Embedded map or None): the box map by its dims, a stored map as member lists or as the map itself"""
    if c["kind"] == "box":
        return c["dims"] + (None,)
    table = inp["members"].reshape(1, -1) if lists else inp["agg"][None, :]
    return (inp["nf"], 0, 0, Embedded(pkg, ctx, table.astype(np.intc), table.size))


@pytest.mark.parametrize("c", TRANSFER, ids=[c["id"] for c in TRANSFER])
def test_restrict(env, c):
    pkg, ctx, lib = env
    P = pkg._lib.ptr
    dtype, full = K.DTYPES[c["dt"]], transfer_inputs(c)
    nf, nc = full["nf"], full["nc"]
    for nrhs, store_d, pad_f, pad_c in ((1, 1, 3, 1), (3, 0, 5, 7), (3, 1, 1, 2)):
        inp = {k: (v[:nrhs] if k in ("b", "w") else v) for k, v in full.items()}
        nx, ny, nz, mem = map_arguments(pkg, ctx, c, inp, True)
        b, w = Embedded(pkg, ctx, inp["b"], nf + pad_f), Embedded(pkg, ctx, inp["w"], nf + pad_f)
        dinv = Embedded(pkg, ctx, inp["dinv_c"][None, :], nc)
        bc, xc, dc = (Embedded(pkg, ctx, blank((nrhs, nc), dtype), nc + pad_c, blank=True) for _ in range(3))
        pkg._lib.check(lib.cgamd_mg_restrict(ctx.handle, K.CODE[c["dt"]], nx, ny, nz, P(mem.ptr) if mem else None, nc, nf + pad_f, nc + pad_c, nrhs,
                                             P(b.ptr), P(w.ptr), P(bc.ptr), P(dinv.ptr), P(xc.ptr), P(dc.ptr), inp["c1"], store_d))
        want_bc, want_t = K.restrict(dtype, inp["members"], inp["b"], inp["w"], inp["dinv_c"], inp["c1"])
        label = f"nrhs {nrhs} store_d {store_d}"
        bc.check(f"{label}: bc", want_bc)
        xc.check(f"{label}: xc", want_t)
        dc.check(f"{label}: dc", want_t if store_d else None)
        b.check(f"{label}: b is only read")
        w.check(f"{label}: w is only read")
        dinv.check(f"{label}: dinv_c is only read")
        if mem:
            mem.check(f"{label}: the member lists are only read")


@pytest.mark.parametrize("c", TRANSFER, ids=[c["id"] for c in TRANSFER])
def test_prolong(env, c):
    pkg, ctx, lib = env
    P = pkg._lib.ptr
    dtype, full = K.DTYPES[c["dt"]], transfer_inputs(c)
    nf, nc = full["nf"], full["nc"]
    for nrhs, omega, pad_f, pad_c, short in ((1, 1.6, 3, 1, 0), (3, 1.0, 5, 7, 0), (3, 1.6, 2, 3, min(3, nf - 1))):
        inp = {k: (v[:nrhs] if k in ("x", "e") else v) for k, v in full.items()}
        n_fine = nf - short                               # (short: the kernel stops at n_fine, the rows behind it keep their bytes)
        nx, ny, nz, agg = map_arguments(pkg, ctx, c, inp, False)
        x = Embedded(pkg, ctx, inp["x"], nf + pad_f)
        e = Embedded(pkg, ctx, inp["e"], nc + pad_c)
        pkg._lib.check(lib.cgamd_mg_prolong(ctx.handle, K.CODE[c["dt"]], nx, ny, nz, P(agg.ptr) if agg else None, n_fine, nf + pad_f, nc + pad_c, nrhs,
                                            P(e.ptr), P(x.ptr), omega))
        want = inp["x"].copy()
        want[:, :n_fine] = K.prolong(dtype, inp["agg"][:n_fine], inp["e"], inp["x"], omega)
        label = f"nrhs {nrhs} omega {omega} n_fine {n_fine} of {nf}"
        x.check(f"{label}: x", want)
        e.check(f"{label}: e is only read")
        if agg:
            agg.check(f"{label}: the map is only read")


# ---- the scan -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,counts", K.scan_cases(), ids=[n for n, _ in K.scan_cases()])
def test_scan(env, name, counts):
    """a[n] and the flag word sit inside canaries: a holds n + 1 ints and nothing behind them is touched; the flag is preset to 0 and
    written only on overflow"""
    pkg, ctx, lib = env
    P = pkg._lib.ptr
    n = counts.size
    start = np.concatenate([counts, [-1]]).astype(np.intc)[None, :]        # (a[n] starts as canary: it has to be written)
    a = Embedded(pkg, ctx, start, n + 1)
    flag = Embedded(pkg, ctx, np.zeros((1, 1), np.intc), 1)
    pkg._lib.check(lib.cgamd_mg_scan(ctx.handle, n, P(a.ptr), P(flag.ptr)))
    want, overflow = K.scan(counts)
    a.check("prefix sums", want[None, :])
    flag.check("overflow flag", np.full((1, 1), overflow, np.intc))
    if overflow:
        assert want[-1] == 2 ** 31 - 1 and want.max() == 2 ** 31 - 1
    else:
        assert np.array_equal(want[1:], np.cumsum(counts))


def test_refusals_with_a_context(env):
    """what only a call with a live context reaches: every refusal leaves the arrays alone"""
    pkg, ctx, lib = env
    P = pkg._lib.ptr
    v = Embedded(pkg, ctx, np.ones((1, 8)), 8)
    ints = Embedded(pkg, ctx, np.zeros((1, 8), np.intc), 8)
    p = P(v.ptr)
    INVALID = pkg._lib.ERR_INVALID
    assert lib.cgamd_mg_smooth_step(ctx.handle, 4, 0, 4, 4, 1, p, p, p, p, p, 0.0, 1.0, 0) == INVALID
    assert lib.cgamd_mg_smooth_step(ctx.handle, 1, 3, 4, 4, 1, p, p, p, p, p, 0.0, 1.0, 0) == INVALID
    assert lib.cgamd_mg_smooth_step(ctx.handle, 1, 2, 4, 3, 1, p, p, p, p, p, 0.0, 1.0, 0) == INVALID
    assert lib.cgamd_mg_smooth_step(ctx.handle, 1, 1, 4, 4, 1, p, p, None, p, p, 0.0, 1.0, 0) == INVALID
    assert lib.cgamd_mg_smooth_step(ctx.handle, 1, 1, 4, 4, 1, p, p, p, None, p, 0.0, 1.0, 1) == INVALID
    assert lib.cgamd_mg_restrict(ctx.handle, 1, 3, 2, 1, None, 3, 6, 2, 1, p, p, p, p, p, p, 1.0, 0) == INVALID        # 2 boxes, not 3
    assert lib.cgamd_mg_restrict(ctx.handle, 1, 3, 2, 1, None, 2, 5, 2, 1, p, p, p, p, p, p, 1.0, 0) == INVALID        # ld_f < 6
    assert lib.cgamd_mg_restrict(ctx.handle, 1, 3, 2, 1, None, 2, 6, 2, 1, p, p, p, p, p, None, 1.0, 1) == INVALID
    assert lib.cgamd_mg_prolong(ctx.handle, 1, 3, 2, 1, None, 7, 8, 2, 1, p, p, 1.0) == INVALID                        # 7 rows on a grid of 6
    assert lib.cgamd_mg_prolong(ctx.handle, 1, 3, 2, 1, None, 6, 6, 1, 1, p, p, 1.0) == INVALID                        # ld_c < 2 boxes
    assert lib.cgamd_mg_scan(ctx.handle, -1, P(ints.ptr), P(ints.ptr)) == INVALID
    v.check("refused calls: values")
    ints.check("refused calls: ints")
