"""GPU tests of the deferred x update (vector.hip "x brought up to date once per group of L iterations"): inside a captured run
of 8 iterations the three / four-launch loop keeps the directions of L iterations and its last d step of the group applies the L
updates x += alpha_j d_j in iteration order.  Every call must end with nothing pending and with x, the history -- and, pinned by
8 further iterations, r and d -- BIT FOR BIT what the handle that updates x in every iteration (lag 1) holds: for every value type,
one and several right-hand sides, sizes with appended rows and scalar tails, and every way of splitting the iteration count over
calls (whole graphs, single iterations before, between and after them).

Small systems reach the loop through the knobs two_launch=0, dev.no_fold_alpha=1, resident=0, resident_wide=0 (the four-launch
family) and dev.x_lag, which forces the lag."""
import numpy as np
import pytest

import cg_numpy
import cg_oracle
from conftest import ALL_DTYPES, rand_vec

pytestmark = pytest.mark.gpu

FOUR_LAUNCH = {"two_launch": 0, "dev.no_fold_alpha": 1, "resident": 0, "resident_wide": 0}
DEFAULTS = {"two_launch": 1, "dev.no_fold_alpha": 0, "resident": 1, "resident_wide": 1, "dev.x_lag": -1}
LAGS = (2, 4, 8)
# iterations per call; "x" = read x back between two calls
PATTERNS = ((8,), (16,), (24,), (5,), (11,), (8, 8), (3, 8, 5), (16, "x", 8))


def _matrix(shape, dtype):
    if shape == "helm24":
        N = 24
        ip, ix, da = cg_numpy.helm_fe_var(N, 12.0, np.ones((N - 1, N - 1)), 0.15, N, N)
    else:
        ip, ix, da = cg_numpy.laplace3d(*shape)
    return ip, ix, da.astype(dtype)


def _rhs(n, nrhs, dtype, seed):
    rng = np.random.default_rng(seed)
    return np.concatenate([(r + 1) * 5.0 + rand_vec(rng, n, dtype) for r in range(nrhs)]).astype(dtype)


def _handle(pkg, ctx, lag, ip, ix, da, nrhs, flags=0):
    """a handle of the four-launch family created under dev.x_lag = lag"""
    lib = pkg._lib.load()
    cfg = dict(FOUR_LAUNCH)
    cfg["dev.x_lag"] = lag
    for k, v in cfg.items():
        pkg._lib.check(lib.cgamd_tune(k.encode(), v))
    try:
        return pkg.Solver(ctx, len(ip) - 1, len(ix), da, ip, ix, nrhs, flags=flags)
    finally:
        for k in cfg:
            pkg._lib.check(lib.cgamd_tune(k.encode(), DEFAULTS[k]))


def _handles(pkg, ctx, ip, ix, da, nrhs):
    """{lag: handle} for lag 1 and every forced lag, each checked for the loop and the lag it reports"""
    lib = pkg._lib.load()
    hs = {lag: _handle(pkg, ctx, lag, ip, ix, da, nrhs) for lag in (1,) + LAGS}
    for lag, s in hs.items():
        assert lib.cgamd_solver_x_lag(s.handle) == lag
        assert lib.cgamd_solver_loop_launches(s.handle) == 4
    return hs


def _same(hs, what):
    ref = (hs[1].x(), hs[1].history())
    for lag in LAGS:
        x, h = hs[lag].x(), hs[lag].history()
        assert h.shape == ref[1].shape, (what, lag)
        assert np.array_equal(h, ref[1], equal_nan=True), f"history differs: lag {lag}, {what}"
        assert np.array_equal(x, ref[0], equal_nan=True), f"x differs: lag {lag}, {what}"


CASES = [(shape, dt, nrhs) for shape in ((20, 16, 12), (13, 7, 5)) for dt in ALL_DTYPES for nrhs in (1, 3)]
CASES += [("helm24", np.complex64, nrhs) for nrhs in (1, 3)]


@pytest.mark.parametrize("shape,dtype,nrhs", CASES, ids=lambda v: getattr(v, "__name__", None) or str(v).replace(" ", ""))
def test_every_call_pattern_leaves_the_bits_of_lag_1(pkg, gpu, shape, dtype, nrhs):
    ctx, queue, kernels = gpu
    ip, ix, da = _matrix(shape, dtype)
    n = len(ip) - 1
    B = _rhs(n, nrhs, dtype, seed=7 * nrhs + n)
    X0 = (0.1 * rand_vec(np.random.default_rng(n), n * nrhs, dtype)).astype(dtype)
    hs = _handles(pkg, ctx, ip, ix, da, nrhs)
    try:
        for pat in PATTERNS:
            for s in hs.values():
                s.set_rhs(B, X0)
            for step, k in enumerate(pat):
                if k == "x":
                    for s in hs.values():
                        s.x()
                    continue
                for s in hs.values():
                    s.iterate(k)
                _same(hs, f"pattern {pat}, call {step}")
            for s in hs.values():           # r and d: what the next iterations are made of
                s.iterate(8)
            _same(hs, f"pattern {pat}, 8 more")
    finally:
        for s in hs.values():
            s.close()


def test_plain_launch_handle_reports_lag_1_and_agrees(pkg, gpu):
    ctx, queue, kernels = gpu
    lib = pkg._lib.load()
    ip, ix, da = _matrix((20, 16, 12), np.float64)
    B = _rhs(len(ip) - 1, 3, np.float64, seed=3)
    plain = _handle(pkg, ctx, 4, ip, ix, da, 3, flags=pkg._lib.NO_GRAPH)
    lagged = _handle(pkg, ctx, 4, ip, ix, da, 3)
    try:
        assert lib.cgamd_solver_x_lag(plain.handle) == 1
        assert lib.cgamd_solver_x_lag(lagged.handle) == 4
        for s in (plain, lagged):
            s.set_rhs(B, None)
            s.iterate(19)
        assert np.array_equal(plain.history(), lagged.history())
        assert np.array_equal(plain.x(), lagged.x())
    finally:
        plain.close()
        lagged.close()


def test_iterate_until_after_a_graph_stops_every_right_hand_side_where_lag_1_does(pkg, gpu):
    ctx, queue, kernels = gpu
    ip, ix, da = _matrix((20, 16, 12), np.float64)
    nrhs = 3
    B = _rhs(len(ip) - 1, nrhs, np.float64, seed=11)
    hs = _handles(pkg, ctx, ip, ix, da, nrhs)
    try:
        out = {}
        for lag, s in hs.items():
            s.set_rhs(B, None)
            s.iterate(8)
            tol = np.sqrt(np.abs(s.history()[0])) * np.array([1e-2, 1e-4, 1e-6])
            its = s.iterate_until(tol, 400)
            out[lag] = (its.copy(), s.x(), s.history())
        its1 = out[1][0]
        assert len(set(its1.tolist())) == nrhs and np.all(its1 > 8) and np.all(its1 < 408), its1     # stopped, each in its own iteration
        for lag in LAGS:
            assert np.array_equal(out[lag][0], its1), (lag, out[lag][0], its1)
            assert np.array_equal(out[lag][2], out[1][2], equal_nan=True), lag
            assert np.array_equal(out[lag][1], out[1][1], equal_nan=True), lag
    finally:
        for s in hs.values():
            s.close()


def test_a_second_right_hand_side_on_the_same_handle_equals_a_fresh_handle(pkg, gpu):
    ctx, queue, kernels = gpu
    ip, ix, da = _matrix((13, 7, 5), np.float32)
    n = len(ip) - 1
    B1, B2 = _rhs(n, 1, np.float32, seed=1), _rhs(n, 1, np.float32, seed=2)
    for lag in LAGS:
        used, fresh = _handle(pkg, ctx, lag, ip, ix, da, 1), _handle(pkg, ctx, lag, ip, ix, da, 1)
        try:
            used.set_rhs(B1, None)
            used.iterate(13)                # a graph and single iterations: the ring and the buffers have been through a group
            for s in (used, fresh):
                s.set_rhs(B2, None)
                s.iterate(16)
            assert np.array_equal(used.history(), fresh.history())
            assert np.array_equal(used.x(), fresh.x())
        finally:
            used.close()
            fresh.close()


@pytest.mark.parametrize("dtype,nrhs", [(np.float64, 1), (np.complex64, 3)])
def test_moved_bytes_price_the_group(pkg, gpu, dtype, nrhs):
    ctx, queue, kernels = gpu
    ip, ix, da = _matrix((13, 7, 5), dtype)
    n, V = len(ip) - 1, np.dtype(dtype).itemsize
    hs = _handles(pkg, ctx, ip, ix, da, nrhs)
    try:
        matrix = hs[1].iter_moved_bytes - 10 * n * V * nrhs      # lag 1: the ten-pass figure
        assert matrix == hs[1].spmv_moved_bytes - 2 * n * V * nrhs
        for lag in LAGS:
            assert hs[lag].iter_moved_bytes == matrix + (9 * lag + 1) * n * V * nrhs // lag
    finally:
        for s in hs.values():
            s.close()


def test_the_knob_takes_the_documented_values_only(pkg, gpu):
    lib = pkg._lib.load()
    for bad in (3, 5, 6, 7, 16, -2):
        assert lib.cgamd_tune(b"dev.x_lag", bad) != 0
    for good in (0, 1, 2, 4, 8, -1):
        assert lib.cgamd_tune(b"dev.x_lag", good) == 0


def test_the_recurrence_is_the_oracles(pkg, gpu):
    """not only the library against itself: delta_k of 40 iterations (5 graphs) against the CPU oracle, at the project's 1e-10"""
    ctx, queue, kernels = gpu
    ip, ix, da = _matrix((20, 16, 12), np.float64)
    B = _rhs(len(ip) - 1, 1, np.float64, seed=5)
    xo, ho = cg_oracle.cg(ip, ix, da, B, n_iterations=40, mode=cg_oracle.MODE_SEQUENTIAL)
    for lag in LAGS:
        s = _handle(pkg, ctx, lag, ip, ix, da, 1)
        try:
            s.set_rhs(B, None)
            s.iterate(40)
            h = s.history()
            err = np.max(np.abs(h[:, 0] - ho[:, 0]) / np.abs(ho[:, 0]))
            print(f"lag {lag}: max rel delta err vs oracle = {err:.3e}")
            assert h.shape == (41, 1) and err < 1e-10, (lag, err)
        finally:
            s.close()
