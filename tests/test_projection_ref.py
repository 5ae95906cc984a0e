"""The numpy restatement of the solution projection (tests/projection_ref.py) must by itself satisfy what the GPU tests lean on."""
import numpy as np
import pytest

import projection_ref as PR

TYPES = [np.float64, np.float32, np.complex128, np.complex64]


@pytest.fixture(scope="module")
def runs():
    cache = {}

    def get(kind, dtype, drop_tol):
        key = (kind, np.dtype(dtype), drop_tol)
        if key not in cache:
            cache[key] = PR.run_sequence(kind, dtype, 4, drop_tol, 9)
        return cache[key]
    return get


@pytest.mark.parametrize("dtype", TYPES, ids=lambda d: np.dtype(d).name)
def test_span3_fills_three_slots_and_then_starts_converged(runs, dtype):
    """right-hand sides in a 3-dimensional space: three vectors span every solution, the fourth is refused, and every later solve
    starts at the tolerance"""
    out = runs("span3", dtype, PR.drop_tol(dtype))
    assert [r["added"] for r in out] == [True] * 3 + [False] * 6
    assert [r["count"] for r in out] == [1, 2, 3] + [3] * 6
    for r in out[3:]:
        print(np.dtype(dtype).name, "solve", r["t"], "start / tol", r["start"] / r["tol"], "iterations", r["its"], "from zero", r["its_zero"])
        assert r["start"] <= 100 * r["tol"]
        assert 5 * r["its"] <= r["its_zero"]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=lambda d: np.dtype(d).name)
def test_moving_source_wraps_the_ring_and_stays_orthonormal(runs, dtype):
    out = runs("moving", dtype, 0.0)
    assert all(r["added"] for r in out)
    assert [r["slot"] for r in out] == [0, 1, 2, 3, 0, 1, 2, 3, 0]
    assert [r["count"] for r in out] == [1, 2, 3, 4, 4, 4, 4, 4, 4]
    for r in out:
        print(np.dtype(dtype).name, "solve", r["t"], "defect / eps", r["defect"] / PR.eps(dtype), "iterations", r["its"], "from zero", r["its_zero"])
        assert r["defect"] < 64 * PR.eps(dtype)
    for r in out[4:]:
        assert r["its"] <= r["its_zero"]


def test_a_refused_column_stores_zeros_and_the_retired_slot_is_not_in_c():
    dtype = np.dtype(np.float64)
    n = PR.NX * PR.NY
    mat = PR.system(dtype)
    P = PR.Projection(mat, n, 2, dtype, 2, 0.0)
    rng = np.random.default_rng(3)
    for t in range(2):
        x0 = P.guess(np.stack([PR.rhs("moving", t, dtype)] * 2))
        x = x0 + rng.standard_normal((2, n))
        x[1] = x0[1] if t == 1 else x[1]            # column 1 found nothing beyond its guess: e = 0, nu = 0
        added = P.update(x)
        assert list(added) == ([True, True] if t == 0 else [True, False])
    assert P.m == 2 and np.all(P.W[1, 1] == 0) and np.any(P.W[1, 0] != 0)
    # a full ring: slot 0 is retired before the update, its c is not formed and it takes no part in e'
    P.guess(np.stack([PR.rhs("moving", 2, dtype)] * 2))
    P.c[:] = 77.0
    old0, old1 = P.W[0].copy(), P.W[1].copy()
    x_last = P.x0[:, :n] + rng.standard_normal((2, n))
    added = P.update(x_last)
    assert list(added) == [True, True] and P.last_slot == 0 and P.head == 1 and P.m == 2
    assert np.all(P.c[0] == 77.0) and np.all(P.c[1] != 77.0)
    assert np.array_equal(P.W[1], old1)
    # e' = e - c_1 w_1 only, and e keeps what slot 0 carried of the guess: e = (x - x0) + alpha_0 w_0
    assert np.array_equal(P.e1, P.ops.axmy(P.e, P.c[1], P.W[1]))
    assert np.array_equal(P.e, P.ops.axpy(P.ops.sub(P._pad(x_last), P.x0), P.alpha[0], old0))
    # padding rows of the stored vectors are zero
    assert np.all(P.W[:, :, n:] == 0)


def test_type_true_dots_follow_the_stated_order():
    """the type-true dot is a double sum of float products in the stated order: equal to the plain double sum up to the double
    rounding of the order, not to float rounding"""
    dtype = np.dtype(np.float32)
    n = PR.NX * PR.NY
    P = PR.Projection(PR.system(dtype), n, 1, dtype, 1, 0.0)
    rng = np.random.default_rng(5)
    a, b = (P._pad(rng.standard_normal((1, n)).astype(dtype)) for _ in range(2))
    exact = np.sum((a * b).astype(np.float64))
    assert abs(P.dot_acc(a, b)[0] - exact) <= n * 2.0 ** -53 * np.sum(np.abs(a * b).astype(np.float64))
    assert P.G == 1 and PR.dots_grid(dtype, 2 * 1024 + 37) == 3 and PR.dots_grid(np.complex128, 10_000_000) == 1024
