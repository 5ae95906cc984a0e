"""The host restatement of the algebraic aggregates (amg_ref.py) on its own: what every map must be, the hash, the rounds the matching
needs on every input the GPU tests give it, and what the aggregates are for -- fewer iterations than the box aggregates where the
couplings are anisotropic.  No GPU."""
import numpy as np
import pytest

import amg_ref
import mg_ref

# every system of test_gpu_amg.py: (name, matrix, options of the hierarchy)
GPU_INPUTS = [("lap 7x6x5", lambda: mg_ref.laplace3d(7, 6, 5), {"min_rows": 2}),
              ("stencil27 7x6x5", lambda: mg_ref.stencil27(7, 6, 5), {"min_rows": 2}),
              ("z100 9x7x6", lambda: amg_ref.zaniso(9, 7, 6), {"min_rows": 2}),
              ("var7 7x6x5", lambda: mg_ref.variable7(7, 6, 5), {"min_rows": 2}),
              ("var7 9x7x1", lambda: mg_ref.variable7(9, 7, 1), {"min_rows": 2}),
              ("var7 13x1x1", lambda: mg_ref.variable7(13, 1, 1), {"min_rows": 2}),
              ("var7 9x7x5", lambda: mg_ref.variable7(9, 7, 5), {"min_rows": 32}),
              ("var7 9x7x5 seed 4", lambda: mg_ref.variable7(9, 7, 5, seed=4), {"min_rows": 32}),
              ("var7 13x11x9", lambda: mg_ref.variable7(13, 11, 9), {"min_rows": 32}),
              ("z100 24x20x16", lambda: amg_ref.zaniso(24, 20, 16), {}),
              ("z100 12x10x8", lambda: amg_ref.zaniso(12, 10, 8), {}),
              ("lap 16^3 permuted", lambda: amg_ref.permuted(mg_ref.laplace3d(16, 16, 16)), {}),
              ("lap 12x10x8 permuted", lambda: amg_ref.permuted(mg_ref.laplace3d(12, 10, 8)), {"min_rows": 32}),
              ("lap 24x24", lambda: mg_ref.laplace3d(24, 24, 1), {"min_rows": 32}),
              ("graph", amg_ref.graph_laplacian, {"min_rows": 2}),
              ("arrowhead", amg_ref.arrowhead, {"min_rows": 2}),
              ("diagonal", amg_ref.diagonal, {"min_rows": 2}),
              ("positive tridiagonal", amg_ref.positive_tridiagonal, {"min_rows": 2})]


@pytest.mark.parametrize("passes", [1, 2, 3])
@pytest.mark.parametrize("name,make,opts", GPU_INPUTS, ids=[g[0] for g in GPU_INPUTS])
def test_maps_are_what_the_header_promises(name, make, opts, passes):
    """a partition, aggregates of at most 2^passes rows, ids ascending with the smallest member, every aggregate connected, every
    matching done within the 32 rounds (an unbounded matching runs as many), coarsening to at most 0.8"""
    A = make()
    H = amg_ref.Hierarchy(A, np.float64, passes=passes, **opts)
    for l, L in enumerate(H.levels[:-1]):
        amg_ref.check_map(L.A, L.agg, H.levels[l + 1].n, passes)
        assert 5 * H.levels[l + 1].n <= 4 * L.n
        B = L.A
        for _ in range(passes):
            match, rounds = amg_ref.match_pass(B, 0.25, max_rounds=10 ** 6)
            assert rounds <= amg_ref.MAX_ROUNDS, (name, l, rounds)
            assert np.array_equal(match, amg_ref.match_pass(B, 0.25)[0])
            i = np.flatnonzero(match >= 0)
            assert np.array_equal(match[match[i]], i)               # a matching: partners name each other
            pmap, nc = amg_ref.number(match)
            B, widest = amg_ref.galerkin(B, pmap, nc, np.float64)
            if widest > amg_ref.MAX_ROW:
                break
    print(f"  {name} passes {passes}: rows {[L.n for L in H.levels]}, most rounds {max(H.rounds, default=0)}")
    assert max(H.rounds, default=0) <= amg_ref.MAX_ROUNDS


def test_hash_is_symmetric_and_spreads():
    rng = np.random.default_rng(2)
    i, j = rng.integers(0, 2 ** 31 - 1, 4000), rng.integers(0, 2 ** 31 - 1, 4000)
    h = amg_ref.pair_hash(i, j)
    assert np.array_equal(h, amg_ref.pair_hash(j, i)) and h.max() < 2 ** 32
    assert int(amg_ref.pair_hash(0, 0)) == 0
    # the reason it is there: along a constant-coefficient grid line the hash orders neighbours differently from the index
    line = amg_ref.pair_hash(np.arange(100), np.arange(1, 101)).astype(np.int64)
    assert 20 < np.count_nonzero(np.diff(line) > 0) < 80
    # one known value, computed by hand from the definition, pins the constants and the shifts
    lo, hi, M = 3, 7, 0xFFFFFFFF
    v = ((lo * 0x9E3779B1) & M) ^ hi
    v ^= v >> 16
    v = (v * 0x85EBCA6B) & M
    v ^= v >> 13
    v = (v * 0xC2B2AE35) & M
    v ^= v >> 16
    assert int(amg_ref.pair_hash(7, 3)) == v


def test_constant_stencil_matches_in_few_rounds():
    """with ties broken by the hash a constant-coefficient line pairs up in a handful of rounds, not one pair per round"""
    match, rounds = amg_ref.match_pass(mg_ref.laplace3d(200, 1, 1), 0.25)
    assert rounds <= 12 and np.count_nonzero(match >= 0) >= 150


def test_strength_rules():
    """a NaN is never strong, positive off-diagonals are never strong, theta = 1 keeps only the row maximum"""
    import scipy.sparse as sp
    A = sp.csr_matrix(np.array([[4.0, -1.0, -2.0, 0.5],
                                [-1.0, 4.0, np.nan, 0.0],
                                [-2.0, np.nan, 4.0, 0.0],
                                [0.5, 0.0, 0.0, 4.0]]))
    match, _ = amg_ref.match_pass(A, 1.0)
    assert match.tolist() == [2, -1, 0, -1]
    match, _ = amg_ref.match_pass(A, 0.25)
    assert match.tolist() == [2, -1, 0, -1]                         # 1 is left with a NaN towards 2 and a taken 0; 3 couples positively
    agg, nc = amg_ref.number(match)
    assert agg.tolist() == [0, 1, 0, 2] and nc == 3


def test_stop_rules():
    for make in (amg_ref.arrowhead, amg_ref.diagonal, amg_ref.positive_tridiagonal):
        assert len(amg_ref.Hierarchy(make(), np.float64, min_rows=2).levels) == 1
    G = amg_ref.graph_laplacian()
    one, three = amg_ref.Hierarchy(G, np.float64, passes=1, min_rows=2), amg_ref.Hierarchy(G, np.float64, passes=3, min_rows=2)
    assert len(one.levels) >= 2 and len(three.levels) >= 1
    # the 64-column rule is what ends both: the product of one more pass would be wider
    for H, passes in ((one, 1), (three, 3)):
        last = H.levels[-1].A
        assert last.shape[0] > 2 and amg_ref.coarsen(last, np.float64, passes) is None
        match, _ = amg_ref.match_pass(last, 0.25)
        pmap, nc = amg_ref.number(match)
        assert amg_ref.galerkin(last, pmap, nc, np.float64)[1] > amg_ref.MAX_ROW


def test_anisotropic_counts():
    """24 x 20 x 16 with 100 x z-coupling to 1e-6 ||b||: algebraic < grid multigrid and algebraic < Jacobi / 2 (22 / 40 / 70)"""
    dims = (24, 20, 16)
    A = amg_ref.zaniso(*dims)
    b = np.random.default_rng(11).standard_normal(A.shape[0])
    tol = 1e-6 * np.linalg.norm(b)
    H, G = amg_ref.Hierarchy(A, np.float64), mg_ref.Hierarchy(A, dims, np.float64)
    dinv = 1.0 / A.diagonal()
    its_a = amg_ref.pcg_count(A, b, lambda r: H.vcycle(r), tol)
    its_g = amg_ref.pcg_count(A, b, lambda r: G.vcycle(r), tol)
    its_j = amg_ref.pcg_count(A, b, lambda r: dinv * r, tol)
    print(f"  algebraic {its_a}, grid multigrid {its_g}, Jacobi {its_j}")
    assert its_a < its_g and its_a < its_j / 2
