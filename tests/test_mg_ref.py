"""The host restatement of the multigrid preconditioner (mg_ref.py) checked on its own, on the 32^3 7-point Laplacian: the V-cycle
is a symmetric operator, and as M^-1 of PCG it cuts the iteration count to a third of plain CG's at least -- the margin the GPU
convergence test (test_gpu_multigrid.py) relies on."""
import numpy as np
import scipy.sparse as sp

import mg_ref
import tridiag_pcg as tp

N = 32


def test_hierarchy_shape():
    """dims halve (rounded up), coarsening stops at the first level of at most 512 rows; a 7-point level stays 7-point"""
    H = mg_ref.Hierarchy(mg_ref.laplace3d(N, N, N), (N, N, N), np.float64)
    assert [L.dims for L in H.levels] == [(32, 32, 32), (16, 16, 16), (8, 8, 8)]
    assert [int(np.max(np.diff(L.A.indptr))) for L in H.levels] == [7, 7, 7]
    H = mg_ref.Hierarchy(mg_ref.laplace3d(7, 6, 5), (7, 6, 5), np.float64, min_rows=4)
    assert [L.dims for L in H.levels] == [(7, 6, 5), (4, 3, 3), (2, 2, 2), (1, 1, 1)]
    # ragged aggregates of 1, 2 and 4 nodes at the far faces
    assert sorted(set(np.bincount(mg_ref.agg_map((7, 6, 5))).tolist())) == [2, 4, 8]
    assert sorted(set(np.bincount(mg_ref.agg_map((7, 7, 5))).tolist())) == [1, 2, 4, 8]


def test_galerkin_is_scipys_product():
    A = mg_ref.variable7(7, 6, 5)
    Ac, _ = mg_ref.galerkin(A, (7, 6, 5), np.float64)
    agg = mg_ref.agg_map((7, 6, 5))
    P = sp.csr_matrix((np.ones(agg.size), (np.arange(agg.size), agg)))
    want = sp.csr_matrix(P.T @ A @ P)
    want.sort_indices()
    assert np.array_equal(Ac.indptr, want.indptr) and np.array_equal(Ac.indices, want.indices)
    assert np.max(np.abs(Ac.data - want.data)) <= 1e-14 * np.max(np.abs(want.data))


def test_vcycle_is_symmetric():
    """|u^T M^-1 v - v^T M^-1 u| <= 1e-12 |u^T M^-1 v|, the cycle in extended precision"""
    H = mg_ref.Hierarchy(mg_ref.laplace3d(N, N, N), (N, N, N), np.float64)
    rng = np.random.default_rng(0)
    u, v = rng.standard_normal(N ** 3), rng.standard_normal(N ** 3)
    a = np.dot(u.astype(np.longdouble), H.vcycle(v, np.longdouble))
    b = np.dot(v.astype(np.longdouble), H.vcycle(u, np.longdouble))
    print(f"u.M^-1 v {float(a):.17e}, v.M^-1 u {float(b):.17e}, difference {float(abs(a - b) / abs(a)):.3e}")
    assert abs(a - b) <= 1e-12 * abs(a)


def test_pcg_iterations_a_third_of_plain_cg():
    A = mg_ref.laplace3d(N, N, N)
    H = mg_ref.Hierarchy(A, (N, N, N), np.float64)
    b = np.random.default_rng(1).standard_normal(N ** 3)
    tol = 1e-8 * np.linalg.norm(b)
    _, i_mg = tp.pcg_sparse(A, b.astype(complex), sp.identity(N ** 3), tol=tol, maxit=400, solve=H.solve())
    _, i_cg = tp.pcg_sparse(A, b.astype(complex), sp.identity(N ** 3), tol=tol, maxit=400, solve=lambda r: r)
    print(f"32^3 to 1e-8 ||b||: multigrid PCG {i_mg + 1} iterations, plain CG {i_cg + 1}")
    assert 3 * (i_mg + 1) <= i_cg + 1
