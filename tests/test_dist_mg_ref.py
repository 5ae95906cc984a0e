"""The host side of multigrid PCG on the row-partitioned handle (dist_mg_oracle.py, dist.local_grid_dims), which needs no GPU: what
the cut costs in iterations, that a wrong cut would show in the histories the GPU tests compare, and the helper that names a rank's
box."""
import importlib

import numpy as np
import pytest

import dist_mg_oracle as dmo
import mg_ref

from conftest import PKG_NAME

DIMS, OPTS = (13, 11, 12), {"min_rows": 16}


def _system():
    A = mg_ref.variable7(*DIMS)
    b = np.random.default_rng(11).standard_normal(A.shape[0])
    return A, b


@pytest.fixture(scope="module")
def counts():
    """iterations to 1e-6 ||b||: Jacobi, one hierarchy, the cut oracle at world 2 and 3 (and the levels of every rank's hierarchy)"""
    A, b = _system()
    tol = 1e-6 * np.linalg.norm(b)
    out = {"jacobi": len(dmo.oracle(A, b, dmo.jacobi_solve(A), 200, tol)[1]) - 1,
           "uncut": len(dmo.oracle(A, b, dmo.uncut_solve(A, np.float64, DIMS, OPTS), 200, tol)[1]) - 1}
    for world in (2, 3):
        ranges = dmo.row_ranges(A.shape[0], world)
        hs = dmo.hierarchies(A, ranges, np.float64, DIMS, OPTS)
        out[world] = len(dmo.oracle(A, b, dmo.block_solve(hs, ranges), 200, tol)[1]) - 1
        out[f"levels{world}"] = [len(h.levels) for h in hs]
    print(f"  iterations to 1e-6 ||b|| on {DIMS}: {out}")
    return out


@pytest.mark.parametrize("world", [2, 3])
def test_the_cut_hierarchies_beat_jacobi(counts, world):
    """measured: 15 (world 2) and 16 (world 3) against Jacobi's 31; one hierarchy needs 14"""
    assert counts[world] < counts["jacobi"], counts
    assert counts["uncut"] <= counts[world], counts
    assert counts[f"levels{world}"] == ([4, 4] if world == 2 else [3, 3, 3]), counts


@pytest.mark.parametrize("world", [2, 3])
def test_a_wrong_cut_shows_in_the_history(world):
    """within the first 8 iterations the cut and the uncut oracle are at least 100 x the fp64 history tolerance (1e-10) apart
    (measured: relative 0.9): a device that applied one hierarchy to all rows, or kept halo couplings, cannot pass for the cut one"""
    A, b = _system()
    ranges = dmo.row_ranges(A.shape[0], world)
    _, h_cut = dmo.oracle(A, b, dmo.block_solve(dmo.hierarchies(A, ranges, np.float64, DIMS, OPTS), ranges), 8)
    _, h_uncut = dmo.oracle(A, b, dmo.uncut_solve(A, np.float64, DIMS, OPTS), 8)
    apart = dmo.hist_dev(h_uncut, h_cut, h_cut, np.ones(9, bool))
    print(f"  world {world}: cut and uncut histories are {apart:.3e} apart within 8 iterations")
    assert apart >= 100 * 1e-10, apart


def test_the_block_oracle_is_the_ranks_own_cycles():
    """M^-1 of the oracle on a vector = every rank's V-cycle on its slice, on the cut block and the rank's own dims"""
    A, b = _system()
    ranges = dmo.row_ranges(A.shape[0], 3)
    hs = dmo.hierarchies(A, ranges, np.float64, DIMS, OPTS)
    z = dmo.block_solve(hs, ranges)(b.astype(complex))
    for g, (lo, hi) in enumerate(ranges):
        assert hs[g].levels[0].dims == (13, 11, 4) and hs[g].levels[0].n == hi - lo
        assert (hs[g].levels[0].A != A[lo:hi, lo:hi]).nnz == 0
        assert np.array_equal(z[lo:hi], hs[g].vcycle(b[lo:hi], np.float64).astype(complex))


def test_local_grid_dims():
    dmod = importlib.import_module(PKG_NAME + ".dist")
    n = 13 * 11 * 12
    assert [dmod.local_grid_dims(DIMS, dmod.row_ranges(n, 2), g) for g in range(2)] == [(13, 11, 6)] * 2
    assert [dmod.local_grid_dims(DIMS, dmod.row_ranges(n, 3), g) for g in range(3)] == [(13, 11, 4)] * 3
    assert dmod.local_grid_dims(DIMS, [(0, 143), (143, n)], 1) == (13, 11, 11)
    assert dmod.local_grid_dims((13, 11), [(0, 39), (39, 143)], 1) == (13, 8, 1)       # nz == 1: whole x-lines
    assert dmod.local_grid_dims((13, 11, 1), [(0, 39), (39, 143)], 0) == (13, 3, 1)
    for dims, ranges, rank in ((DIMS, dmod.row_ranges(n, 5), 1),          # 343 rows: mid-plane
                               (DIMS, [(0, 150), (150, n)], 0), (DIMS, [(0, 150), (150, n)], 1),
                               ((13, 11), [(0, 40), (40, 143)], 0),      # mid-line
                               (DIMS, [(0, n + 143)], 0), ((13,), [(0, 13)], 0), ((13, 0, 2), [(0, 13)], 0)):
        with pytest.raises(ValueError):
            dmod.local_grid_dims(dims, ranges, rank)
