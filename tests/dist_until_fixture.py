"""What the tolerance-stop tests of the row-partitioned solver share (test_dist_until_gloo.py, test_gpu_dist_until.py): how a
tolerance is chosen from a fixed-count history so that the stopping iteration is known beforehand and sits off every chunk
boundary."""
import numpy as np

MAXIT = 24      # iterations of the reference run; the stop must fall inside


def choose_tol(hist, first=11, chunk=8):
    """(tol, k): k = the first index >= `first` at which sqrt|hist| is a new minimum and which is no multiple of `chunk`; tol = the
    geometric mean of that norm and the minimum before it.  Every earlier norm is >= the previous minimum > tol and the norm at k
    is < tol, so the rule `first k >= 1 with !(sqrt|r.r| >= tol)` stops exactly at k, with a factor sqrt(ratio) of margin on
    either side."""
    norms = np.sqrt(np.abs(np.asarray(hist)))
    assert np.all(np.isfinite(norms))
    for k in range(first, len(norms)):
        before = float(np.min(norms[:k]))
        if norms[k] < before and k % chunk != 0:
            return float(np.sqrt(norms[k] * before)), k
    raise AssertionError("the history has no new minimum off a chunk boundary")


def stop_index(hist, tol):
    """the rule itself on a history: first k >= 1 with !(sqrt|hist[k]| >= tol), or None"""
    norms = np.sqrt(np.abs(np.asarray(hist)))
    for k in range(1, len(norms)):
        if not norms[k] >= tol:
            return k
    return None
