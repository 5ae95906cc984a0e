"""CPU test of the host merge behind the row-pair SpMV (csrc/row_pairs.cpp merge_pair_slots): the slots of rows 2p and 2p + 1 merged
into one sequence keyed by the offset.  The C++ function is compiled together with a stand-alone program (tests/row_pairs_merge_main.cpp)
under -fsanitize=address,undefined and run as a program; its answers are compared with the Python restatement below on the pattern
pairs of the grids the GPU cases use, on unsorted stored orders and on pairs whose union does not fit 8 slots.  Independent of the
restatement, every answer is checked for what the kernel relies on: each row's stored order survives as a subsequence, two slots are
merged exactly when their offsets are equal, and the length is the shortest possible (len0 + len1 - longest common subsequence)."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "conjugate-gradient-pyopencl_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def lcs_table(a, b):
    L = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(len(a) - 1, -1, -1):
        for j in range(len(b) - 1, -1, -1):
            L[i][j] = L[i + 1][j + 1] + 1 if a[i] == b[j] else max(L[i + 1][j], L[i][j + 1])
    return L


def merge(a, b):
    """the restatement: equal heads merge; else the head whose removal keeps the longer common subsequence, row 2p's on a tie"""
    L = lcs_table(a, b)
    total = len(a) + len(b) - L[0][0]
    if total > 8:
        return ("long", total)
    i = j = 0
    out = []
    while i < len(a) or j < len(b):
        if i < len(a) and j < len(b) and a[i] == b[j]:
            out.append((a[i], i, j)); i += 1; j += 1
        elif j == len(b) or (i < len(a) and L[i + 1][j] >= L[i][j + 1]):
            out.append((a[i], i, -1)); i += 1
        else:
            out.append((b[j], -1, j)); j += 1
    return ("ok", out)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("row_pairs") / "merge_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "row_pairs_merge_main.cpp"), os.path.join(CSRC, "row_pairs.cpp"), "-o", exe])
    return exe


def run(exe, cases):
    text = "".join(f"{len(a)} {' '.join(map(str, a))} {len(b)} {' '.join(map(str, b))}\n" for a, b in cases)
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = []
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "long":
            out.append(("long", int(w[1])))
        else:
            v = list(map(int, w[2:]))
            assert len(v) == 3 * int(w[1])
            out.append(("ok", [tuple(v[k:k + 3]) for k in range(0, len(v), 3)]))
    assert len(out) == len(cases)
    return out


def check_properties(a, b, got):
    L = lcs_table(a, b)
    total = len(a) + len(b) - L[0][0]
    if got[0] == "long":
        assert total > 8 and got[1] == total
        return
    slots = got[1]
    assert len(slots) == total <= 8
    assert [s[1] for s in slots if s[1] >= 0] == list(range(len(a)))        # row 2p's stored order, every slot once
    assert [s[2] for s in slots if s[2] >= 0] == list(range(len(b)))
    for off, i, j in slots:
        assert i >= 0 or j >= 0
        assert i < 0 or a[i] == off
        assert j < 0 or b[j] == off


def grid_pairs(ip, ix):
    """the distinct (offsets of row 2p, offsets of row 2p + 1) of a CSR matrix, in stored order; a lone last row pairs with ()"""
    n = len(ip) - 1
    seq = [tuple((ix[ip[i]:ip[i + 1]] - i).tolist()) for i in range(n)] + [()]
    return sorted({(seq[r], seq[r + 1]) for r in range(0, n, 2)})


def test_merge_on_the_grids_of_the_gpu_cases(program):
    import cg_numpy
    cases = []
    for grid in ((23, 19, 31), (130, 5, 4), (40, 30, 20), (7, 3, 3)):
        ip, ix, _ = cg_numpy.laplace3d(*grid)
        cases += grid_pairs(np.asarray(ip), np.asarray(ix))
    ip, ix, _ = cg_numpy.poisson2d(15)
    cases += grid_pairs(np.asarray(ip), np.asarray(ix))
    cases = sorted(set(cases))
    assert len(cases) > 27 and any(a != b for a, b in cases) and any(b == () for a, b in cases)
    got = run(program, cases)
    for (a, b), g in zip(cases, got):
        assert g == merge(a, b), (a, b, g)
        assert g[0] == "ok" and len(g[1]) <= 7      # a 7-point stencil in ascending order: the union of two neighbours has at most 7 offsets
        check_properties(a, b, g)


def test_merge_unsorted_overlong_and_edge_cases(program):
    full = (-300, -20, -1, 0, 1, 20, 300)
    cases = [
        ((), ()), ((0,), ()), ((), (0,)), (full, full), (full, ()), ((), full),
        (full, tuple(reversed(full))),                      # ascending against descending: longest common subsequence 1, 13 slots
        (full, (-20, -300, -1, 0, 1, 20, 300)),             # one swap: 8 slots, still fits
        (full, (-20, -300, 0, -1, 1, 20, 300)),             # two swaps: 9 slots
        ((0, 1, 2, 3, 4, 5, 6), (7, 8, 9, 10, 11, 12, 13)),  # nothing in common: 14
        ((0, 1, 2, 3), (4, 5, 6, 7)),                       # nothing in common, 8: fits exactly
        ((0, 1, 2, 3), (4, 5, 6, 7, 8)),
        ((5, 5, 5), (5, 5)), ((1, 2, 1, 2), (2, 1, 2, 1)),  # repeated offsets (duplicate columns in a row)
        ((-1, 0, 1), (0, 1)), ((0, 1), (-1, 0, 1)),
        (tuple(range(8)), tuple(range(8))), (tuple(range(8)), (8,)),
    ]
    rng = np.random.default_rng(20)
    for _ in range(400):
        la, lb = rng.integers(0, 8, size=2)
        cases.append((tuple(rng.integers(-3, 4, size=la).tolist()), tuple(rng.integers(-3, 4, size=lb).tolist())))
    got = run(program, cases)
    assert got[6] == ("long", 13) and got[7][0] == "ok" and len(got[7][1]) == 8 and got[8] == ("long", 9) and got[9] == ("long", 14)
    assert got[10][0] == "ok" and got[11] == ("long", 9)
    assert any(g[0] == "long" for g in got[18:]) and any(g[0] == "ok" for g in got[18:])
    for (a, b), g in zip(cases, got):
        assert g == merge(a, b), (a, b, g)
        check_properties(a, b, g)
