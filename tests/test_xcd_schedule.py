"""CPU test of the plane-matched XCD schedule behind the row- and pair-coded SpMV (csrc/xcd_schedule.cpp build_xcd_schedule): table[b]
is the super block XCD b % 8 runs as its (b / 8)-th work-group.  The C++ function is compiled together with a stand-alone program
(tests/xcd_schedule_main.cpp) under -fsanitize=address,undefined and run as a program.  Checked for every case: every super block
appears exactly once, every other entry is -1, the entries of one XCD ascend, the grid is 8 x the longest list, and super block s sits
on XCD floor(8 frac(centre(s) / unit_rows)), centre(s) = s rows_per_super + rows_per_super / 2, restated here in exact integers.
For the headline (9766 super blocks of 1024 rows, unit 50 000) the super blocks that hold rows r and r + 50 000 share an XCD for at
least 85 % of r: the two centres differ from 50 000 by 176 or 848 rows (50 000 = 48 x 1024 + 848), an eighth of the unit is 6250 rows,
so about 2 x 176 x 848 / 1024 / 6250 = 4.7 % of the rows fall apart -- the table gives 95.3 %.  xcd_schedule_balanced, the default
rule's last condition, is checked against the lists of nine 3-D systems: the measured ones pass, planes of 9, 10, 12, 20 and 36 super
blocks -- two blocks of every plane on one XCD, launches 1.11 to 1.78 times as long -- are declined."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "conjugate-gradient-pyopencl_amd", "csrc")

SUPERS = (1, 7, 8, 9, 48, 49, 977, 9766)
UNITS = (1024, 1500, 8192, 50_000, 215_296, 10**7, 10**9)
ROWS_PER_SUPER = 1024


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("xcd_schedule") / "schedule_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "xcd_schedule_main.cpp"), os.path.join(CSRC, "xcd_schedule.cpp"), "-o", exe])
    return exe


def run(exe, cases):
    text = "".join(f"{s} {rps} {u}\n" for s, rps, u in cases)
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = []
    for line in r.stdout.splitlines():
        v = list(map(int, line.split()))
        assert v[1] == len(v) - 3, "the table is as long as the program says"
        out.append((v[0], np.array(v[3:], dtype=np.int64), bool(v[2])))
    assert len(out) == len(cases)
    return out


def xcd_formula(s, rps, unit):
    centre = s * rps + rps // 2
    return 8 * (centre % unit) // unit        # exact: Python integers


@pytest.fixture(scope="module")
def tables(program):
    cases = [(s, ROWS_PER_SUPER, u) for s in SUPERS for u in UNITS]
    return dict(zip(cases, run(program, cases)))


@pytest.mark.parametrize("unit", UNITS)
@pytest.mark.parametrize("supers", SUPERS)
def test_table_is_a_schedule(tables, supers, unit):
    grid, table, _ = tables[(supers, ROWS_PER_SUPER, unit)]
    assert grid == len(table) and grid % 8 == 0 and grid >= 8
    real = table[table >= 0]
    assert np.array_equal(np.sort(real), np.arange(supers)), "every super block exactly once"
    assert np.all(table[table < 0] == -1), "every other entry is -1"
    lists = [table[x::8] for x in range(8)]
    longest = 0
    for x, lst in enumerate(lists):
        mine = lst[lst >= 0]
        assert np.all(np.diff(mine) > 0), f"XCD {x}: ascending"
        assert np.all(lst[len(mine):] == -1), f"XCD {x}: the padding follows the list"
        assert all(xcd_formula(int(s), ROWS_PER_SUPER, unit) == x for s in mine), f"XCD {x}: the formula's super blocks"
        longest = max(longest, len(mine))
    assert grid == 8 * longest


def test_headline_neighbours_across_the_plane_share_an_xcd(tables):
    supers, unit, n = 9766, 50_000, 250 * 200 * 200
    assert supers == -(-n // ROWS_PER_SUPER)
    grid, table, balanced = tables[(supers, ROWS_PER_SUPER, unit)]
    assert balanced
    xcd = np.full(supers, -1)
    for x in range(8):
        lst = table[x::8]
        xcd[lst[lst >= 0]] = x
    assert np.all(xcd >= 0)
    r = np.arange(n - unit)
    same = xcd[r // ROWS_PER_SUPER] == xcd[(r + unit) // ROWS_PER_SUPER]
    share = float(np.mean(same))
    print(f"rows r and r + {unit} on one XCD: {100 * share:.2f} % of r; grid {grid}, lists of "
          f"{[int(np.sum(table[x::8] >= 0)) for x in range(8)]}")
    assert share >= 0.85
    # the eight XCDs carry the same load to within a few super blocks: the launch is as long as the longest list
    assert grid <= 8 * (supers // 8 + 8)


def test_arguments_that_are_not_positive_give_no_table(program):
    for grid, table, balanced in run(program, [(0, 1024, 50_000), (5, 0, 50_000), (5, 1024, 0), (-3, 1024, -7)]):
        assert grid == 0 and len(table) == 0 and not balanced


# (grid nx, ny, nz) -> what the default rule must do with the table of its plane nx * ny; every system is above 256 MB in fp64
BALANCE = [((250, 200, 200), True), ((464, 464, 464), True),        # the measured systems: planes that drift against the super blocks
           ((96, 96, 1100), False), ((128, 80, 1000), False), ((128, 96, 800), False), ((160, 128, 500), False), ((192, 192, 300), False),
           ((256, 256, 160), True), ((512, 512, 40), True)]         # planes of 64 and 256 super blocks: multiples of 8, every XCD 8 / 32 per plane


@pytest.mark.parametrize("dims,want", BALANCE, ids=["x".join(map(str, d)) for d, _ in BALANCE])
def test_the_default_rule_takes_only_balanced_tables(program, dims, want):
    """A launch lasts as long as the longest XCD list.  A plane that is a whole number of super blocks but no multiple of 8 (96 x 96 =
    9216 rows = 9 blocks) puts two blocks of EVERY plane on the same XCD: lists of 400 and 800, a launch 1.78 times as long as the
    cycle's.  xcd_schedule_balanced, which the default rule asks (solver.cpp setup_xcd_schedule), accepts a table only where the
    longest list is at most 2 % above an eighth of the super blocks; checked here against the lists themselves."""
    n, unit = dims[0] * dims[1] * dims[2], dims[0] * dims[1]
    supers = -(-n // ROWS_PER_SUPER)
    assert unit >= 8 * ROWS_PER_SUPER and n * 7 * 12 > 256 << 20, "a system the rule would otherwise take"
    (grid, table, balanced), = run(program, [(supers, ROWS_PER_SUPER, unit)])
    longest = max(int(np.sum(table[x::8] >= 0)) for x in range(8))
    ratio = longest / (supers / 8)
    print(f"{dims}: plane {unit} rows = {unit / ROWS_PER_SUPER:.2f} super blocks, longest list {longest}, {ratio:.3f} of an eighth")
    assert grid == 8 * longest
    assert balanced == (ratio <= 1.02) == want
    if dims == (96, 96, 1100):
        assert ratio > 1.7
