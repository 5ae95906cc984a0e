"""CPU test of the range checks behind the five multigrid / AMG preconditioner entries (csrc/mg_params.cpp: mg_params_grid,
mg_params_amg).  The file is compiled alone into a stand-alone program (tests/mg_params_main.cpp), once under
-fsanitize=address,undefined and once plain, and fed the table tests/golden/mg_params_cases.json.  Status and message of every tuple
must be what the entries answered before the checks had one home: tests/golden/mg_params_parent.json, recorded on a device from
cgamd_solver_set_preconditioner_multigrid / _batched_multigrid / _amg and cgamd_dist_set_preconditioner_multigrid / _amg on a
12 x 10 x 8 system of 960 rows (f64; the batched handle 2 systems, the distributed one a single rank), one handle of each kind taking
the whole table in order.

The table holds, for every argument, the two values on each side of each limit, boxes whose plane or volume is just off, a zero
dimension, and tuples that break two rules at once (the order of the checks).  What an accepted tuple fills in is checked against
the defaults of struct MgParams (1 smoothing step, over-correction 1.6, 512 rows, 3 passes, strength 0.25): a default exactly where
0 (or -0.0) was passed, the argument everywhere else; a refused tuple leaves *out alone."""
import json
import math
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "conjugate-gradient-pyopencl_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
ENTRIES = {
    "grid": {"cgamd_solver_set_preconditioner_multigrid": ("set_preconditioner_multigrid", "-"),
             "cgamd_solver_set_preconditioner_batched_multigrid": ("set_preconditioner_batched_multigrid", "-"),
             "cgamd_dist_set_preconditioner_multigrid": ("dist_set_preconditioner_multigrid", "~(the~rank's~own~box:~n_local~rows)")},
    "amg": {"cgamd_solver_set_preconditioner_amg": ("set_preconditioner_amg", None),
            "cgamd_dist_set_preconditioner_amg": ("dist_set_preconditioner_amg", None)},
}
UNTOUCHED = -7


def table():
    spec = json.load(open(os.path.join(GOLDEN, "mg_params_cases.json")))
    recorded = json.load(open(os.path.join(GOLDEN, "mg_params_parent.json")))
    assert len(recorded) == len(spec["cases"])
    return spec["rows"], spec["cases"], recorded


@pytest.fixture(scope="module", params=["sanitized", "plain"])
def program(request, tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("mg_params") / ("main_" + request.param))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else ["-O2"]
    subprocess.check_call([cxx, "-std=c++17", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "mg_params_main.cpp"),
                           os.path.join(CSRC, "mg_params.cpp"), "-o", exe])
    return exe


def run(exe, lines):
    r = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = []
    for line in r.stdout.splitlines():
        head, _, message = line.partition(" | ")
        w = head.split()
        out.append({"status": int(w[0]), "nx": int(w[1]), "ny": int(w[2]), "nz": int(w[3]), "smooth_steps": int(w[4]), "min_rows": int(w[5]),
                    "omega": float(w[6]), "algebraic": int(w[7]), "passes": int(w[8]), "theta": float(w[9]), "message": message})
    assert len(out) == len(lines)
    return out


def input_line(kind, who, note, rows, c):
    if kind == "grid":
        return f"grid {who} {rows} {note} {c['nx']} {c['ny']} {c['nz']} {c['smooth_steps']} {c['over_correction']} {c['min_rows']}"
    return f"amg {who} {c['passes']} {c['strength']} {c['smooth_steps']} {c['over_correction']} {c['min_rows']}"


def or_default(value, default):
    return default if value == 0 else value         # (-0.0 == 0: the default)


def test_status_and_message_are_the_recorded_ones(program):
    rows, cases, recorded = table()
    asked, lines = [], []
    for c, rec in zip(cases, recorded):
        assert set(rec) == set(ENTRIES[c["kind"]]), c
        for entry, (who, note) in ENTRIES[c["kind"]].items():
            asked.append((c, entry, rec[entry]))
            lines.append(input_line(c["kind"], who, note, rows, c))
    got = run(program, lines)
    refused = 0
    for (c, entry, want), g in zip(asked, got):
        assert g["status"] == want["status"], (entry, c, g, want)
        assert g["message"] == want["message"], (entry, c, g, want)
        refused += want["status"] != 0
    assert refused >= 3 * len(asked) // 10 and len(asked) - refused >= 3 * len(asked) // 10       # the record holds both answers


def test_defaults_are_filled_only_where_zero_was_passed(program):
    rows, cases, recorded = table()
    lines = [input_line(c["kind"], "who", "-", rows, c) for c in cases]
    got = run(program, lines)
    seen_default, seen_given = set(), set()
    for c, rec, g in zip(cases, recorded, got):
        accepted = all(v["status"] == 0 for v in rec.values())
        assert accepted == (g["status"] == 0), c
        if not accepted:
            assert all(g[k] == UNTOUCHED for k in ("nx", "ny", "nz", "smooth_steps", "min_rows", "omega", "passes", "theta")), (c, g)
            continue
        oc = float(c["over_correction"])
        want = {"smooth_steps": or_default(c["smooth_steps"], 1), "min_rows": or_default(c["min_rows"], 512), "omega": or_default(oc, 1.6)}
        if c["kind"] == "grid":
            want.update(nx=c["nx"], ny=c["ny"], nz=c["nz"], algebraic=0, passes=3, theta=0.25)
        else:
            want.update(nx=1, ny=1, nz=1, algebraic=1, passes=or_default(c["passes"], 3), theta=or_default(float(c["strength"]), 0.25))
        for k, v in want.items():
            assert g[k] == v, (k, c, g)
        for k, arg in (("smooth_steps", c["smooth_steps"]), ("min_rows", c["min_rows"]), ("omega", oc), ("passes", c.get("passes")),
                       ("theta", float(c.get("strength", "nan")))):
            if arg is not None and not (isinstance(arg, float) and math.isnan(arg)):
                (seen_default if arg == 0 else seen_given).add(k)
    assert seen_default == seen_given == {"smooth_steps", "min_rows", "omega", "passes", "theta"}


def test_the_table_holds_both_sides_of_every_limit():
    rows, cases, recorded = table()
    grid = [c for c in cases if c["kind"] == "grid"]
    amg = [c for c in cases if c["kind"] == "amg"]

    def values(group, key):
        return {c[key] for c in group}

    for group in (grid, amg):
        assert {-1, 0, 4, 5} <= values(group, "smooth_steps")
        assert {"-0.0", "nan", "inf"} <= values(group, "over_correction") and any(float(v) < 0 for v in values(group, "over_correction"))
        assert {-1, 0} <= values(group, "min_rows")
    assert {-1, 0, 3, 4} <= values(amg, "passes")
    st = [float(v) for v in values(amg, "strength")]
    assert any(v < 0 for v in st) and 0.0 in st and 1.0 in st and any(1.0 < v < 1.0 + 1e-15 for v in st) and any(math.isnan(v) for v in st)
    planes = [c["nx"] * c["ny"] for c in grid]
    assert any(2 ** 31 - 1 < p <= 2 ** 31 + 2 ** 16 for p in planes)
    volumes = [c["nx"] * c["ny"] * c["nz"] for c in grid if min(c["nx"], c["ny"], c["nz"]) > 0]
    assert rows - 1 in volumes and rows + 1 in volumes and rows in volumes
    assert all(any(c[d] == 0 for c in grid) for d in ("nx", "ny", "nz"))
    assert sum(c["note"].startswith("two rules") for c in grid) >= 2 and sum(c["note"].startswith("two rules") for c in amg) >= 2
    # the record was taken from all five entries, and a refusal is CGAMD_ERR_INVALID with the entry's own name in front
    for c, rec in zip(cases, recorded):
        for entry, (who, _) in ENTRIES[c["kind"]].items():
            assert rec[entry]["status"] in (0, 1)
            assert rec[entry]["message"].startswith(who + ": ") == (rec[entry]["status"] == 1)
