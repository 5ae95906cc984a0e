"""CPU test of the SpMV form decision (csrc/spmv_form.cpp choose_spmv_form): the function the launcher launches from and the solver's
accessors and byte models ask.  The file is compiled alone into a stand-alone program (tests/spmv_form_main.cpp), once under
-fsanitize=address,undefined and once plain, and fed the table tests/golden/spmv_form_parent.json: per case the ints of
cgamd_solver_spmv_form's `inputs` (call, plan, tuning) and the cgamd_last_spmv_form record of the launch the PARENT build made for
that call, each case in a process of its own (scripts/record_spmv_form.py; small matrices of tests/spmv_ref.py, at most 2301 rows).
Rules no small matrix reaches -- the n * sizeof(T) >= 2^30 gate, a row-block list, an empty one -- are cases written by hand, their
form read off the parent's condition, marked "derived": at most a tenth of the table."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "conjugate-gradient-pyopencl_amd", "csrc")
FORM_FIELDS = ("family", "vec", "width", "index_bits", "value_codes", "nt", "fused", "wide", "grid", "partials")


LAUNCH_FIELDS = ("grid_y", "depth", "pair_slots", "table", "cycle", "cap", "chunk", "body", "lds")


def launch_fields(i, form):
    """what the launch of the RECORDED form needs beyond the record, by the formulas of the launcher before the decision had one home
    (spmv_impl of the parent commit): LDS slice capacity and bytes, schedule cycle, pipeline depth, pair slots, SpMM chunk"""
    V, acc, nrhs, fam = i["c.value_bytes"], i["c.acc_bytes"], i["c.nrhs"], form["family"]
    out = dict.fromkeys(LAUNCH_FIELDS, 0)
    out["grid_y"] = 1
    cycle = i["t.spmv_cycle"] if i["t.spmv_cycle"] > 0 else 1
    up4, up16 = (lambda v: (v + 3) & ~3), (lambda v: (v + 15) & ~15)

    def slice_lds(cap, bits):
        return up16(cap * (V + 1)) if bits == 8 else up16(cap * (V + 2)) if bits == 16 else cap * (V + 4)
    depth = i["t.dev_row_pipe"] if i["t.dev_row_pipe"] in (1, 2, 4) else 4 if V <= 4 else 1
    if fam == 9:
        out["body"] = int(i["plan.lr.n_regular"] > 0)
    elif fam == 0:
        out["lds"] = acc * nrhs * 4 if form["fused"] and nrhs > 1 else 0
    elif fam == 4:
        lv = {2: 0, 4: 1, 8: 2, 16: 3, 32: 4}[form["width"]]
        out.update(cap=up4(i[f"plan.chunk_span[{lv}]"]), cycle=cycle)
        out["lds"] = slice_lds(out["cap"], form["index_bits"])
    elif fam == 5:
        out.update(cap=up4(i["plan.max_span"]), cycle=cycle, chunk=i["t.spmm_rb"] if 0 < i["t.spmm_rb"] < nrhs else nrhs)
        out["lds"] = out["cap"] * (V + 4) + acc * nrhs * 4
    else:
        out.update(cap=up4(i["plan.max_span"]), cycle=cycle)
        if fam == 1:
            out.update(grid_y=nrhs, lds=slice_lds(out["cap"], form["index_bits"]))
        else:
            out["cycle"] = max(1, cycle // 4)
            if fam in (2, 3):
                out["lds"] = up16(out["cap"] * 4) + 16
            elif fam == 7:
                out.update(depth=depth, table=i["plan.sched"], lds=i["plan.n_patterns"] * (8 * V + 36))
            else:
                np_ = i["plan.n_pair_patterns"]
                out.update(depth=min(2, depth), table=i["plan.sched"], pair_slots=7 if i["plan.pair_slots"] <= 7 else 8,
                           lds=2 * np_ * 8 * V + np_ * 8 * 4 + np_ * 4)
    return out


def table():
    t = json.load(open(os.path.join(ROOT, "tests", "golden", "spmv_form_parent.json")))
    return t["names"], t["cases"]


@pytest.fixture(scope="module", params=["sanitized", "plain"])
def program(request, tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("spmv_form") / ("main_" + request.param))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else ["-O2"]
    subprocess.check_call([cxx, "-std=c++17", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "spmv_form_main.cpp"),
                           os.path.join(CSRC, "spmv_form.cpp"), "-o", exe])
    return exe


def test_every_case_gets_the_form_the_parent_launched(program):
    names, cases = table()
    r = subprocess.run([program, "names"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == names, "the table was recorded for another layout of the inputs"
    r = subprocess.run([program], input="".join(" ".join(str(v) for v in c["inputs"]) + "\n" for c in cases), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = r.stdout.splitlines()
    assert len(got) == len(cases)
    for c, line in zip(cases, got):
        record, _, launch = line.partition(" | ")
        want = "none" if c["form"] is None else " ".join(str(c["form"][k]) for k in FORM_FIELDS)
        assert record == want, (c["label"], dict(zip(FORM_FIELDS, record.split())), c["form"])
        if c["form"] is not None:
            got_launch = dict(zip(LAUNCH_FIELDS, (int(v) for v in launch.split())))
            assert got_launch == launch_fields(dict(zip(names, c["inputs"])), c["form"]), (c["label"], got_launch)


def test_derived_cases_are_at_most_a_tenth():
    _, cases = table()
    derived = [c for c in cases if c.get("derived")]
    assert derived and 10 * len(derived) <= len(cases), (len(derived), len(cases))


def test_the_table_holds_both_sides_of_every_gate():
    names, cases = table()
    col = {k: {c["inputs"][i] for c in cases} for i, k in enumerate(names)}
    forms = [c["form"] for c in cases if c["form"] is not None]
    launched = {k: {f[k] for f in forms} for k in FORM_FIELDS}
    # every family of the DESIGN section 2 table, every template argument the forms are launched with
    assert launched["family"] == {0, 1, 2, 3, 4, 5, 7, 8, 9}
    assert {4, 5, 7, 8} <= {f["width"] for f in forms if f["family"] in (1, 2, 3, 7, 8)}
    assert {2, 4, 8, 16, 32} == {f["width"] for f in forms if f["family"] == 4}
    assert {2, 3, 4, 5, 6, 8} == {f["width"] for f in forms if f["family"] == 5}
    assert launched["index_bits"] == {0, 8, 16} and launched["value_codes"] == {0, 1, 2, 3}
    assert launched["nt"] == launched["fused"] == launched["wide"] == launched["vec"] == {0, 1}
    assert any(c["form"] is None for c in cases)                                             # the empty row-block list
    # each boolean of SpmvCall and of the plan
    for k in ("c.vec", "c.codes_for", "c.vcodes_for", "c.rcodes_for", "c.fuse", "c.rb_list", "c.x16", "c.y16", "c.d16", "plan.wide", "plan.nt", "plan.codes", "plan.codes16",
              "plan.vcodes", "plan.jcodes", "plan.rcodes", "plan.pcodes", "plan.pdict", "plan.sched", "plan.lr.on"):
        assert col[k] == {0, 1}, k
    assert {4, 8, 16} == col["c.value_bytes"] and {8, 16} == col["c.acc_bytes"] and {1, 2} <= col["c.nrhs"]
    assert {0, 5, 6, 7} == col["plan.kind"] and {5, 7} <= col["plan.lr.body_kind"]
    assert {0, 1} <= col["c.rb_count"] and max(col["c.rb_count"]) > 1
    # each knob the decision reads, on both sides of its default
    for k, values in (("t.index_codes", {0, 1}), ("t.value_codes", {0, 1}), ("t.dev_joint_codes", {0, 1}), ("t.dev_row_codes", {0, 1}),
                      ("t.dev_vc_pipe", {0, 1}), ("t.dev_row_pipe", {0, 1, 2, 4}), ("t.dev_row_pairs", {-1, 0, 1}), ("t.spmv_nt", {-1, 0, 1}),
                      ("t.spmv_cycle", {1, 64}), ("t.spmv_unroll", {0, 4, 5}), ("t.spmm_rb", {0, 4}), ("t.spmm_group", {0, 3})):
        assert values <= col[k], (k, col[k])
    assert {7, 8} <= col["plan.pair_slots"]
    # the longest row on each side of every batch length, a slice on each side of the 2048 entries the code staging holds, rows on
    # each side of the 2^30-byte gate
    assert {3, 4, 5, 7, 8, 9} <= col["plan.max_row"]
    coded = [c for c in cases if c["inputs"][names.index("plan.vcodes")]]
    spans = {c["inputs"][names.index("plan.max_span")] for c in coded}
    assert any(s <= 2048 for s in spans) and any(s > 2048 for s in spans)
    rows8 = {c["inputs"][names.index("c.n")] for c in coded if c["inputs"][names.index("c.value_bytes")] == 8}
    assert (1 << 27) in rows8 and any((1 << 27) - 256 < n < (1 << 27) for n in rows8)
    # depths and slots as launched are not in the record: their inputs are, and the accessor test reads the depth on the device
    pair = [c for c in cases if c["form"] and c["form"]["family"] == 8]
    assert {7, 8} <= {c["inputs"][names.index("plan.pair_slots")] for c in pair}
    # the three alignments apart: each alone keeps a handle with pair codes on the row form, dvec only where the dot is fused
    def aligned(c):
        return tuple(c["inputs"][names.index(k)] for k in ("c.x16", "c.y16", "c.d16", "c.fuse"))
    with_pairs = [c for c in cases if c["inputs"][names.index("plan.pcodes")] and c["form"]["family"] in (7, 8)]
    by_family = {fam: {aligned(c) for c in with_pairs if c["form"]["family"] == fam} for fam in (7, 8)}
    assert {(1, 0, 1, 1), (1, 1, 0, 1), (0, 1, 1, 0), (0, 1, 0, 1)} <= by_family[7]
    assert {(1, 1, 1, 1), (1, 1, 1, 0), (1, 1, 0, 0)} <= by_family[8]
    assert {0, 1, 4} <= {c["inputs"][names.index("t.dev_row_pipe")] for c in pair}
