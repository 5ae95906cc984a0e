"""CPU tests of tests/cg_step_ref.py, the host restatement the device module test_gpu_cg_steps.py compares with bit for bit.

* accuracy: the restated partials, sums and alpha stay inside the bounds derived in cg_step_ref's docstring against np.longdouble, and
  eight restated iterations agree with cg_oracle.cg / cg_numpy.pcg_diag at the suite's tolerances (1e-10 for the 64-bit types, 1e-4 for
  the 32-bit ones): the restatement is the recurrence.
* the mutation table: a CONDITION on the inputs, not a measurement.  For the input sets of the device module (same generators, same
  seeds: cg_step_ref.cases()), every mutation of cg_step_ref.Rules must change at least one compared bit in every (kernel group x value
  type) cell where it applies; where it cannot apply the table says why.  The three groups of very large systems (fold, unrolled,
  alpha2) exist for the alpha launch alone: there a mutation is judged on alpha, formed from the restated d.q partials.
* valid inputs: nothing formed in T from the chosen inputs is subnormal, infinite or NaN, and no accumulator is -0 (cg_step_ref pads
  with +0, and the sign of a NaN or the flushing of a subnormal would make host and device differ for reasons that are no bugs).

Observation behind the choice of inputs (measured with this module's mutations): with N(0, 1) data in float32 every r.r partial of a
256-thread work-group has the same bits under any order -- 24-bit products add exactly in double -- which is why the inputs spread
over 2^+-16 and why the partials and scalars themselves are compared, not only x, r, d and the history."""
import numpy as np
import pytest

import cg_numpy
import cg_oracle
import cg_step_ref as C
import spmv_ref as R

CASES = C.cases()
SMALL = [c for c in CASES if c["group"] not in C.LARGE_GROUPS]
LARGE = [c for c in CASES if c["group"] in C.LARGE_GROUPS]

MUTATIONS = {
    "wave sums pairwise": dict(waves="pairwise"),
    "lanes summed sequentially": dict(tree="sequential"),
    "member-blocked <-> strided": dict(swap_blocked=True),
    "pack values after the strided pass": dict(pack_after=True),
    "tail first": dict(tail_first=True),
    "accumulation in T": dict(acc_in_T=True),
    "d.q not rounded to T": dict(dq_unrounded=True),
    "textbook complex division": dict(textbook_div=True),
    "cg_alpha2 in one pass": dict(alpha2_onepass=True),
}
MUTATIONS.update({f"contracted {name}": dict(contract=name) for name in C.CONTRACTIBLE})


def applies(mut, group, dt):
    """True, or the reason the mutation cannot change anything in this cell (one entry, `tail first` in `stride`, is a mutation that can
    but is not required to: it says so)"""
    cplx, narrow, E = dt in ("c64", "c128"), dt in ("f32", "c64"), C.pack_values(C.DT[dt])
    large = group in C.LARGE_GROUPS
    hidden = "alpha = T(delta / T(d.q)): rounding the double sum to float32 hides its order (all but 2^-29 of the draws)"
    if mut in ("wave sums pairwise", "lanes summed sequentially"):
        return hidden if large and narrow else True
    if mut == "member-blocked <-> strided":
        if narrow:
            return hidden.replace("alpha = T(delta / T(d.q))", "every prologue sum is rounded to T before it is used")
        return True if group in ("loops", "pcg", "wide") or large else "at most 256 partials: both orders give thread t the partial t"
    if mut == "d.q not rounded to T":
        return True if narrow else "T is the accumulator type"
    if mut == "textbook complex division":
        if dt == "c64":
            return "the quotient of two widened float32 pairs is rounded to float32: both algorithms give its bits"
        return True if cplx else "real division is one operation"
    if mut == "cg_alpha2 in one pass":
        if group == "alpha2" and narrow:
            return hidden
        return True if group == "alpha2" else "no cg_alpha2 launch below 16384 partials"
    if large:
        return "judged at the small sizes: the group exists for its alpha launch"
    if mut == "pack values after the strided pass":
        if E == 1:
            return "one value per pack"
        return True if group == "stride" else "one pack per thread"
    if mut == "tail first":
        if E == 1:
            return "one value per pack: no tail"
        if group == "stride":
            # (it DOES apply here -- n = 5003 with pad_rows = 0 has a tail -- but the tail is one value in one thread of 256 and more
            # and the block sum absorbs its place: 1 of 200 draws at n = 1001, none of 200 at n = 5003.  The rule is pinned by `edges`)
            return "not required here, judged in edges: a seed in which the block sum does not absorb the tail's place is 1 draw of 200 or fewer"
        return True if group == "edges" else "sizes are whole packs (appended rows)"
    if mut == "accumulation in T":
        return True if narrow else "T is the accumulator type"
    name = mut.replace("contracted ", "")
    if name == "dot":
        return True if cplx else "a real product is one operation"
    if name == "mr":
        if not cplx:
            return "a real product is one operation"
        return True if group in ("pcg", "wide") else "no preconditioner"
    if name == "pcg_dir":
        return True if group in ("pcg", "wide") else "no preconditioner"
    if name == "aypx":
        return True if group != "pcg" else "the preconditioned direction is pcg_dir"
    return True


def run_small(case, rules, cache, inputs=None):
    """the states after set_rhs and after every iteration"""
    st, inp = C.build_steps(case, rules=rules, cache=cache, inputs=inputs)
    states = [st.state()]
    for _ in range(case["iters"]):
        st.iterate(1)
        states.append(st.state())
    return states, inp


def differs(a, b):
    return any(not R.bit_equal(sa[k], sb[k]) for sa, sb in zip(a, b) for k in sa)


_BASE = {}


def baseline(case):
    if case["id"] not in _BASE:
        cache = {}
        watch = C.Watch()
        st, inp = C.build_steps(case, watch=watch, cache=cache)
        states = [st.state()]
        for _ in range(case["iters"]):
            st.iterate(1)
            states.append(st.state())
        _BASE[case["id"]] = (states, inp, cache if case["group"] not in C.LARGE_GROUPS else None, watch)
    return _BASE[case["id"]]


def test_case_table_is_what_the_issue_lists():
    ids = [c["id"] for c in CASES]
    assert len(set(ids)) == len(ids)
    groups = {c["group"] for c in CASES}
    assert groups == {"edges", "stride", "loops", "lag", "pcg", "wide", "fold", "unrolled", "alpha2"}
    plans = {c["id"]: C.host_plan(c) for c in CASES}
    by = lambda g: [c for c in CASES if c["group"] == g]
    assert {plans[c["id"]]["n_partials"] for c in by("fold")} == {2048, 2049} and [plans[c["id"]]["fold"] for c in by("fold")] == [1, 0]
    assert {plans[c["id"]]["n_partials"] for c in by("unrolled")} == {9221} and all(plans[c["id"]]["alpha2"] == 0 for c in by("unrolled"))
    assert {plans[c["id"]]["n_partials"] for c in by("alpha2")} == {16384, 16391} and all(plans[c["id"]]["alpha2"] == 1 for c in by("alpha2"))
    assert any(plans[c["id"]]["vec"] == 0 for c in by("edges")) and any(plans[c["id"]]["n"] != c["n"] for c in by("edges"))
    # grid-stride rounds: 3 to 10 packs per thread
    per_thread = {-(-(plans[c["id"]]["n"] // C.pack_values(C.DT[c["dt"]])) // (plans[c["id"]]["vgrid"] * 256)) for c in by("stride") if "vec_grid" in c["id"]}
    assert min(per_thread) >= 2 and max(per_thread) <= 20 and len(per_thread) >= 3, per_thread
    # wave order is judged on at least 8 work-groups
    assert any(plans[c["id"]]["vgrid"] >= 8 for c in by("loops"))


@pytest.mark.parametrize("dt", list(C.DT))
def test_restated_steps_stay_inside_the_bounds(dt):
    dtype = C.DT[dt]
    picked = []
    for group in ("stride", "loops", "pcg", "lag"):       # two cases of every group, the eight-launch loop aside (its d.q partials are overwritten)
        picked += [c for c in SMALL if c["dt"] == dt and c["group"] == group and c["n"] < 10000 and C.UNFUSED not in c["flags"]][:2]
    assert len(picked) == 8
    for case in picked:
        states, inp, cache, _ = baseline(case)
        plan = C.host_plan(case)
        E = C.pack_values(dtype)
        pcg, two = bool(case.get("jacobi")), bool(case.get("two"))
        m = None if inp["m"] is None else np.broadcast_to(C.pad_vectors(inp["m"], inp["m"].shape[0], case["n"], plan["n"]), states[0]["r"].shape)
        for k in range(1, len(states)):
            s = states[k]
            w = C.check_partials(s["part_rr"], s["r"], s["r"], dtype, plan["vgrid"], E, plan["vec"], case["id"])
            w2 = C.check_partials(s["part_dq"], s["q"], s["d"] if two else states[k - 1]["d"], dtype, plan["n_partials"], 1, False, case["id"])
            ws = C.check_sum(s["history"][-1], s["part_rr"], dtype, case["id"])
            print(case["id"], k, "partials", w, w2, "sum", ws)
            if pcg:
                z = C.Ops(dtype).mr(m, s["r"])
                print("  r.z", C.check_partials(s["part_rz"], s["r"], z, dtype, plan["vgrid"], E, plan["vec"], case["id"]),
                      "rho", C.check_sum(s["delta"], s["part_rz"], dtype, case["id"]))
            if not R.is_complex(dtype):
                print("  alpha", C.check_alpha(s["alpha"], states[k - 1]["delta"], s["part_dq"], dtype, case["id"]))


@pytest.mark.parametrize("dt", list(C.DT))
@pytest.mark.parametrize("jacobi", [None, "shared"])
def test_eight_restated_iterations_agree_with_the_oracles(dt, jacobi):
    dtype = C.DT[dt]
    n, nrhs = 3001, 2
    tol = 1e-10 if dt in ("f64", "c128") else 1e-4
    rng = np.random.default_rng(5)
    ip, ix, da = C.chain_matrix(n, dtype)
    B = np.stack([(1.0 + R.rand_values(rng, n, dtype)).astype(dtype) for _ in range(nrhs)])
    wide = C.acc_type(dtype)
    m = (1.0 / da[ip[:-1] + (np.arange(n) > 0)]).astype(dtype) if jacobi else None
    case = {"dt": dt, "n": n, "nrhs": nrhs, "knobs": dict(C.LAUNCHED), "flags": (), "jacobi": jacobi}
    plan = C.host_plan(case)
    nt = plan["n"]
    st = C.Steps(C.pad_system(ip, nt), ix, da, dtype, nrhs, plan, m=None if m is None else C.pad_vectors(m, 1, n, nt))
    st.set_rhs(C.pad_vectors(B, nrhs, n, nt)).iterate(8)
    hist, x = np.stack(st.history), st.x[:, :n]
    if jacobi:
        for r in range(nrhs):
            xo, _, ho = cg_numpy.pcg_diag(ip, ix, da.astype(wide), B[r].astype(wide), m=m.astype(wide), tol=0.0, maxit=8, history=True)
            assert np.max(np.abs(hist[:, r] - ho) / np.abs(ho)) < tol
            assert np.linalg.norm(x[r] - xo) / np.linalg.norm(xo) < tol
    else:
        xo, ho = cg_oracle.cg(ip, ix, da.astype(wide), B.reshape(-1).astype(wide), nrhs=nrhs, n_iterations=8, mode=cg_oracle.MODE_SEQUENTIAL)
        assert np.max(np.abs(hist - ho) / np.abs(ho)) < tol
        assert np.linalg.norm(x.reshape(-1) - xo) / np.linalg.norm(xo) < tol


def test_inputs_are_valid():
    """nothing subnormal, infinite or NaN in T, no accumulator -0, on every input set of the device module"""
    for case in CASES:
        watch = baseline(case)[3]
        assert watch.seen > 0 and watch.bad_T == 0 and watch.neg_zero == 0, (case["id"], watch.bad_T, watch.neg_zero)


def test_every_mutation_is_detected_in_every_cell_where_it_applies():
    cells = sorted({(c["group"], c["dt"]) for c in CASES})
    table, missed = {}, []
    for group, dt in cells:
        members = [c for c in CASES if c["group"] == group and c["dt"] == dt]
        for mut, kw in MUTATIONS.items():
            why = applies(mut, group, dt)
            if why is not True:
                table[(group, dt, mut)] = "n/a: " + why
                continue
            rules = C.Rules(**kw)
            hit = 0
            for case in members:
                states, inp, cache, _ = baseline(case)
                if group in C.LARGE_GROUPS:
                    plan, dtype = C.host_plan(case), C.DT[dt]
                    got = C.alpha_value(states[1]["part_dq"], states[0]["delta"], plan, dtype, rules)
                    assert R.bit_equal(C.alpha_value(states[1]["part_dq"], states[0]["delta"], plan, dtype), states[1]["alpha"])
                    hit += not R.bit_equal(got, states[1]["alpha"])
                else:
                    hit += differs(run_small(case, rules, cache, inp)[0], states)
            table[(group, dt, mut)] = f"{hit}/{len(members)}"
            if hit == 0:
                missed.append((group, dt, mut))
    for mut in MUTATIONS:
        print(f"\n{mut}")
        for group, dt in cells:
            print(f"    {group:9s} {dt:5s} {table[(group, dt, mut)]}")
    assert not missed, "\n".join(map(str, missed))
