"""CPU tests of tests/rowmajor_ref.py, the host restatement tests/test_gpu_rowmajor_steps.py compares the row-major loop with.

* the inputs are what the device module's docstring says they are: the random pattern holds its empty quad, empty strip, quads of 32
  and 33 entries and its row of 77; the grids reach TQ 5 / a second round of TQ 8; under dev.spmm_wgs = 1 every wave makes 3 or 4 steps,
  under the default grid the random system leaves waves of every XCD idle and the grids give every wave one strip.
* the strip assignment hands every strip to exactly one wave; the restated recurrence is the CG recurrence.
* the mutation table: a CONDITION on the inputs, not a measurement.  On the very inputs of the device cases (rowmajor_ref.spmm_inputs /
  loop_inputs: same generators, same seeds) every plausible mistake must be caught in every (type, width) cell where it applies:
  the three mistakes inside the SpMM (`spmm_model` faults) must fail BOTH q checks -- the integer-exact compare and the format bound --,
  the others must change a compared bit of the restated state.  Where a mistake cannot show, `applies` says why.
  The stand-in for the device's q on the host is the longdouble product rounded to T: the restatement starts behind q."""
import numpy as np
import pytest

import cg_step_ref as C
import rowmajor_ref as M
import spmv_ref as R

IDS = [f"{dt}x{w}" for dt, w in M.WIDTHS]
LOOP_SYSTEMS = ("grid5", "random")

Q_FAULTS = ("neighbour_row", "drop_round", "row_map")
MUTATIONS = {
    "output-slot row maps swapped": dict(row_map_swapped=True),
    "strips round-robin over all waves": dict(round_robin=True),
    "partial stored at [wg][c]": dict(partial_wg_major=True),
    "shuffle tree from off = 1": dict(tree_from_1=True),
    "waves summed pairwise": dict(waves="pairwise"),
    "complex re with +": dict(re_plus=True),
    "alpha / beta of column c + 1": dict(next_column=True),
    "products accumulated in T": dict(acc_in_T=True),
    "contracted r update": dict(contract="axmy"),
    "contracted x update": dict(contract="axpy"),
    "contracted d update": dict(contract="aypx"),
    "x updated with the new d": dict(x_new_d=True),
}


def applies(mut, dt):
    narrow, cplx = dt in ("f32", "c64"), dt == "c64"
    if mut == "output-slot row maps swapped" and narrow:
        # under the grid of the loop cases a wave has one strip: the 16 products of a column meet in the wave sum under either map
        return "the 16 float32 products of a strip add exactly in double under either map (the q checks catch the map: the store " \
               "and the d.q sum take their row from the same lrow(i))"
    if mut == "complex re with +":
        return True if cplx else "real type"
    if mut == "products accumulated in T":
        return True if narrow else "T is the accumulator type"
    return True


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------
def test_patterns_hold_what_the_device_cases_need():
    ip, ix = M.pattern("random")
    n = len(ip) - 1
    cnt = np.diff(ip)
    quad = np.add.reduceat(cnt, np.arange(0, n, 4))
    assert n == 1543 and n % 16 == 7
    assert (cnt == 0).sum() > 100 and cnt[777] == 77
    assert quad[10] == 0 and not cnt[160:176].any() and quad[50] == 32 and quad[75] == 33
    assert any(np.any(np.diff(ix[ip[i]:ip[i + 1]]) < 0) for i in range(n)), "columns are sorted"
    assert all(len(set(ix[ip[i]:ip[i + 1]])) == cnt[i] for i in range(n)), "duplicate columns"
    assert M.max_quad(ip) > 32 and sorted(set(quad[quad > 32])) [0] == 33
    ip5, _ = M.pattern("grid5")
    ip9, _ = M.pattern("grid9")
    assert len(ip5) - 1 == 1521 and 1521 % 16 == 1 and M.max_quad(ip5) == 20
    assert M.max_quad(ip9) == 36 and M.host_plan(ip9, np.float64, 16)["tq_fused"] == 8 and M.host_plan(ip5, np.float64, 16)["tq_fused"] == 5
    for name in M.SMALL_N:
        ips, _ = M.pattern(str(name))
        assert len(ips) - 1 == name and 0 < M.max_quad(ips) <= 20


@pytest.mark.parametrize("name", list(M.SYSTEMS) + [str(n) for n in M.SMALL_N])
def test_strips_are_dealt_once_and_the_grids_reach_their_paths(name):
    ip, _ = M.pattern(name)
    n = len(ip) - 1
    for knobs in ({}, {"dev.spmm_wgs": 1}):
        plan = M.host_plan(ip, np.float32, 16, knobs)
        nwg, strips = plan["nwg_fused"], plan["strips"]
        seen = sorted(s for wg in range(nwg) for w in range(4) for s in M.strips_of(wg, w, nwg, strips))
        assert seen == list(range(strips))
        assert np.array_equal(np.bincount(M.row_groups(n, nwg), minlength=nwg), [16 * sum(len(M.strips_of(wg, w, nwg, strips)) for w in range(4))
                                                                                 - (16 * strips - n) * any(strips - 1 in M.strips_of(wg, w, nwg, strips) for w in range(4))
                                                                                 for wg in range(nwg)])
        steps = M.wave_steps(nwg, strips)
        if name in M.SYSTEMS and knobs:          # W = 4 waves per XCD: both pipeline buffers; random (97 strips) leaves the step loop by both exits
            assert nwg == 8 and set(steps.reshape(-1)) == ({3, 4} if name == "random" else {3}) and plan["paced_fused"] == 8
        elif name == "random":                   # W = 16 > the 12 or 13 strips of an XCD: idle waves, nothing paces
            assert nwg == 32 and set(steps.reshape(-1)) == {0, 1} and plan["paced_fused"] == 0
        elif name in M.SYSTEMS:                  # 96 strips: W = 12 = the strips of every XCD, one step per wave, the pacing rule at its threshold
            assert nwg == 24 and set(steps.reshape(-1)) == {1} and plan["paced_fused"] == 8
        elif name == "100":
            assert strips == 7 and any(not steps[wg::8].any() for wg in range(8)), "no XCD without a strip"


def test_restated_recurrence_is_cg():
    """three restated iterations on an SPD system against the textbook recurrence in longdouble"""
    ip, ix = M.pattern("grid5")
    n = len(ip) - 1
    rows = np.repeat(np.arange(n), np.diff(ip))
    da = np.where(rows == ix, 4.5, -1.0)
    rng = np.random.default_rng(3)
    B = M.values(rng, (16, n), np.float64, "rand")
    plan = M.host_plan(ip, np.float64, 16)
    st = M.RmSteps(np.float64, 16, plan).set_rhs(B, None, np.zeros((16, n)))

    def mul(v):
        out = np.zeros(v.shape, M.LD)
        for r in range(16):
            np.add.at(out[r], rows, da.astype(M.LD) * v[r, ix])
        return out
    x, r = np.zeros((16, n), M.LD), B.astype(M.LD)
    d, hist = r.copy(), [(r * r).sum(axis=1)]
    for _ in range(3):
        st.iterate(M.spmm_model(ip, ix, da, st.d, np.float64))
        q = mul(d)
        al = hist[-1] / (d * q).sum(axis=1)
        x, r = x + al[:, None] * d, r - al[:, None] * q
        hist.append((r * r).sum(axis=1))
        d = r + (hist[-1] / hist[-2])[:, None] * d
    assert np.max(np.abs(np.stack(st.history) - np.stack(hist)) / np.stack(hist)) < 1e-12
    assert np.max(np.abs(st.x - x)) / np.max(np.abs(x)) < 1e-12


# ---- the q checks reject the mistakes inside the SpMM ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,nrhs", M.WIDTHS, ids=IDS)
@pytest.mark.parametrize("name", list(M.SYSTEMS) + ["17", "129"])
def test_q_checks_accept_the_product_and_reject_the_faults(name, dt, nrhs):
    dtype = M.DT[dt]
    ip, _ = M.pattern(name)
    tq = M.host_plan(ip, dtype, nrhs)["tq_plain"]
    for kind, check in (("int", M.check_q_exact), ("rand", M.check_q_bound)):
        ip, ix, da, X = M.spmm_inputs(name, dt, nrhs, kind)
        check(M.spmm_model(ip, ix, da, X, dtype, tq), ip, ix, da, X, dtype, f"{name} {dt}x{nrhs} {kind}")
        for fault in Q_FAULTS:
            if fault == "drop_round" and M.max_quad(ip) <= 4 * tq:
                continue                      # every quad fits one round: judged on grid9 and random
            bad = M.spmm_model(ip, ix, da, X, dtype, tq, fault)
            with pytest.raises(AssertionError):
                check(bad, ip, ix, da, X, dtype, f"{name} {dt}x{nrhs} {kind} {fault}")
    assert name not in ("grid9", "random") or M.max_quad(ip) > 4 * tq


def test_a_row_without_entries_must_be_plus_zero():
    ip, ix, da, X = M.spmm_inputs("random", "f32", 16, "rand")
    q = M.spmm_model(ip, ix, da, X, np.float32)
    q[3, 41] = -0.0
    with pytest.raises(AssertionError):
        M.check_q_bound(q, ip, ix, da, X, np.float32, "minus zero")


# ---- the mutation table ---------------------------------------------------------------------------------------------------------------------
def _run(name, dt, nrhs, rules, qs=None, knobs=None):
    """set_rhs and three iterations on the "rand" inputs of the loop case; qs: the q of every step (default: the model's, from the
    restatement's own x0 / d).  Returns (states after every step, qs)"""
    dtype = M.DT[dt]
    ip, ix, da, B, X0 = M.loop_inputs(name, dt, nrhs, "rand")
    plan = M.host_plan(ip, dtype, nrhs, knobs)
    tq = plan["tq_fused"]
    st = M.RmSteps(dtype, nrhs, plan, rules)
    made = []
    q = qs[0] if qs else M.spmm_model(ip, ix, da, X0, dtype, tq)
    made.append(q)
    st.set_rhs(B, X0, q)
    states = [{k: np.copy(v) for k, v in st.state().items()}]
    for k in range(3):
        q = qs[k + 1] if qs else M.spmm_model(ip, ix, da, st.d, dtype, tq)
        made.append(q)
        st.iterate(q)
        states.append({k_: np.copy(v) for k_, v in st.state().items()})
    return states, made


_EXACT = {}


def _exact(name, dt, nrhs):
    if (name, dt, nrhs) not in _EXACT:
        _EXACT[name, dt, nrhs] = _run(name, dt, nrhs, M.EXACT)
    return _EXACT[name, dt, nrhs]


@pytest.mark.parametrize("dt,nrhs", M.WIDTHS, ids=IDS)
def test_inputs_are_valid(dt, nrhs):
    """nothing of the restated states is subnormal, infinite or NaN, and no partial is -0"""
    for name in LOOP_SYSTEMS:
        states, _ = _exact(name, dt, nrhs)
        w = C.Watch()
        for s in states:
            for k, v in s.items():
                if k.startswith("part"):
                    w.note_acc(v)
                elif k != "iter":
                    w.note_T(v)
        assert w.bad_T == 0 and w.neg_zero == 0 and w.seen > 0


@pytest.mark.parametrize("dt,nrhs", M.WIDTHS, ids=IDS)
@pytest.mark.parametrize("mut", list(MUTATIONS))
def test_every_mutation_changes_a_compared_bit(mut, dt, nrhs):
    why = applies(mut, dt)
    changed = set()
    for name in LOOP_SYSTEMS:          # (one kernel instance per cell but for TQ, which no rule below reads: a cell is judged on both systems)
        want, qs = _exact(name, dt, nrhs)
        got, _ = _run(name, dt, nrhs, M.Rules(**MUTATIONS[mut]), qs)
        changed |= {k for a, b in zip(got, want) for k in M.differing(a, b)}
    if why is True:
        assert changed, f"{mut} on {dt}x{nrhs}: no compared bit changes"
    else:
        assert not changed, f"{mut} on {dt}x{nrhs} shows in {sorted(changed)}, the table says: {why}"


def test_vec_grid_2_walks_many_rounds_with_a_partial_last_one():
    """the vec_grid = 2 case of the device module: 512 threads, more than one grid-stride round, the last one partial"""
    for dt, nrhs in M.WIDTHS:
        ip, _ = M.pattern("random")
        plan = M.host_plan(ip, M.DT[dt], nrhs, {"vec_grid": 2})
        npack = plan["n"] * nrhs // C.pack_values(M.DT[dt])
        assert plan["vgrid"] == 2 and npack > 512 * 12 and npack % 512 != 0


def test_integer_partials_need_no_order():
    """on the integer loop inputs the restated d.q partials are the integer sums over the rows of each work-group"""
    for dt, nrhs in (("f64", 16), ("f32", 64), ("c64", 32)):
        dtype = M.DT[dt]
        ip, ix, da, B, _ = M.loop_inputs("random", dt, nrhs, "int")
        plan = M.host_plan(ip, dtype, nrhs)
        q = M.q_integer(ip, ix, da, B, dtype)
        assert R.bit_equal(M.dq_partials(B, q, dtype, plan["nwg_fused"]), M.dq_integer(B, q, dtype, plan["nwg_fused"]))
