"""determinize at the limits of its routes.  Every route of determinize.hip returns the same FST — the one-workgroup narrow
kernel, the device-wide launch per phase, the hand-over between them in `auto`, a level run again after the arrays
doubled, the narrow kernel launched again after its level budget — so only the counters of wfst_ctx_get_determinize_stats
show which one ran.  Without a GPU: the symbol, a literal restatement of the host loop, ph_check, the narrow kernel's exit
order and Run::reserve (predict) against closed forms written out by hand, and every input below on the limit it is
built for.  On the device: every input ON a limit and its twin one step beyond it, bit-exact against the oracle, every
counter against the prediction, under WFST_DETERMINIZE_PATH = auto, narrow and wide.

Capacities that cannot bind alone (ph_check tests six; four have a pair of inputs here):
  slots  2 * (hi + K) > slots: reserve sets slots = the power of two >= 2 * states after every change of states, so
         hi + K <= states implies 2 * (hi + K) <= 2 * states <= slots.  Whenever it is true, `hi + K > states` is true too.
  ltab   T > ltab: T is the least power of two >= max(64, 2 * K); cands is 1024 doubled some times, a power of two >= 4096,
         and ltab = the power of two >= 2 * cands = 2 * cands.  K <= cands gives 2 * K <= ltab, and ltab is a power of two
         >= 8192, so T <= ltab.  Whenever it is true, `K > cands` is true too.

The stability of ph_expand's sort cannot be seen in a result (test_sort_ties_cannot_be_observed): the sort key is (label,
dest) and what follows reads only the weights of equal keys, through plus = (b < a ? b : a), which keeps the first of two
weights that compare equal.  Two f32 that compare equal with different bits are 0.0 and -0.0 only.  A raw candidate's weight
is element weight + arc weight; an element weight is the seed's 0.0 or a quantize() result floor(v / delta + 0.5) * delta with
v = w - min >= 0 or v = -0.0, which is never -0.0 (floor(0.5) = 0.0, times delta = +0.0); and x + y is -0.0 only when both
are.  So no raw candidate is -0.0, tied candidates of equal key have equal bits, and their order changes nothing.  The
inputs still carry -0.0 arc weights: 0.0 + -0.0 = +0.0 must come out of the device as it does of the oracle.

Run::reserve's keep counts: so[hi] ends the subset of the last state of the level that waits, so every input that grows
the states reads it (parity); hnext[lo, hi) is read only when a chain is walked past a head that lies in the waiting
level: chain_across_growth, in the narrow kernel and in a wide level.  A lost entry holds whatever the new block held.

ph_lookup's `id < best` (lowest_id_*): a chain is pushed at its head, level after level, so a walk meets the ids of
different levels in descending order and the LAST match is the lowest id with or without that comparison.  Only two states
of one sequence created in the SAME wide level can sit on the chain in ascending order (their atomicExch race), which no
input can force; lowest_id_same_level is the input in which it would show."""
import functools
import time

import numpy as np
import pytest

from rustfst_amd._lib import TR_DTYPE
from oracle import model
from oracle.model import ACCEPTOR, F32, KDELTA
import helpers
from helpers import assert_flat_identical, to_device, to_oracle
from determinize_cases import (BUDGET_CHAIN, BUDGET_FAN, LAYERED, OTHER, SORT_WIDTHS, analysis, case, chain_spec,
                               det_levels, fan_then_chain, layered)

PATHS = ("auto", "narrow", "wide")
NARROW_STATES, NARROW_CANDS, BUDGET = 256, 8192, 1 << 16  # determinize.hip
FIRST_RESERVE = (1024, 4096, 4096, 4096)  # states, elements, arcs, candidates of one level
COUNTERS = ("levels", "wide_levels", "narrow_launches", "exit_wide_states", "exit_wide_cands", "exit_budget", "exit_need",
            "exit_done", "wide_need", "grow_states", "grow_elts", "grow_arcs", "grow_cands", "rehashes", "cap_states",
            "cap_elts", "cap_arcs", "cap_cands", "rounds_max")
GROW = ("grow_states", "grow_elts", "grow_arcs", "grow_cands")
CAP = ("cap_states", "cap_elts", "cap_arcs", "cap_cands")


# ---------------------------------------------------------------- restatement of the routing
def predict(figs, path="auto", budget=BUDGET, trace=None):
    """Every counter of wfst_ctx_get_determinize_stats from the per-level figures (states L, raw candidates K, new states,
    new elements, valid arcs, m): determinize_acceptor's loop, statement by statement.

    reserve(states, elts, arcs, cands): every array becomes max(have, 1024) doubled until it holds the request; the first
    call asks for (1024, 4096, 4096, 4096) and is not counted; the state table follows the states, so rehashes == grow_states.
    ph_check: need = K > cands or hi + K > states or n_elts + K > elts or n_arcs + K > arcs (slots and ltab: module docstring).
    Host loop: L == 0 ends; a pending need reserves (hi + K + 1, n_elts + K, n_arcs + K, K) with K >= 1; the narrow kernel
    is launched when the path is narrow, or auto and L <= 256, with limits (256, 8192) in auto and none in narrow; inside,
    per level and in this order: L == 0 -> exit 4, L > limit -> exit 1, levels of this launch >= budget -> exit 2, need ->
    exit 3, K > limit -> exit 1, else the level runs.  After exit 1 in auto, and always in wide, ONE level runs device-wide:
    count and check (need -> back to the top), then the resolve rounds two at a time.
    rounds_max: every round makes the lowest unresolved candidate of each hash a new state and resolves those that
    approx-match it; a candidate that is still unresolved matches no leader so far.  A hash (= a state-id sequence) whose
    candidates create m new states is therefore settled by round m and not before; the host reads `rem` after rounds 2, 4,
    ... and stops at the first r = 2 j with r >= m.  It always runs the first pair, so a wide level ends with
    r = 2 * max(1, ceil(m / 2)), m = the largest such count of the level (0: every candidate found an older state).
    trace (a list): receives, per completed level, (regime, grow_states when the level ran)."""
    s = dict.fromkeys(COUNTERS, 0)
    cap = [0, 0, 0, 0]

    def reserve(want, first=False):
        for k, w in enumerate(want):
            n = max(cap[k], 1024)
            while n < w:
                n *= 2
            if n > cap[k]:
                if not first:
                    s[GROW[k]] += 1
                    s["rehashes"] += k == 0
                cap[k] = n

    for a, b in zip(figs, figs[1:]):
        assert a[2] == b[0], "a level holds the states the level before it created"
    assert figs[0][0] == 1 and figs[-1][2] == 0
    reserve(FIRST_RESERVE, first=True)
    i, hi, n_elts, n_arcs = 0, 1, 1, 0
    need_k = None

    def fig(k):
        return figs[k] if k < len(figs) else (0, 0, 0, 0, 0, 0)

    def short(K):
        return K > cap[3] or hi + K > cap[0] or n_elts + K > cap[1] or n_arcs + K > cap[2]

    def run(regime):
        nonlocal i, hi, n_elts, n_arcs
        _, _, new, nel, valid, m = fig(i)
        hi, n_elts, n_arcs, i = hi + new, n_elts + nel, n_arcs + valid, i + 1
        s["levels"] += 1
        if regime == "wide":
            s["wide_levels"] += 1
            s["rounds_max"] = max(s["rounds_max"], 2 * max(1, -(-m // 2)))
        if trace is not None:
            trace.append((regime, s["grow_states"]))

    for _ in range(4 * len(figs) + 64):
        L = fig(i)[0]
        if L == 0:
            break
        if need_k is not None:
            K = max(need_k, 1)
            reserve((hi + K + 1, n_elts + K, n_arcs + K, K))
            need_k = None
        if path == "narrow" or (path == "auto" and L <= NARROW_STATES):
            max_l, max_k = (NARROW_STATES, NARROW_CANDS) if path == "auto" else (1 << 32, 1 << 32)
            s["narrow_launches"] += 1
            it = 0
            while True:
                L, K = fig(i)[:2]
                if L == 0:
                    code = 4
                elif L > max_l:
                    code = 1
                elif it >= budget:
                    code = 2
                elif short(K):
                    code, need_k = 3, K
                elif K > max_k:
                    code = 1
                else:
                    run("narrow")
                    it += 1
                    continue
                break
            if code == 1:
                s["exit_wide_states" if fig(i)[0] > NARROW_STATES else "exit_wide_cands"] += 1
            s["exit_budget"] += code == 2
            s["exit_need"] += code == 3
            s["exit_done"] += code == 4
            if not (code == 1 and path == "auto"):
                continue
        K = fig(i)[1]
        if short(K):
            need_k = K
            s["wide_need"] += 1
            continue
        run("wide")
    else:
        raise AssertionError("the host loop did not end")
    for k in range(4):
        s[CAP[k]] = cap[k]
    return s


# ---------------------------------------------------------------- inputs
CAP_PAIRS = (("cap_states", 0), ("cap_states_wide", 0), ("cap_elts", 1), ("cap_arcs", 2), ("cap_cands", 3))


def same(got, exp, what):
    assert_flat_identical(got, exp, what, check_props=True)


# ================================================================ no GPU
def test_new_symbol_declared_exported_and_bound(wfst_lib):
    import rustfst_amd
    helpers.check_counter_getter(wfst_lib, "wfst_ctx_get_determinize_stats", COUNTERS, rustfst_amd.Context.determinize_stats)


def test_null_ctx_is_ko(wfst_lib):
    helpers.null_ctx_is_ko(wfst_lib, "wfst_ctx_get_determinize_stats", len(COUNTERS))


def _stats(**kw):
    s = dict.fromkeys(COUNTERS, 0)
    s.update(dict(zip(CAP, FIRST_RESERVE)))
    s.update(kw)
    return s


def test_restatement_against_closed_forms():
    # a plain chain of 300 states: one narrow launch that ends with nothing left; in wide 300 levels of two rounds
    chain = layered(chain_spec(300))[1]
    assert predict(chain, "auto") == predict(chain, "narrow") == _stats(levels=300, narrow_launches=1, exit_done=1)
    assert predict(chain, "wide") == _stats(levels=300, wide_levels=300, rounds_max=2)
    # budget b: a launch runs b levels and ends with exit 2 while states are left; `nothing left` is looked at first, so
    # the launch that completes level 300 ends with exit 4: ceil(300 / b) launches, all but the last by budget
    for b, launches in ((1, 300), (7, 43), (64, 5), (299, 2), (300, 1)):
        assert predict(chain, "narrow", b) == _stats(levels=300, narrow_launches=launches, exit_budget=launches - 1, exit_done=1)
    # one fan level, 1 -> 300 states without arcs: the launch completes level 0 and stops at level 1 (300 > 256), which runs
    # device-wide without candidates (two rounds); then nothing is left, and no narrow launch sees that
    fan = [(1, 300, 300, 300, 300, 1), (300, 0, 0, 0, 0, 0)]
    assert predict(fan, "auto") == _stats(levels=2, wide_levels=1, narrow_launches=1, exit_wide_states=1, rounds_max=2)
    assert predict(fan, "narrow") == _stats(levels=2, narrow_launches=1, exit_done=1)
    assert predict(fan, "wide") == _stats(levels=2, wide_levels=2, rounds_max=2)
    # 1 -> 256: nothing leaves the narrow kernel
    fan = [(1, 256, 256, 256, 256, 1), (256, 0, 0, 0, 0, 0)]
    assert predict(fan, "auto") == _stats(levels=2, narrow_launches=1, exit_done=1)
    # one growth: a chain of 1100 states.  Level 1023 has hi = 1024, K = 1: 1025 > 1024 states; the request is (1026, 1025,
    # 1024, 1): the states double, the rest stays
    chain = layered(chain_spec(1100))[1]
    grown = dict(levels=1100, grow_states=1, rehashes=1, cap_states=2048)
    assert predict(chain, "narrow") == _stats(narrow_launches=2, exit_need=1, exit_done=1, **grown)
    assert predict(chain, "wide") == _stats(wide_levels=1100, wide_need=1, rounds_max=2, **grown)
    # rounds of a wide level by the most new states m that share a state-id sequence
    for m, r in ((0, 2), (1, 2), (2, 2), (3, 4), (4, 4), (5, 6)):
        assert predict([(1, 9, 9, 18, 9, m), (9, 0, 0, 0, 0, 0)], "wide")["rounds_max"] == r
    # a level of at most 256 states and more than 8192 candidates in auto: need first (K > 4096 candidates), then the
    # relaunch ends with exit 1 and the level runs device-wide
    wide_k = [(1, 9000, 1, 1, 9000, 1), (1, 0, 0, 0, 0, 0)]
    assert predict(wide_k, "auto") == _stats(levels=2, wide_levels=1, narrow_launches=3, exit_need=1, exit_wide_cands=1,
                                             exit_done=1, grow_states=1, grow_elts=1, grow_arcs=1, grow_cands=1, rehashes=1,
                                             cap_states=16384, cap_elts=16384, cap_arcs=16384, cap_cands=16384, rounds_max=2)


SMALL = sorted(set(LAYERED) | set(OTHER))


def test_layered_inputs_have_the_figures_they_are_built_for():
    for name in sorted(LAYERED):
        assert analysis(name)["figs"] == case(name)[1], name
    flat, figs = fan_then_chain(140, 70)  # the generator of budget_real at a size the restatement can walk
    assert det_levels(flat)["figs"] == figs


def test_every_input_lands_on_its_limit():
    p = {name: {path: predict(case(name)[1], path) for path in PATHS} for name in SMALL + ["budget_real"]}
    # regime switch by states: the level of 257 leaves the narrow kernel once, and the levels after it run narrow again
    a, b = p["states_256"]["auto"], p["states_257"]["auto"]
    assert (a["exit_wide_states"], a["wide_levels"], a["narrow_launches"], a["exit_done"]) == (0, 0, 1, 1)
    assert (b["exit_wide_states"], b["wide_levels"], b["narrow_launches"], b["exit_done"]) == (1, 1, 2, 1)
    assert a["levels"] == b["levels"] == 5 and a["exit_wide_cands"] == b["exit_wide_cands"] == 0
    trace = []
    predict(case("states_257")[1], "auto", trace=trace)
    assert [r for r, _ in trace] == ["narrow", "wide", "narrow", "narrow", "narrow"]
    # ... and the host, which chooses for the level after a wide one, sends 256 states back to the narrow kernel and 257 not
    for name, regimes in (("after_wide_256", ["narrow", "wide"] + ["narrow"] * 4), ("after_wide_257", ["narrow", "wide", "wide"] + ["narrow"] * 3)):
        trace = []
        st = predict(case(name)[1], "auto", trace=trace)
        assert [r for r, _ in trace] == regimes and (st["exit_wide_states"], st["narrow_launches"], st["exit_done"]) == (1, 2, 1)
        assert case(name)[1][2][0] == (256 if name == "after_wide_256" else 257)
    # regime switch by candidates
    assert [f[:2] for f in case("cands_8192")[1][:2]] == [(1, 64), (64, 8192)]
    assert [f[:2] for f in case("cands_8193")[1][:2]] == [(1, 64), (64, 8193)]
    a, b = p["cands_8192"]["auto"], p["cands_8193"]["auto"]
    assert (a["exit_wide_cands"], a["wide_levels"], a["exit_wide_states"]) == (0, 0, 0)
    assert (b["exit_wide_cands"], b["wide_levels"], b["exit_wide_states"]) == (1, 1, 0)
    assert a["exit_need"] == b["exit_need"] == 1 and a["cap_cands"] == 8192 and b["cap_cands"] == 16384
    # capacities: the twin differs by one growth of exactly that array, found by the narrow kernel or by a wide check
    for stem, k in CAP_PAIRS:
        for path in PATHS:
            a, b = p[stem + "_fit"][path], p[stem + "_over"][path]
            diff = {c for c in COUNTERS if a[c] != b[c]}
            want = {GROW[k], CAP[k]} | ({"rehashes"} if k == 0 else set())
            want |= {"wide_need"} if path == "wide" or (stem == "cap_states_wide" and path == "auto") else {"exit_need", "narrow_launches"}
            assert diff == want, (stem, path, diff)
            assert b[GROW[k]] == a[GROW[k]] + 1 and b[CAP[k]] == 2 * a[CAP[k]], (stem, path)
            assert b["exit_need"] + b["wide_need"] == a["exit_need"] + a["wide_need"] + 1
    assert p["cap_states_fit"]["auto"]["grow_states"] == 0 and p["cap_states_wide_fit"]["auto"]["grow_states"] == 0
    assert p["cap_states_wide_over"]["auto"]["exit_wide_states"] == 1
    # level budget at its real value: the fan takes the capacities past the chain, so the launch ends by budget alone
    b = p["budget_real"]["auto"]
    assert b["exit_budget"] == 1 and b["levels"] == BUDGET_CHAIN + 2 and b["wide_levels"] == 2
    assert b["cap_states"] >= 1 + BUDGET_FAN + BUDGET_CHAIN and b["grow_states"] == 2
    # resolve rounds
    assert [p[n]["wide"]["rounds_max"] for n in ("rounds_3_4", "rounds_5_2", "rounds_1_2")] == [4, 6, 2]
    assert sorted(f[5] for f in case("rounds_3_4")[1])[-1] == 4 and case("rounds_3_4")[1][1][2] == 7
    for n in ("collision_8_40", "collision_16_100"):
        assert p[n]["wide"]["rounds_max"] >= 4 and p[n]["narrow"]["rounds_max"] == 0, n
    assert case("collision_16_100")[1][1][:2] == (16, 3200)
    # the LDS scratch limit of the batch kernel
    assert max(f[1] for f in case("lds_496")[1]) == 496 and max(f[1] for f in case("lds_497")[1]) == 497
    assert [f[1] > 496 for f in case("lds_alternating")[1]] == [False, True, False, True, False, False, True, False]


def _reaches(name, path):
    """(level, regime and growths when it ran, regime and growths when the reached state was created) of every reach"""
    trace = []
    predict(case(name)[1], path, trace=trace)
    out = []
    for i, levels in enumerate(analysis(name)["reach"]):
        for j in levels:
            out.append((i, trace[i], trace[j - 1] if j else ("seed", 0)))
    return out


def test_reuse_inputs_cross_the_boundary_they_are_built_for():
    r = _reaches("reuse_regimes", "auto")
    assert any(a[0] == "wide" and b[0] == "narrow" for _, a, b in r), "a wide level reaching a state a narrow level created"
    assert any(a[0] == "narrow" and b[0] == "wide" for _, a, b in r), "a narrow level reaching a state a wide level created"
    assert any(a[0] == "wide" and b[0] == "seed" for _, a, b in r)
    for name, path, regime in (("reuse_growth", "auto", "wide"), ("reuse_growth", "narrow", "narrow"),
                               ("reuse_growth", "wide", "wide"), ("reuse_growth_narrow", "auto", "narrow")):
        r = _reaches(name, path)
        assert predict(case(name)[1], path)["grow_states"] >= 1
        # the level whose own check grew the states, and a level after it, reach states created before the re-hash
        assert any(i == 1 and a == (regime, 1) and b[1] == 0 for i, a, b in r), (name, path)
        assert any(i == 2 and a[1] == 1 and b[1] == 0 for i, a, b in r), (name, path)


def test_growth_input_reaches_the_second_entry_of_a_chain():
    """what Run::reserve keeps of hnext ([0, hi)) is needed only when a chain of two or more states, the newer of them in
    the level whose check grows the arrays, is walked past its head after the growth"""
    an = analysis("chain_across_growth")
    ab = [k for k, t in enumerate(an["tuples"]) if tuple(q for q, _ in t) == (4, 5)]
    assert [int(round(float(an["tuples"][k][1][1]) / KDELTA)) for k in ab] == [3, 5]  # O, N: the candidates of 2 and 3 joined O
    O, N = ab
    level = an["level_of"][N]
    assert an["level_of"][O] == level - 1
    off, arcs = an["fst"]["offsets"], an["fst"]["arcs"]
    for path, regimes in (("auto", ("narrow", "wide")), ("narrow", ("narrow", "narrow")), ("wide", ("wide", "wide"))):
        trace = []
        predict(an["figs"], path, trace=trace)
        # the states grow for the first time while N's level waits: the chain of (A, B) is N -> O, and hnext[N] lies in [lo, hi)
        assert trace[level - 1][1] == 0 and trace[level][1] == 1, path
        for lv, regime in zip((level, level + 1), regimes):  # the level itself and the one after it walk on to O
            src = [q for q in range(an["fst"]["n_states"]) if an["level_of"][q] == lv]
            dests = [int(d) for q in src for d in arcs["nextstate"][off[q]:off[q + 1]]]
            assert O in dests and N not in dests and trace[lv][0] == regime, (path, lv)
            assert level - 1 in an["reach"][lv]


def test_lowest_id_inputs_match_two_older_states():
    for name in ("lowest_id_levels", "lowest_id_same_level"):
        an = analysis(name)
        ab = [k for k, t in enumerate(an["tuples"]) if tuple(q for q, _ in t) == (4, 5)]
        res = [int(round(float(an["tuples"][k][1][1]) / KDELTA)) for k in ab]
        assert res == [3, 5] and ab[0] < ab[1], name  # no state for the 4 KDELTA candidate
        older, newer = an["tuples"][ab[0]], an["tuples"][ab[1]]
        mid = ((4, F32(0.0)), (5, F32(4 * KDELTA)))
        for t in (older, newer):
            assert all(model.approx_eq(w, v) for (_, w), (_, v) in zip(mid, t))
        arcs = an["fst"]["arcs"]
        assert int((arcs["nextstate"] == ab[0]).sum()) == 2 and int((arcs["nextstate"] == ab[1]).sum()) == 1, name
        levels = [an["level_of"][k] for k in ab]
        assert (levels[0] == levels[1]) == (name == "lowest_id_same_level")
        assert any(levels[0] in r for r in an["reach"]), name  # found among the states of earlier levels


def test_sort_input_has_the_widths_it_is_built_for():
    flat, figs = case("sort_widths")
    an = analysis("sort_widths")
    deg = np.diff(flat["offsets"].astype(np.int64))
    raw = [int(sum(deg[q] for q, _ in t)) for t, lv in zip(an["tuples"], an["level_of"]) if lv == 1]
    assert raw == list(SORT_WIDTHS) and figs[1][1] == sum(SORT_WIDTHS) and figs[0][1] == 2 * len(SORT_WIDTHS)
    assert all(len(t) == 2 for t, lv in zip(an["tuples"], an["level_of"]) if lv == 1)
    arcs = flat["arcs"]
    assert np.isinf(arcs["weight"]).any() and (arcs["ilabel"] >= 1 << 31).any()
    assert (np.signbit(arcs["weight"]) & (arcs["weight"] == 0)).any()
    # keys arrive out of order, and some (label, dest) arrive twice in a state
    dup = 0
    for t, lv in zip(an["tuples"], an["level_of"]):
        if lv == 1:
            keys = [(int(a["ilabel"]), int(a["nextstate"])) for q, _ in t for a in arcs[flat["offsets"][q]:flat["offsets"][q + 1]]]
            dup += len(keys) - len(set(keys))
            assert len(keys) < 3 or keys != sorted(keys)
    assert dup >= 20


def test_sort_ties_cannot_be_observed():
    """module docstring: no raw candidate is -0.0 (det_levels asserts it for every candidate it builds), so candidates of
    equal key that compare equal have equal bits, and reversing every tie leaves the result as it is"""
    for name in ("sort_widths", "collision_8_40", "lowest_id_levels"):
        flat = case(name)[0]
        same(det_levels(flat, reverse_ties=True)["fst"], analysis(name)["fst"], name)
    # the one way to -0.0: both terms -0.0, and quantize never returns it
    assert np.signbit(F32(-0.0) + F32(-0.0)) and not np.signbit(F32(0.0) + F32(-0.0))
    for v in (F32(0.0), F32(-0.0), F32(KDELTA / 4), F32(3 * KDELTA)):
        q = model.quantize(v, KDELTA)
        assert not (q == 0 and np.signbit(q))


def test_restatement_matches_the_oracle(oracle):
    for name in SMALL:
        flat = case(name)[0]
        exp = to_oracle(oracle, flat).determinize_fsa(KDELTA).to_flat()
        exp["props"] = model.determinize_props(flat["props"], True)
        same(analysis(name)["fst"], exp, name)


# ================================================================ GPU
@functools.lru_cache(maxsize=None)
def _expected(oracle, name):
    flat = case(name)[0]
    exp = to_oracle(oracle, flat).determinize_fsa(KDELTA).to_flat()
    exp["props"] = model.determinize_props(flat["props"], True)
    return exp


def _check(ctx, oracle, monkeypatch, name, paths=PATHS, budget=None):
    flat, figs = case(name)
    dev = to_device(flat, ctx)
    for path in paths:
        monkeypatch.setenv("WFST_DETERMINIZE_PATH", path)
        got = dev.determinize().to_flat()
        st = ctx.determinize_stats()
        same(got, _expected(oracle, name), f"{name} {path}")
        want = predict(figs, path, budget or BUDGET)
        assert st == want, f"{name} {path}: " + ", ".join(f"{k} {st[k]} != {want[k]}" for k in COUNTERS if st[k] != want[k])
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in SMALL if n not in ("chain_300", "diamond_300")])
def test_every_limit_on_the_device(gpu_ctx, oracle, monkeypatch, name):
    _check(gpu_ctx, oracle, monkeypatch, name)


@pytest.mark.gpu
def test_counters_are_those_of_the_last_call(gpu_ctx, oracle, monkeypatch):
    import rustfst_amd
    monkeypatch.setenv("WFST_DETERMINIZE_PATH", "auto")
    for name in ("states_257", "cap_arcs_over", "states_256"):
        flat, figs = case(name)
        to_device(flat, gpu_ctx).determinize()
        assert gpu_ctx.determinize_stats() == predict(figs, "auto"), name
    flat, figs = case("states_257")
    out, _ = rustfst_amd.determinize_with_distance(to_device(flat, gpu_ctx), np.zeros(flat["n_states"], np.float32))
    same(out.to_flat(), _expected(oracle, "states_257"), "with distance")
    assert gpu_ctx.determinize_stats() == predict(figs, "auto")
    empty = dict(n_states=0, start=None, offsets=np.zeros(1, np.uint32), arcs=np.zeros(0, TR_DTYPE),
                 finals=np.zeros(0, np.float32), props=ACCEPTOR)
    to_device(empty, gpu_ctx).determinize()
    assert gpu_ctx.determinize_stats() == dict.fromkeys(COUNTERS, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("budget", (1, 7, 64))
def test_level_budget_knob(gpu_ctx, oracle, monkeypatch, budget):
    monkeypatch.setenv("WFST_DETERMINIZE_LEVEL_BUDGET", str(budget))
    for name in ("chain_300", "diamond_300"):
        st = _check(gpu_ctx, oracle, monkeypatch, name, ("auto", "narrow"), budget)
        assert st["exit_budget"] == -(-len(case(name)[1]) // budget) - 1 and st["exit_done"] == 1


@pytest.mark.gpu
def test_level_budget_knob_ignores_other_values(gpu_ctx, oracle, monkeypatch):
    for value in ("0", "-3", "65536", "70000", "x"):
        monkeypatch.setenv("WFST_DETERMINIZE_LEVEL_BUDGET", value)
        assert _check(gpu_ctx, oracle, monkeypatch, "chain_300", ("auto",))["exit_budget"] == 0


@pytest.mark.gpu
def test_level_budget_at_its_real_value(gpu_ctx, oracle, monkeypatch):
    """65 540 chain levels behind a fan of 140 000 (which takes the capacities to 524 288, so no growth ends the launch
    early): the first chain launch ends by budget after 65 536 levels.  Measured: profiles/determinize_timing.md."""
    flat, figs = case("budget_real")
    monkeypatch.setenv("WFST_DETERMINIZE_PATH", "auto")
    dev = to_device(flat, gpu_ctx)
    t0 = time.perf_counter()
    out = dev.determinize()
    print(f"budget_real: determinize of {flat['n_states']} states in {time.perf_counter() - t0:.3f} s")
    st = gpu_ctx.determinize_stats()
    same(out.to_flat(), _expected(oracle, "budget_real"), "budget_real auto")
    assert st == predict(figs, "auto")
    assert st["exit_budget"] == 1 and st["levels"] == BUDGET_CHAIN + 2
