"""Look-ahead composition (compose_lookahead.hip) at every limit.  The single-wave kernel hands a composition to the wide driver
when it grows past a state count or a level width, or when its arena is full; it processes items and interns destinations 64
at a time; lookahead_fst finds what is reachable in one of two ways.  Every route returns the same FST: a wrong guard changes
no result, an off-by-one inside a branch does, but only on an input that sits exactly on the limit.  Every generator of
lookahead_cases.py places an input ON a limit and its twin one step beyond; only the counters of
wfst_ctx_get_lookahead_stats show which route answered.

Without a GPU: the symbol, where every generator lands (from the oracle's look-ahead composition: its ids are first-touch BFS
order, so its levels are contiguous id ranges; its tuple list gives the pair of states and the filter state behind every id),
and a Python restatement of the routing (lookahead_cases.Handle) that predicts the counters of every call made below.  On the
device: every result against the oracle bit for bit, property word included, and the counters against the prediction —
by default, under WFST_LOOKAHEAD_PATH=wave and under WFST_LOOKAHEAD_PATH=wide, the three results identical.

handed_over_states / handed_over_width are told apart the way the getter's contract says: by the state count the wave
reports against the state limit in force.  A star of 4351 leaves (4352 states = S, no overflow) therefore counts as handed
over by STATES, although it is its first level's width that makes the kernel stop; so does every input beyond both limits
whose wide level comes after the state limit is passed."""
import os
import re

import numpy as np
import pytest

import helpers
from helpers import ROOT, assert_flat_identical, empty_flat, to_device
import lookahead_cases as lc
from lookahead_cases import (CAP_A, CAP_H, CAP_S, COUNTERS, NO_LABEL, PATHS, SWITCH_STATES, SWITCH_STATES_ONE, SWITCH_WIDTH,
                             SWITCH_WIDTH_ONE, WAVE, ZERO, analyse)

NAME = "wfst_ctx_get_lookahead_stats"
START_LESS = empty_flat()


def counters(**kw):
    assert set(kw) <= set(COUNTERS)
    return dict(ZERO, **kw)


# ================================================================ the cases: name -> (first operand, calls); a call is a list of
# second operands (one: wfst_compose_lookahead, more: wfst_compose_lookahead_batch)
def _hand_over_one():
    chain2, both1 = lc.loop2(lc.CHAIN_LABELS), lc.wide_chain1(60, 600)
    c = {"chain:%d" % n: (lc.chain1(n), [[chain2]]) for n in (SWITCH_STATES_ONE, SWITCH_STATES_ONE + 1)}
    c.update({"star:%d" % w: (lc.star1(w), [[lc.loop2(lc.star_labels(w))]]) for w in (SWITCH_WIDTH_ONE, SWITCH_WIDTH_ONE + 1)})
    c["beyond_both"] = (both1, [[lc.loop2(lc.star_labels(60)[:-1] + list(lc.CHAIN_LABELS))]])
    return c


def _hand_over_batch():
    chain2, small_chain2 = lc.loop2(lc.CHAIN_LABELS), lc.loop2([1])
    c = {"chain:%d" % n: (lc.chain1(n), [[chain2, small_chain2]]) for n in (SWITCH_STATES, SWITCH_STATES + 1)}
    c.update({"star:%d" % w: (lc.star1(w), [[lc.loop2([100]), lc.loop2(lc.star_labels(w))]]) for w in (SWITCH_WIDTH, SWITCH_WIDTH + 1)})
    c["chain:513_in_a_batch_then_alone"] = (lc.chain1(SWITCH_STATES_ONE + 1), [[chain2, small_chain2], [chain2]])
    c["chain:513_beside_a_start_less_item"] = (lc.chain1(SWITCH_STATES_ONE + 1), [[chain2, START_LESS]])
    return c


def _arenas():
    par2 = lc.loop2(lc.parallel_labels(513))
    links = CAP_A // 512
    c = {"arcs:%d" % CAP_A: (lc.parallel1(links), [[par2]]), "arcs:%d" % (CAP_A + 1): (lc.parallel1(links, one_more=True), [[par2]])}
    for leaves in (CAP_S - 1, CAP_S):
        f2 = lc.loop2(lc.star_labels(leaves)[:-1])
        c["states:%d" % (leaves + 1)] = (lc.star1(leaves, tail=False), [[f2], [f2, lc.loop2([100], final=lc.INF)]])
    return c


HAND_OVER_ONE, HAND_OVER_BATCH, ARENAS = _hand_over_one(), _hand_over_batch(), _arenas()
ITEM_CASES = [(n, side, multi) for n in lc.ITEM_ARCS for side in lc.ITEM_SIDES for multi in (None, WAVE - 1, WAVE) if multi is None or multi <= n]
_ITEMS = {}


def items_case(n, side, multi):
    if (n, side, multi) not in _ITEMS:
        _ITEMS[n, side, multi] = lc.items_pair(n, side, multi)
    return _ITEMS[n, side, multi]


INTERN = {"%s:%d" % (fold, n): lc.intern_pair(n, fold) for n in lc.INTERN_ARCS for fold in lc.INTERN_FOLDS}
TWINS = {kind: lc.twin_pair(kind) for kind in lc.TWINS}
BRANCH2 = {name: lc.branch2(labels, final) for name, (labels, final) in lc.BRANCH_SECONDS.items()}
QUANT2 = {name: lc.quant2(w) for name, w in lc.quant_weights().items()}
QUANT2["tie_of_zeros"] = lc.quant2(-0.0, 0.0)
HUB2 = dict(small=lc.hub_chain2(7), chain=lc.hub_chain2(SWITCH_STATES + 1), star_one=lc.hub_star2(SWITCH_WIDTH_ONE + 1),
            star_one_padded=lc.hub_star2(SWITCH_WIDTH_ONE + 1, 460), star=lc.hub_star2(SWITCH_WIDTH + 1), parallel=lc.hub_parallel2(),
            start_less=START_LESS)
MIXED = ("small", "chain", "star", "parallel", "start_less", "small")


def widths(an):
    return [lv[3] for lv in an["levels"]]


def predict_calls(oracle, f1, calls, paths=PATHS):
    """{path: [prediction of every call]} for one handle that serves the calls under each path in turn, as the device tests do"""
    h = lc.Handle(f1)
    return {path: [h.predict([analyse(oracle, f1, f2) for f2 in call], path) for call in calls] for path in paths}


# ================================================================ no GPU
def test_getter_declared_exported_and_bound(wfst_lib):
    import rustfst_amd
    from rustfst_amd import _lib
    header = helpers.check_counter_getter(wfst_lib, NAME, COUNTERS, rustfst_amd.Context.lookahead_stats)
    assert _lib.COUNTERS["lookahead"] == (NAME, COUNTERS)
    text = header[header.index("which route answered the compositions of the last wfst_compose_lookahead"):header.index("wfst_status " + NAME)]
    text = " ".join(text.replace("\n *", " ").split())
    for limit in ("S = 2 * 2048 + 256 = 4352", "A = 4 * S = 17408", "H = pow2(2 * S + 128) = 16384", "passes 2048 states",
                  "more than 256 states", "the limits are 512 and 48", "S = 16 * 2048", "within a factor of two"):
        assert limit in text, limit
    for doc in ("DESIGN.md", "INTEGRATION.md", "README.md"):
        with open(os.path.join(ROOT, doc)) as f:
            assert NAME in f.read(), doc


def test_null_ctx_is_ko(wfst_lib):
    helpers.null_ctx_is_ko(wfst_lib, NAME, len(COUNTERS))


def test_constants_are_the_kernels():
    with open(os.path.join(ROOT, "rustfst_amd", "csrc", "compose_lookahead.hip")) as f:
        src = f.read()
    for name, value in (("WIDE_SWITCH_STATES", SWITCH_STATES), ("WIDE_SWITCH_WIDTH", SWITCH_WIDTH),
                        ("WIDE_SWITCH_STATES_ONE", SWITCH_STATES_ONE), ("WIDE_SWITCH_WIDTH_ONE", SWITCH_WIDTH_ONE)):
        m = re.search(r"constexpr uint32_t " + name + r" = (\d+);", src)
        assert m and int(m.group(1)) == value, name
    assert "const uint64_t est_s = 2ull * WIDE_SWITCH_STATES + 256;" in src
    assert src.count("const LaCaps caps{(uint32_t)est_s, (uint32_t)(4 * est_s), next_pow2(2 * est_s + 128)};") == 2
    assert "uint64_t est_s = 16ull * WIDE_SWITCH_STATES;" in src and "est_s *= 4;" in src
    assert (CAP_S, CAP_A, CAP_H, lc.REGROW_S) == (4352, 17408, 16384, 32768)
    with open(os.path.join(ROOT, "rustfst_amd", "csrc", "compose_wide.h")) as f:
        wide = f.read()
    assert "est_s = std::max<uint64_t>(est_s, 1ull << 18);" in wide and "constexpr uint32_t CUR_SHARDS = 64;" in wide
    assert "batch_cap = 4;" in wide


def test_hand_over_generators_sit_on_their_limits(oracle):
    """one composition: 512 states stay, 513 leave; a level of 48 new states stays, 49 leaves"""
    lone = dict(items=1, one_limits=1)
    for n, want in ((512, counters(wave_answered=1, **lone)), (513, counters(handed_over_states=1, wide_items=1, **lone))):
        f1, calls = HAND_OVER_ONE["chain:%d" % n]
        an = analyse(oracle, f1, calls[0][0])
        assert an["n_states"] == n and set(widths(an)) == {0, 1} and len(an["levels"]) == n
        assert (an["r1"]["arcs"]["olabel"] == 0).sum() == (n - 1) // 2  # every second arc is x:eps
        assert (an["tuples"][:, 4] != NO_LABEL).sum() > n // 4  # every x:eps arc sees ONE arc ahead: its label is pushed
        p = predict_calls(oracle, f1, calls)
        assert p[None] == [want] and p["wave"] == [counters(items=1, wave_answered=1)]
        assert p["wide"] == [counters(items=1, wide_items=1)]
    for w, want in ((48, counters(wave_answered=1, **lone)), (49, counters(handed_over_width=1, wide_items=1, **lone))):
        f1, calls = HAND_OVER_ONE["star:%d" % w]
        an = analyse(oracle, f1, calls[0][0])
        assert widths(an) == [w, 1, 1, 0] and an["n_states"] == w + 3 <= SWITCH_STATES_ONE
        assert predict_calls(oracle, f1, calls)[None] == [want]
    f1, calls = HAND_OVER_ONE["beyond_both"]
    an = analyse(oracle, f1, calls[0][0])
    assert an["n_states"] > SWITCH_STATES_ONE and widths(an)[0] == 60 > SWITCH_WIDTH_ONE and set(widths(an)[1:]) == {0, 1}
    # the wide level is the first: the wave stops with 61 states, below the state limit
    assert predict_calls(oracle, f1, calls)[None] == [counters(handed_over_width=1, wide_items=1, **lone)]


def test_batch_generators_sit_on_their_limits(oracle):
    """two compositions in a call: the limits are 2048 states and 256 new states in a level; a start-less item does not count"""
    for n, big in ((2048, counters(items=2, wave_answered=2)), (2049, counters(items=2, wave_answered=1, handed_over_states=1, wide_items=1))):
        f1, calls = HAND_OVER_BATCH["chain:%d" % n]
        an, small = analyse(oracle, f1, calls[0][0]), analyse(oracle, f1, calls[0][1])
        assert an["n_states"] == n and set(widths(an)) == {0, 1} and 1 <= small["n_states"] < 8
        p = predict_calls(oracle, f1, calls)
        assert p[None] == [big] and p["wave"] == [counters(items=2, wave_answered=2)] and p["wide"] == [counters(items=2, wide_items=2)]
    for w, big in ((256, counters(items=2, wave_answered=2)), (257, counters(items=2, wave_answered=1, handed_over_width=1, wide_items=1))):
        f1, calls = HAND_OVER_BATCH["star:%d" % w]
        an = analyse(oracle, f1, calls[0][1])
        assert widths(an) == [w, 1, 1, 0] and an["n_states"] <= SWITCH_STATES
        assert predict_calls(oracle, f1, calls)[None] == [big]
    f1, calls = HAND_OVER_BATCH["chain:513_in_a_batch_then_alone"]
    assert predict_calls(oracle, f1, calls)[None] == [counters(items=2, wave_answered=2),
                                                      counters(items=1, handed_over_states=1, wide_items=1, one_limits=1)]
    f1, calls = HAND_OVER_BATCH["chain:513_beside_a_start_less_item"]  # m = 1: the limits of ONE composition
    assert predict_calls(oracle, f1, calls)[None] == [counters(items=2, items_no_start=1, handed_over_states=1, wide_items=1, one_limits=1)]


def test_arena_generators_fill_the_arena_exactly(oracle):
    lone = dict(items=1, one_limits=1)
    for arcs, want, wave in ((CAP_A, counters(wave_answered=1, **lone), counters(items=1, wave_answered=1)),
                             (CAP_A + 1, counters(overflow_arcs=1, wide_items=1, wide_grows=1, **lone),
                              counters(items=1, overflow_arcs=1, wave_regrows=1, wave_answered=1))):
        f1, calls = ARENAS["arcs:%d" % arcs]
        an = analyse(oracle, f1, calls[0][0])
        assert an["n_arcs"] == arcs and an["n_states"] <= 36 and set(widths(an)) == {0, 1}  # neither switch limit interferes
        assert sorted({lv[2] for lv in an["levels"]} - {0}) == ([512] if arcs == CAP_A else [512, 513])
        assert int(an["items"].max()) == 513  # 512 arcs on either side: the first operand iterates, + the loop item
        p = predict_calls(oracle, f1, calls)
        assert p[None] == [want] and p["wave"] == [wave]
        # pinned to the wide driver: one state per level, so one slice of 2^20 / 64 arcs takes every arc, and grows once
        assert p["wide"] == [counters(items=1, wide_items=1, wide_grows=1)]
    for states in (CAP_S, CAP_S + 1):
        f1, calls = ARENAS["states:%d" % states]
        an = analyse(oracle, f1, calls[0][0])
        assert widths(an) == [states - 1, 0] and an["n_states"] == states and an["levels"][0][2] == states - 1 <= CAP_A
        assert (an["r1"]["arcs"]["olabel"] == 0).sum() == (states - 1) // 3
        p = predict_calls(oracle, f1, calls)
        if states == CAP_S:  # the level fits; 4352 states are more than either state limit
            assert p[None] == [counters(handed_over_states=1, wide_items=1, **lone),
                               counters(items=2, wave_answered=1, handed_over_states=1, wide_items=1)]
            assert p["wave"] == [counters(items=1, wave_answered=1), counters(items=2, wave_answered=2)]
        else:
            assert p[None] == [counters(overflow_states=1, wide_items=1, **lone),
                               counters(items=2, wave_answered=1, overflow_states=1, wide_items=1)]
            assert p["wave"] == [counters(items=1, overflow_states=1, wave_regrows=1, wave_answered=1),
                                 counters(items=2, overflow_states=1, wave_regrows=1, wave_answered=2)]


def test_item_generators_fill_their_chunks(oracle):
    """items = arcs of the iterated side + 1: 63 arcs fill one chunk, 64 start a second; which side iterates; every item emits at
    most one arc (positions from a ballot), or one item emits three (positions from a scan) in lane 63 / in lane 0 of the next
    chunk"""
    seen = set()
    for n, side, multi in ITEM_CASES:
        an = analyse(oracle, *items_case(n, side, multi))
        counts = lc.item_counts(an)
        assert int(an["items"][0]) == n + 1 == len(counts) and bool(an["first_iterates"][0]) == (side != "second")
        assert (int(an["n1"][0]) == int(an["n2"][0])) == (side == "tie")
        assert sum(counts) == int(an["degree"][0]) == an["levels"][0][2], (n, side, multi)
        assert (an["r1"]["arcs"]["olabel"][:int(an["n1"][0])] == 0).sum() >= 1
        many = [j for j, c in enumerate(counts) if c > 1]
        assert many == ([] if multi is None else [multi]) and max(counts) == (1 if multi is None else 3)
        seen.add(((n + 1 + WAVE - 1) // WAVE, None if multi is None else (multi // WAVE, multi % WAVE)))
    assert {(1, None), (2, None), (3, None), (1, (0, 63)), (2, (0, 63)), (2, (1, 0)), (3, (1, 0))} <= seen


def test_intern_generators_fill_their_chunks(oracle):
    for name, (f1, f2) in INTERN.items():
        fold, n = name.split(":")[0], int(name.split(":")[1])
        an = analyse(oracle, f1, f2)
        lo, hi, emitted, new = an["levels"][1]
        assert (lo, hi, emitted) == (1, 2, n) and an["levels"][0][2:] == (1, 1)
        assert an["tuples"][1].tolist() == [1, 0, 0, 0, NO_LABEL]  # the hub under a pushed weight of 0
        nx = an["flat"]["arcs"]["nextstate"][1:1 + n].tolist()
        if fold == "one":
            assert set(nx) == {2} and new == 1
        elif fold == "distinct":
            assert nx == list(range(2, 2 + n)) and new == n
        elif fold == "border":
            assert (nx[63] == nx[64] and new == n - 1 and len(set(nx)) == n - 1) if n > 64 else new == n
        else:
            back = [j for j in (5, 63, 64) if j < n]
            assert [j for j, x in enumerate(nx) if x == 1] == back and new == n - len(back) == len(set(nx)) - 1
    for kind, (f1, f2) in TWINS.items():
        an = analyse(oracle, f1, f2)
        level = next(lv for lv in an["levels"] if lv[2] >= 70)
        e0 = int(an["flat"]["offsets"][level[0]])
        dest = an["tuples"][an["flat"]["arcs"]["nextstate"][e0:e0 + WAVE]]  # the destinations of the level's first chunk
        pairs = [(a, b) for a in range(WAVE) for b in range(a + 1, WAVE)
                 if tuple(dest[a][:2]) == tuple(dest[b][:2]) and tuple(dest[a]) != tuple(dest[b])]
        assert len(pairs) == 1, kind
        a, b = dest[pairs[0][0]], dest[pairs[0][1]]
        differ = [i for i in (2, 3, 4) if a[i] != b[i]]
        assert differ == [dict(alt=2, weight=3, label=4)[kind]], (kind, a, b)


def test_lookahead_fst_takes_both_branches(oracle):
    import rustfst_amd
    f1 = lc.branch1()
    la = rustfst_amd.LookAhead.reachable_from_arrays(f1["n_states"], f1["offsets"], f1["arcs"], f1["finals"])
    intervals = la.data()["intervals"]
    k = lc.BRANCH_K
    assert [len(iv) for iv in intervals] == [1, 1, k, k, k + 1, 1]
    assert intervals[2] == [(2 * i + 1, 2 * i + 2) for i in range(k)]
    taken = {name: lc.branches_taken(analyse(oracle, f1, f2), intervals) for name, f2 in BRANCH2.items()}
    assert taken["n0"] == (4, 0) and taken["n2"] == (3, 2) and taken["n3"] == (1, 4) and taken["n4"] == (0, 5)
    # 2 n == K walks the intervals (n3 at A and B), 2 n < K scans the arcs (n2 at A, B and A2)
    tuples = {name: analyse(oracle, f1, f2)["tuples"] for name, f2 in BRANCH2.items()}
    pushed = lambda name: sorted(int(t[0]) for t in tuples[name] if t[4] != NO_LABEL)
    assert pushed("n1_prefix") == [1, 2, 4] and pushed("n1_other") == [1, 3]  # exactly one reachable arc: the prefix
    assert pushed("n1_final") == [1, 2]  # ... but not from A2, which also reaches the final label
    assert pushed("n2_same_label") == [] and analyse(oracle, f1, BRANCH2["n2_same_label"])["n_states"] == 5
    assert analyse(oracle, f1, BRANCH2["n2_unread"])["n_states"] == 1 and analyse(oracle, f1, BRANCH2["n0_final"])["n_states"] == 3


def test_quantization_generators(oracle):
    """the pushed weight of state 1 is quantize(w), which the restatement of semiring.rs:132-145 gives as well; the halves
    round up, their lower neighbours down"""
    weights = dict(lc.quant_weights(), tie_of_zeros=-0.0)
    for name, f2 in QUANT2.items():
        an = analyse(oracle, lc.quant1(), f2)
        assert an["n_states"] == 3 and an["tuples"][1].tolist()[:3] == [1, 0, 0] and an["tuples"][1][4] == NO_LABEL
        q = np.array([an["tuples"][1][3]], np.uint32).view(np.float32)[0]
        assert q == lc.quantize(weights[name]), (name, q)
    k = lc.KDELTA
    assert lc.quantize(3.5 * k) == 4 * k and lc.quantize(np.nextafter(np.float32(3.5 * k), np.float32(0))) == 3 * k
    assert lc.quantize(-4.5 * k) == -4 * k and lc.quantize(2.0 ** 20 + 0.5) == 2.0 ** 20 + 0.5


def test_hint_and_mixed_batch_predictions(oracle):
    f1 = lc.hub1()
    an = {name: analyse(oracle, f1, f2) for name, f2 in HUB2.items()}
    assert an["small"]["n_states"] == 7 and an["chain"]["n_states"] == SWITCH_STATES + 1 and set(widths(an["chain"])) == {0, 1}
    assert widths(an["star_one"]) == [SWITCH_WIDTH_ONE + 1, 1, 1, 0] == widths(an["star_one_padded"])
    assert widths(an["star"]) == [SWITCH_WIDTH + 1, 1, 1, 0]
    par = an["parallel"]
    assert par["n_arcs"] == 1 + 512 * lc.HUB_LINKS > CAP_A and set(widths(par)) == {0, 1}
    # the hint: the arcs of the wide result, + 1/4 + 65536, must pass the unhinted 4 * 8 * 4096
    assert par["n_arcs"] + par["n_arcs"] // 4 + 65536 > 4 * 8 * 4096
    n_par, n_pad, n_star = (len(HUB2[k]["arcs"]) for k in ("parallel", "star_one_padded", "star_one"))
    assert n_pad <= 2 * n_par + 16 and n_par <= 2 * n_pad + 16 and not n_pad <= 2 * n_star + 16
    h = lc.Handle(f1)
    lone = dict(items=1, one_limits=1, wide_items=1)
    assert h.predict([par]) == counters(overflow_arcs=1, wide_grows=1, **lone)
    assert h.predict([an["star_one_padded"]]) == counters(handed_over_width=1, wide_hinted=1, **lone)
    assert h.predict([an["star_one"]]) == counters(handed_over_width=1, **lone)
    mixed = [an[k] for k in MIXED]
    assert lc.Handle(f1).predict(mixed) == counters(items=6, items_no_start=1, wave_answered=2, handed_over_states=1,
                                                    handed_over_width=1, overflow_arcs=1, wide_items=3, wide_grows=1)


# ================================================================ on the device
def run_calls(ctx, oracle, monkeypatch, f1, calls, paths=PATHS):
    """One handle serves `calls` under every path in turn.  Every output equals the oracle's FST bit for bit, the counters of
    every call equal the prediction, and a call's outputs are identical under the three paths.  Returns {path: [counters]}."""
    import rustfst_amd
    la = rustfst_amd.LookAhead(to_device(f1, ctx))
    model = lc.Handle(f1)
    second = {}
    seen, flats = {}, {}
    for path in paths:
        if path is None:
            monkeypatch.delenv("WFST_LOOKAHEAD_PATH", raising=False)
        else:
            monkeypatch.setenv("WFST_LOOKAHEAD_PATH", path)
        seen[path] = []
        for ci, call in enumerate(calls):
            ans = [analyse(oracle, f1, f2) for f2 in call]
            want = model.predict(ans, path)
            for f2 in call:
                if id(f2) not in second:  # (a second operand that comes twice is the same handle twice)
                    second[id(f2)] = la.relabel(to_device(f2, ctx))
            d2 = [second[id(f2)] for f2 in call]
            outs = [la.compose(d2[0], ctx)] if len(call) == 1 else la.compose_batch(d2, ctx)
            got = ctx.lookahead_stats()
            assert len(outs) == len(call)
            out_flats = [o.to_flat() for o in outs]
            for i, (flat, an) in enumerate(zip(out_flats, ans)):
                assert_flat_identical(flat, an["flat"], f"call {ci} item {i} under {path}", check_props=True)
            assert got == want, f"call {ci} under {path}: " + ", ".join(f"{k} {got[k]} != {want[k]}" for k in COUNTERS if got[k] != want[k])
            seen[path].append(got)
            for i, flat in enumerate(out_flats):
                if (ci, i) in flats:
                    assert_flat_identical(flat, flats[ci, i], f"call {ci} item {i}: {path} against {paths[0]}", check_props=True)
                else:
                    flats[ci, i] = flat
    return seen


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(HAND_OVER_ONE))
def test_hand_over_one_composition(gpu_ctx, oracle, monkeypatch, name):
    seen = run_calls(gpu_ctx, oracle, monkeypatch, *HAND_OVER_ONE[name])
    assert seen[None][0]["one_limits"] == 1 and seen["wave"][0]["wave_answered"] == 1 and seen["wide"][0]["wide_items"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(HAND_OVER_BATCH))
def test_hand_over_batch(gpu_ctx, oracle, monkeypatch, name):
    run_calls(gpu_ctx, oracle, monkeypatch, *HAND_OVER_BATCH[name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ARENAS))
def test_arenas(gpu_ctx, oracle, monkeypatch, name):
    run_calls(gpu_ctx, oracle, monkeypatch, *ARENAS[name])


@pytest.mark.gpu
@pytest.mark.parametrize("side", lc.ITEM_SIDES)
def test_items_per_state(gpu_ctx, oracle, monkeypatch, side):
    for n, s, multi in ITEM_CASES:
        if s == side:
            f1, f2 = items_case(n, s, multi)
            run_calls(gpu_ctx, oracle, monkeypatch, f1, [[f2]])


@pytest.mark.gpu
@pytest.mark.parametrize("fold", lc.INTERN_FOLDS + ("twins",))
def test_interning_chunks(gpu_ctx, oracle, monkeypatch, fold):
    cases = TWINS.values() if fold == "twins" else [INTERN["%s:%d" % (fold, n)] for n in lc.INTERN_ARCS]
    for f1, f2 in cases:
        run_calls(gpu_ctx, oracle, monkeypatch, f1, [[f2]])


@pytest.mark.gpu
def test_lookahead_fst_branches(gpu_ctx, oracle, monkeypatch):
    """every second operand alone, then all of them in one call"""
    seconds = list(BRANCH2.values())
    run_calls(gpu_ctx, oracle, monkeypatch, lc.branch1(), [[f2] for f2 in seconds] + [seconds])


@pytest.mark.gpu
def test_pushed_weight_quantization(gpu_ctx, oracle, monkeypatch):
    seconds = list(QUANT2.values())
    run_calls(gpu_ctx, oracle, monkeypatch, lc.quant1(), [seconds] + [[f2] for f2 in seconds])


@pytest.mark.gpu
def test_arena_hint(gpu_ctx, oracle, monkeypatch):
    """a wide result sizes the next wide arena of its handle when the second operands are of one size; the results do not
    depend on it: each equals the same call on a fresh handle (and the oracle)"""
    import rustfst_amd
    f1 = lc.hub1()
    calls = [[HUB2["parallel"]], [HUB2["star_one_padded"]], [HUB2["star_one"]]]
    seen = run_calls(gpu_ctx, oracle, monkeypatch, f1, calls, paths=(None,))[None]
    assert [s["wide_hinted"] for s in seen] == [0, 1, 0] and [s["hint_fallbacks"] for s in seen] == [0, 0, 0]
    assert [s["wide_items"] for s in seen] == [1, 1, 1]
    for call in calls[1:]:
        fresh = run_calls(gpu_ctx, oracle, monkeypatch, f1, [call], paths=(None,))[None]
        assert fresh[0]["wide_hinted"] == 0 and fresh[0]["wide_items"] == 1


@pytest.mark.gpu
def test_mixed_batch(gpu_ctx, oracle, monkeypatch):
    """stays in the wave, handed over by states, handed over by width, arc overflow, start-less and the first handle again in
    ONE call: outputs in order, equal to the single calls; the counters are the sum"""
    f1 = lc.hub1()
    mixed = [HUB2[k] for k in MIXED]
    seen = run_calls(gpu_ctx, oracle, monkeypatch, f1, [mixed] + [[f2] for f2 in mixed[:5]])
    assert seen[None][0] == counters(items=6, items_no_start=1, wave_answered=2, handed_over_states=1, handed_over_width=1,
                                     overflow_arcs=1, wide_items=3, wide_grows=1)


@pytest.mark.gpu
def test_refused_operand_leaves_only_items(gpu_ctx, oracle, monkeypatch):
    """the counters are reset when the call begins: a call that is KO for an unsorted operand does not keep the last call's"""
    import rustfst_amd
    f1, calls = HAND_OVER_ONE["star:%d" % (SWITCH_WIDTH_ONE + 1)]
    assert run_calls(gpu_ctx, oracle, monkeypatch, f1, calls, paths=(None,))[None][0]["wide_items"] == 1
    la = rustfst_amd.LookAhead(to_device(f1, gpu_ctx))
    unsorted = helpers.fst([[(2, 2, 0.0, 0), (1, 1, 0.0, 0)]], [0.0])
    with pytest.raises(rustfst_amd.WfstError, match="not sorted"):
        la.compose_batch([la.relabel(to_device(calls[0][0], gpu_ctx)), to_device(unsorted, gpu_ctx)], gpu_ctx)
    assert gpu_ctx.lookahead_stats() == counters(items=2)
