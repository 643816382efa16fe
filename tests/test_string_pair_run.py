"""The pair levels of string_compose_sp_kernel (compose.hip): the loop that takes the run levels also carries a frontier of one
or two states over a level whose matches, in (frontier state, arc position) order, are one or two with distinct destinations.

The rule, as walk() below restates it.  A level at `pos` is carried when the run is on (it was entered at a level of ONE
state with a block of at most 64 arcs, a level behind it in the string and hi + 1 < maxs, and no level since has ended it),
WFST_STRING_PAIR is not 0, every frontier state's block has at most 64 arcs, pos + 1 < L, the matches number t in {1, 2}, two
matches go to two states, and hi + t < maxs.  One state and one match is a run level (string_run_stats()); every other carried
level is a pair level (string_pair_counts(): pair_levels, and pair_splits for t == 2).  Everything else ends the run and is
the general level's: no match, three matches or more, two matches into one state, a block of 65 arcs, the string's last
level, the slice limit.

Every case is answered five ways and compared bit for bit — pair levels on, WFST_STRING_PAIR=0, WFST_STRING_RUN=0, the general
kernel (WFST_STRING_KERNEL=0), the oracle: path arcs, weights and final weight of every string, the composed states and arcs
of the call — and both counter sets are compared with the walk, so a pair path that is silently off fails the test."""
import collections
import functools

import numpy as np
import pytest

from rustfst_amd import synth

import helpers
from helpers import analyse_string, assert_flat_identical, finals_of, fst, string, to_device, wstring
from string_cases import RUN_BLOCK, STR_LEVEL, STR_MAXS, STR_SCALAR_MAX_N, string_slice

INF = float("inf")
ZERO_RUN = dict(run_levels=0, runs=0)
ZERO_PAIR = dict(pair_levels=0, pair_splits=0)


# ================================================================ the prediction
def walk(labels, t, maxs, pairs=True):
    """what the kernel's vector path does with string o T in a slice of maxs states: composed states, widest level, the four
    counters, and `shapes`: how many levels were ("run" | "pair" | "general", frontier states, matches, new states)"""
    off, arcs = t["offsets"].tolist(), t["arcs"]
    il, ns = arcs["ilabel"].tolist(), arcs["nextstate"].tolist()
    L = len(labels)
    frontier, hi, widest = [int(t["start"])], 1, 1
    c = dict(run_levels=0, runs=0, pair_levels=0, pair_splits=0)
    shapes = collections.Counter()
    on = prev_run = False
    for pos in range(L):
        lab = int(labels[pos])
        dests = [ns[e] for q in frontier for e in range(off[q], off[q + 1]) if il[e] == lab]  # (frontier state, arc position) order
        t_, new, F = len(dests), list(dict.fromkeys(dests)), len(frontier)
        blocks_ok = all(off[q + 1] - off[q] <= RUN_BLOCK for q in frontier)
        if not on:  # the run is entered at a level of one state
            on = F == 1 and blocks_ok and pos + 1 < L and hi + 1 < maxs
        is_run = on and F == 1 and t_ == 1
        carried = is_run or (on and pairs and F <= 2 and blocks_ok and pos + 1 < L and 1 <= t_ <= 2 and len(new) == t_
                             and hi + t_ < maxs)
        # the run level as string_cases.walk states it, without the state `on`
        assert is_run == (F == 1 and blocks_ok and pos + 1 < L and hi + 1 < maxs and t_ == 1)
        if is_run:
            c["run_levels"] += 1
            c["runs"] += not prev_run
        elif carried:
            c["pair_levels"] += 1
            c["pair_splits"] += t_ == 2
        prev_run = is_run
        shapes[("run" if is_run else "pair" if carried else "general", F, t_, len(new))] += 1
        hi += len(new)
        widest = max(widest, len(new))
        frontier = new
        # the loop goes on while the next level has short blocks, a level behind it and a free state beyond the next one
        on = carried and all(off[q + 1] - off[q] <= RUN_BLOCK for q in new) and pos + 2 < L and hi + 1 < maxs
        if not frontier:
            break
    return dict(n_states=hi, widest=widest, shapes=shapes, **c)


def brute_force(labels, t, maxs):
    """the same counters from a frontier enumeration with sets of numpy arrays first and the rule's words second"""
    off, il, ns = t["offsets"].astype(np.int64), t["arcs"]["ilabel"], t["arcs"]["nextstate"].astype(np.int64)
    L, levels, front, hi = len(labels), [], np.array([int(t["start"])]), 1
    for pos in range(L):
        idx = np.concatenate([np.arange(off[q], off[q + 1]) for q in front]) if len(front) else np.zeros(0, dtype=np.int64)
        hit = idx[il[idx] == labels[pos]]
        d = ns[hit]
        _, first = np.unique(d, return_index=True)
        new = d[np.sort(first)]
        levels.append(dict(F=len(front), t=len(d), distinct=len(new) == len(d), hi=hi, last=pos + 1 == L,
                           short=bool(np.all(off[front + 1] - off[front] <= 64))))
        hi += len(new)
        front = new
        if not len(front):
            break
    c = dict(run_levels=0, runs=0, pair_levels=0, pair_splits=0)
    on = prev = False
    for lv in levels:
        enter = lv["F"] == 1 and lv["short"] and not lv["last"] and lv["hi"] + 1 < maxs
        on = on or enter
        kind = None
        if on and lv["F"] <= 2 and lv["short"] and not lv["last"] and lv["t"] in (1, 2) and lv["distinct"] and lv["hi"] + lv["t"] < maxs:
            kind = "run" if (lv["F"], lv["t"]) == (1, 1) else "pair"
        if kind == "run":
            c["run_levels"] += 1
            c["runs"] += prev != "run"
        elif kind == "pair":
            c["pair_levels"] += 1
            c["pair_splits"] += lv["t"] == 2
        prev, on = kind, kind is not None
    return dict(n_states=hi, **c)


def predict(strs, t, scalar, unpacked):
    """(string_run_stats(), string_pair_counts(), problems answered, problems handed back) of one call with everything on"""
    eligible = [s for s in strs if s["n_states"] <= STR_MAXS]
    run, pair, answered, back = dict(ZERO_RUN), dict(ZERO_PAIR), 0, 0
    if not eligible:
        return run, pair, answered, back
    vector = scalar == "0" or (scalar is None and len(eligible) > STR_SCALAR_MAX_N)
    maxs = string_slice(len(eligible), max(s["n_states"] for s in eligible), unpacked)
    for s in eligible:
        w = walk(s["arcs"]["ilabel"], t, maxs)
        if w["widest"] <= STR_LEVEL and w["n_states"] <= maxs:
            answered += 1
            if vector:  # (scalar rows: neither the run nor the pair levels are entered)
                for k in run:
                    run[k] += w[k]
                for k in pair:
                    pair[k] += w[k]
        else:
            back += 1
    return run, pair, answered, back


MODES = (("pair", {}), ("no_pair", {"WFST_STRING_PAIR": "0"}), ("no_run", {"WFST_STRING_RUN": "0"}),
         ("general", {"WFST_STRING_KERNEL": "0"}))
KNOBS = ("WFST_STRING_PAIR", "WFST_STRING_RUN", "WFST_STRING_KERNEL", "WFST_STRING_SCALAR", "WFST_STRING_UNPACKED")


def five_ways(ctx, oracle, monkeypatch, strs, t, sizes, scalar=None, unpacked=False, min_pair_levels=1, handed_back=0):
    import rustfst_amd
    dt, handles = to_device(t, ctx), rustfst_amd.DeviceFst.upload_many(strs, ctx)
    ans = [analyse_string(oracle, s, t) for s in strs]
    seen = 0
    for n in sizes:
        want_run, want_pair, answered, back = predict(strs[:n], t, scalar, unpacked)
        assert back == handed_back, (n, back)
        seen += want_pair["pair_levels"]
        for mode, env in MODES:
            for name in KNOBS:
                monkeypatch.delenv(name, raising=False)
            for name, val in dict(env, WFST_STRING_SCALAR=scalar, WFST_STRING_UNPACKED="1" if unpacked else None).items():
                if val is not None:
                    monkeypatch.setenv(name, val)
            outs, n_arcs = rustfst_amd.compose_shortest_path_batch(handles[:n], dt)
            what = "%s, batch of %d" % (mode, n)
            for k in range(n):
                assert_flat_identical(outs[k].to_flat(), ans[k]["path"], "%s, string %d" % (what, k), check_props=True)
            assert n_arcs == sum(a["n_arcs"] for a in ans[:n]), what
            assert int(ctx.stats()["compose_states"]) == sum(a["n_states"] for a in ans[:n]), what
            got_run, got_pair, st = ctx.string_run_stats(), ctx.string_pair_counts(), ctx.compose_path_stats()
            assert got_run == (want_run if mode in ("pair", "no_pair") else ZERO_RUN), (what, got_run, want_run)
            assert got_pair == (want_pair if mode == "pair" else ZERO_PAIR), (what, got_pair, want_pair)
            if mode != "general":
                assert (st["string_answered"], st["string_handed_back"]) == (answered, back), (what, st)
            else:
                assert st["string_answered"] == 0, (what, st)
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    assert seen >= min_pair_levels, "the case has no pair level at all"


# ================================================================ generators
H, A, B, A2, B2, C, D, FAN0, N_FAN = 0, 1, 2, 3, 4, 5, 6, 7, 10


@functools.lru_cache(maxsize=None)
def ev_t():
    """the hub H and the pair (A, B) it splits into on label 5 (A at 1/2, B at 1/4).  Every arc has its own output label, so
    a path names its arcs.  On the pair: 1 only A has (-> H), 8 only B (-> H); 2 takes A -> A2 and B -> B2, and back; 10
    keeps both; 11: B matches two arcs (-> A, B) and A none; 12: A matches two (-> A2, B2) and B none; 3 and 13 take both
    to C, at tied totals (3/4 each way) and with the second way better; 15: two arcs of A and one of B.  On H: 1, 2, 3 one
    arc each; 4 and 14 two arcs into D (second better / equal); 6 nothing; 7 three arcs; 16 fans out to ten states that
    keep themselves on 16 and fall back to H on 17"""
    rows = [[] for _ in range(FAN0 + N_FAN)]
    ol = [1000]

    def arc(s, label, w, d):
        ol[0] += 1
        rows[s].append((label, ol[0], w, d))

    for label, w in ((1, 0.125), (2, 0.25), (3, 0.375)):
        arc(H, label, w, H)
    arc(H, 4, 0.75, D), arc(H, 4, 0.25, D)
    arc(H, 5, 0.5, A), arc(H, 5, 0.25, B)
    arc(H, 7, 0.125, A), arc(H, 7, 0.25, B), arc(H, 7, 0.5, A2)
    arc(H, 14, 0.5, D), arc(H, 14, 0.5, D)
    for k in range(N_FAN):
        arc(H, 16, 0.125 * (k % 3), FAN0 + k)
    arc(A, 1, 0.25, H), arc(A, 2, 0.125, A2), arc(A, 3, 0.25, C), arc(A, 10, 0.25, A), arc(A, 12, 0.125, A2), arc(A, 12, 0.25, B2)
    arc(A, 13, 0.5, C), arc(A, 15, 0.125, A2), arc(A, 15, 0.25, B2)
    arc(B, 2, 0.375, B2), arc(B, 3, 0.5, C), arc(B, 8, 0.125, H), arc(B, 10, 0.5, B), arc(B, 11, 0.25, A), arc(B, 11, 0.125, B)
    arc(B, 13, 0.25, C), arc(B, 15, 0.125, C)
    arc(A2, 1, 0.5, H), arc(A2, 2, 0.25, A)
    arc(B2, 2, 0.125, B), arc(B2, 8, 0.25, H)
    arc(C, 1, 0.125, H)
    arc(D, 1, 0.25, H)
    for k in range(N_FAN):
        for j in range(N_FAN):
            arc(FAN0 + k, 16, 0.125 * ((k + j) % 4), FAN0 + j)
        arc(FAN0 + k, 17, 0.125 * (k % 5), H)
    return fst(rows, finals_of(len(rows), {s: 0.125 * (s % 4) for s in range(len(rows))}))


EV_L = 21


def ev_string(event, at, L=EV_L, final_weight=0.0):
    s = [1 + k % 3 for k in range(L)]
    s[at:at + len(event)] = event
    assert at + len(event) <= L
    return string(s, final_weight)


SIMPLE_AT = (0, EV_L // 2, EV_L - 3, EV_L - 2)


@functools.lru_cache(maxsize=None)
def simple_strings():
    """1 -> 2 -> 1 through state 0 of the pair (5 1) and through state 1 (5 8), the split at pos 0, mid-string, L - 3 and L - 2"""
    return [ev_string(ev, at, final_weight=0.25 * (at % 2)) for ev in ([5, 1], [5, 8]) for at in SIMPLE_AT]


CHAINS = {"one_each_then_state_0": [5, 2, 1], "one_each_then_state_1": [5, 2, 8], "stays_two": [5, 10, 10, 2, 2, 1],
          "state_1_matches_two_then_0": [5, 11, 1], "state_1_matches_two_then_1": [5, 11, 8],
          "state_0_matches_two_then_0": [5, 12, 1], "state_0_matches_two_then_1": [5, 12, 8], "again_at_once": [5, 1, 5, 8, 5, 1]}
NOT_CARRIED = {"same_destination_better_second": [4, 1], "same_destination_equal": [14, 1], "diamond_tie": [5, 3, 1],
               "diamond_second_better": [5, 13, 1], "three_of_one": [7, 1], "three_of_two": [5, 15, 1], "no_match_of_two": [5, 6, 1]}


@functools.lru_cache(maxsize=None)
def chain_strings():
    return [ev_string(ev, at) for ev in CHAINS.values() for at in (0, 7)]


@functools.lru_cache(maxsize=None)
def not_carried_strings():
    return [ev_string(ev, at) for ev in NOT_CARRIED.values() for at in (0, 7)]


BOUNDARY_L = 140
BOUNDARY_AT = (62, 63, 64, 126, 127)


@functools.lru_cache(maxsize=None)
def boundary_strings():
    """the split at pos 62, 63, 64, 126 and 127 of 140 labels, as the simple event and as a pair kept over the boundary; every
    string arc has a weight of its own position, so a weight read from the wrong chunk changes the path's arcs"""
    out = []
    for at in BOUNDARY_AT:
        for ev in ([5, 8], [5, 10, 10, 2, 2, 1]):
            s = ev_string(ev, at, L=BOUNDARY_L)
            out.append(wstring(s["arcs"]["ilabel"], [0.125 * (k % 7) for k in range(BOUNDARY_L)], 0.25))
    return out


X64, X65, S1, G = 1, 2, 3, 4


@functools.lru_cache(maxsize=None)
def blk_t():
    """H splits into (X64, S) on 20, (X65, S) on 21, (S, X64) on 22, (S, X65) on 23; X64 has 64 arcs (labels 1..64), X65 65, S
    one (label 70); all of them go to G, which goes back to H on 1"""
    rows = [[(1, 500, 0.125, H), (20, 501, 0.5, X64), (20, 502, 0.25, S1), (21, 503, 0.5, X65), (21, 504, 0.25, S1),
             (22, 505, 0.5, S1), (22, 506, 0.25, X64), (23, 507, 0.5, S1), (23, 508, 0.25, X65)],
            [(l, 1000 + l, 0.125 * (l % 5), G) for l in range(1, 65)],
            [(l, 2000 + l, 0.125 * (l % 7), G) for l in range(1, 66)],
            [(70, 3000, 0.375, G)],
            [(1, 4000, 0.125, H)]]
    return fst(rows, finals_of(5, {H: 0.0, G: 0.5}))


BLOCKS = {20: 2, 21: 1, 22: 2, 23: 1}  # the split's label -> pair levels of [1, split, x, 1, 1]: a block of 65 ends the run behind the split


@functools.lru_cache(maxsize=None)
def block_strings():
    """the match in the first lane, in the last lane of a block of 64, in the second chunk of a block of 65, and in the short block"""
    return [string([1, split, x, 1, 1]) for split in BLOCKS for x in (1, 64, 65, 70) if not (x == 65 and split in (20, 22))]


def limit_string(hi_at_split, tail):
    """[16] * 40 [17] makes 402 states, one state per label 1 after that: the 5 finds `hi_at_split` states made"""
    head = [16] * 40 + [17]
    return string(head + [1] * (hi_at_split - (2 + 10 * 40)) + tail)


@functools.lru_cache(maxsize=None)
def limit_strings():
    """a slice of 512: a split with hi + 2 == 511 (carried), one with hi + 2 == 512 (general; the string ends in 512 states),
    and a string of 513 states (handed back); then 13 short strings with events"""
    short = [ev_string(ev, 2, L=9) for ev in list(CHAINS.values()) + list(NOT_CARRIED.values())[:5]]
    return [limit_string(509, [5, 1, 6]), limit_string(510, [5, 6]), limit_string(510, [5, 1, 6])] + short


LADDER_N = 72


@functools.lru_cache(maxsize=None)
def ladder_t(kind):
    """positions 0..72 with two states each, U and V.  U: 1 goes on, 2 goes on at +inf, 5 splits into (U, V), 6 splits with U
    at +inf, 9 goes on (V has no 9).  V: 1 and 2 go on, 8 crosses to U (U has no 8).  Weights: "w" off the 1/8 grid, "zero"
    all +0.0, "neg" -0.0 and +0.0 in turn"""
    def w(s, k):
        return {"w": 0.125 * ((3 * s + k) % 7), "zero": 0.0, "neg": -0.0 if (s + k) % 2 else 0.0}[kind]
    rows = []
    for s in range(LADDER_N):
        u, v, o = 2 * s + 2, 2 * s + 3, 100 * s
        rows.append([(1, o + 1, w(s, 0), u), (2, o + 2, INF, u), (5, o + 3, w(s, 1), u), (5, o + 4, w(s, 2), v),
                     (6, o + 5, INF, u), (6, o + 6, w(s, 3), v), (9, o + 7, w(s, 4), u)])
        rows.append([(1, o + 51, w(s, 5), v), (2, o + 52, w(s, 6), v), (8, o + 53, w(s, 1), u)])
    rows += [[], []]
    return fst(rows, finals_of(len(rows), {s: 0.0 for s in range(len(rows))}))


LADDER_L = 70


@functools.lru_cache(maxsize=None)
def ladder_strings(kind):
    """U unreached beside V and the path through V (6 1 1 8); the merge through the unreached state (6 1 9: no path); +inf on
    a T arc inside a pair (5 2 1 8); a pair kept across the label chunk; +inf on a string arc at the split and on a pair
    level; in the "neg" family -0.0 on every string arc"""
    sw = {"w": lambda k: 0.125 * (k % 5), "zero": lambda k: 0.0, "neg": lambda k: -0.0}[kind]
    fw = {"w": 0.25, "zero": 0.0, "neg": -0.0}[kind]

    def make(event, at, inf_at=None):
        s = [1] * LADDER_L
        s[at:at + len(event)] = event
        weights = [sw(k) for k in range(LADDER_L)]
        if inf_at is not None:
            weights[inf_at] = INF
        return wstring(s, weights, fw)
    out = [make([6, 1, 1, 8], 2), make([6, 1, 9], 2), make([5, 2, 1, 8], 3), make([5] + [1] * 10 + [8], 58),
           make([5] + [1] * 10 + [9], 58), make([5, 1, 1, 8], 4, inf_at=4), make([5, 1, 1, 8], 4, inf_at=5),
           make([5, 1, 1, 9], 4, inf_at=6), make([5, 5, 5, 8], 0), make([6, 2, 8], 62)]
    return out


RANDOM_SEED, RANDOM_STATES, RANDOM_FANOUT, RANDOM_SIGMA, RANDOM_N, RANDOM_L = 20, 40, 4, 6, 32, 100
RANDOM_SHAPES = (("run", 1, 1, 1), ("pair", 1, 2, 2), ("pair", 2, 1, 1), ("pair", 2, 2, 2), ("general", 1, 2, 1), ("general", 2, 2, 1))


@functools.lru_cache(maxsize=None)
def random_case():
    t = synth.make_transducer(RANDOM_STATES, RANDOM_FANOUT, RANDOM_SIGMA, 0.0, seed=RANDOM_SEED)
    return t, synth.make_acceptors(t, RANDOM_N, RANDOM_L, seed0=7000)


def random_shapes():
    t, strs = random_case()
    shapes, widest = collections.Counter(), 0
    for s in strs:
        w = walk(s["arcs"]["ilabel"], t, 512)
        shapes += w["shapes"]
        widest = max(widest, w["widest"])
    return shapes, widest


# ================================================================ no GPU
def test_new_symbol_declared_exported_and_bound(wfst_lib):
    import rustfst_amd
    from rustfst_amd import _lib
    name = "wfst_ctx_get_string_pair_counts"
    helpers.check_counter_getter(wfst_lib, name, ("pair_levels", "pair_splits"), rustfst_amd.Context.string_pair_counts)
    assert _lib.STRING_PAIR_COUNTS == ("pair_levels", "pair_splits")
    assert all(symbol != name for symbol, _ in _lib.COUNTERS.values())  # outside the table of the *_stats families


def test_the_walk_against_a_brute_force_enumeration():
    """10 000 states, fan-out 10 over 24 labels: levels of one to a few states in every mix, at three slice sizes"""
    t = synth.make_transducer(10_000, 10, 24, 0.0, seed=3)
    total = collections.Counter()
    for seed in range(40):
        labels = synth.random_walk_labels(t, 60, 9000 + seed)[0]
        for maxs in (48, 96, 2048):
            w, b = walk(labels, t, maxs), brute_force(labels, t, maxs)
            assert {k: w[k] for k in b} == b, (seed, maxs)
            total += {k: b[k] for k in ("run_levels", "pair_levels", "pair_splits")}
            off = walk(labels, t, maxs, pairs=False)
            assert (off["run_levels"], off["runs"], off["pair_levels"]) == (w["run_levels"], w["runs"], 0)
    assert total["run_levels"] > 100 and total["pair_levels"] > 100 and 20 < total["pair_splits"] < total["pair_levels"]


def test_the_generators_promise_their_levels():
    t = ev_t()
    for at, s in zip(SIMPLE_AT * 2, simple_strings()):
        w = walk(s["arcs"]["ilabel"], t, 2048)
        carried_merge = at + 2 < EV_L  # at L - 2 the two-state level is the string's last: general
        assert (w["pair_levels"], w["pair_splits"]) == (1 + carried_merge, 1), at
        assert w["shapes"][("general", 2, 1, 1)] == (not carried_merge)
        assert w["run_levels"] == EV_L - 1 - w["pair_levels"] and w["n_states"] == EV_L + 2
    want = {"one_each_then_state_0": (3, 2), "one_each_then_state_1": (3, 2), "stays_two": (6, 5), "state_1_matches_two_then_0": (3, 2),
            "state_1_matches_two_then_1": (3, 2), "state_0_matches_two_then_0": (3, 2), "state_0_matches_two_then_1": (3, 2),
            "again_at_once": (6, 3)}
    for (name, ev), s in zip([(n, e) for n, e in CHAINS.items() for _ in (0, 7)], chain_strings()):
        w = walk(s["arcs"]["ilabel"], t, 2048)
        assert (w["pair_levels"], w["pair_splits"]) == want[name], name
    assert walk(chain_strings()[6]["arcs"]["ilabel"], t, 2048)["shapes"][("pair", 2, 2, 2)] == 1  # state 1 matches two, state 0 none
    general = {"same_destination_better_second": ("general", 1, 2, 1), "same_destination_equal": ("general", 1, 2, 1),
               "diamond_tie": ("general", 2, 2, 1), "diamond_second_better": ("general", 2, 2, 1), "three_of_one": ("general", 1, 3, 3),
               "three_of_two": ("general", 2, 3, 3), "no_match_of_two": ("general", 2, 0, 0)}
    for (name, ev), s in zip([(n, e) for n, e in NOT_CARRIED.items() for _ in (0, 7)], not_carried_strings()):
        w = walk(s["arcs"]["ilabel"], t, 2048)
        assert w["shapes"][general[name]] == 1, (name, w["shapes"])
        assert w["pair_levels"] == (1 if ev[0] == 5 else 0), name
    for s in boundary_strings():
        w = walk(s["arcs"]["ilabel"], t, 2048)
        assert w["pair_levels"] in (2, 6) and w["n_states"] == BOUNDARY_L + 1 + (w["pair_levels"] - 1)
    for s in block_strings():
        labels = s["arcs"]["ilabel"].tolist()
        w = walk(labels, blk_t(), 2048)
        assert w["pair_levels"] == BLOCKS[labels[1]], labels
        assert w["shapes"][("general", 2, 1, 1)] == (BLOCKS[labels[1]] == 1), labels
    lim = limit_strings()
    assert len(lim) == 16 and string_slice(16, max(s["n_states"] for s in lim), False) == 512
    carried, general_, beyond = (walk(s["arcs"]["ilabel"], t, 512) for s in lim[:3])
    assert carried["n_states"] == 512 and carried["shapes"][("pair", 1, 2, 2)] == 1 and carried["shapes"][("general", 2, 1, 1)] == 1
    assert general_["n_states"] == 512 and general_["shapes"][("pair", 1, 2, 2)] == 0 and general_["shapes"][("general", 1, 2, 2)] == 1
    assert beyond["n_states"] == 513 and max(w["widest"] for w in (carried, general_, beyond)) == N_FAN
    assert walk(lim[1]["arcs"]["ilabel"], t, 2048)["shapes"][("pair", 1, 2, 2)] == 1  # (the slice, not the string, made it general)
    for kind in ("w", "zero", "neg"):
        for s in ladder_strings(kind):
            w = walk(s["arcs"]["ilabel"], ladder_t(kind), 2048)
            assert w["pair_levels"] >= 3 and w["n_states"] > LADDER_L + 1


def test_the_random_case_has_every_shape():
    shapes, widest = random_shapes()
    assert widest <= STR_LEVEL
    for shape in RANDOM_SHAPES:
        assert shapes[shape] >= 1, (shape, shapes)
    assert any(k[0] == "general" and k[2] >= 3 for k in shapes)


# ================================================================ GPU
@pytest.mark.gpu
def test_simple_event_at_the_start_mid_string_and_the_end(gpu_ctx, oracle, monkeypatch):
    strs = simple_strings()
    five_ways(gpu_ctx, oracle, monkeypatch, strs + strs[:4], ev_t(), (12,), min_pair_levels=20)


@pytest.mark.gpu
def test_chains_of_two_state_levels_and_their_parents(gpu_ctx, oracle, monkeypatch):
    strs = chain_strings()
    assert len(strs) == 16
    five_ways(gpu_ctx, oracle, monkeypatch, strs, ev_t(), (16,), min_pair_levels=50)
    # the path of "state_1_matches_two" goes through B both times (parent lo + 1), that of "state_0_matches_two" through A
    arcs = {int(o) for s in strs for o in analyse_string(oracle, s, ev_t())["path"]["arcs"]["olabel"]}
    t = ev_t()
    by_b = {int(a["olabel"]) for a in t["arcs"][t["offsets"][B]:t["offsets"][B + 1]] if a["ilabel"] == 11}
    by_a = {int(a["olabel"]) for a in t["arcs"][t["offsets"][A]:t["offsets"][A + 1]] if a["ilabel"] == 12}
    assert by_b <= arcs and by_a <= arcs


@pytest.mark.gpu
def test_equal_destinations_three_matches_and_no_match_end_the_run(gpu_ctx, oracle, monkeypatch):
    strs = not_carried_strings()
    five_ways(gpu_ctx, oracle, monkeypatch, strs, ev_t(), (len(strs),), min_pair_levels=6)
    t = ev_t()
    tie = {int(o) for o in analyse_string(oracle, strs[4], t)["path"]["arcs"]["olabel"]}
    better = {int(o) for o in analyse_string(oracle, strs[6], t)["path"]["arcs"]["olabel"]}
    via = lambda s, label: {int(a["olabel"]) for a in t["arcs"][t["offsets"][s]:t["offsets"][s + 1]] if a["ilabel"] == label}
    assert via(A, 3) <= tie and via(B, 13) <= better  # the earlier source stays on a tie; the second way wins when it is better


@pytest.mark.gpu
def test_blocks_of_64_and_65_arcs_in_either_state_of_a_pair(gpu_ctx, oracle, monkeypatch):
    strs = block_strings()
    assert len(strs) == 14
    five_ways(gpu_ctx, oracle, monkeypatch, strs, blk_t(), (len(strs),), min_pair_levels=18)


@pytest.mark.gpu
def test_splits_around_the_label_chunks(gpu_ctx, oracle, monkeypatch):
    strs = boundary_strings()
    five_ways(gpu_ctx, oracle, monkeypatch, strs, ev_t(), (len(strs),), min_pair_levels=40)


@pytest.mark.gpu
def test_split_at_the_last_states_of_a_packed_slice(gpu_ctx, oracle, monkeypatch):
    five_ways(gpu_ctx, oracle, monkeypatch, limit_strings(), ev_t(), (16,), handed_back=1)


@pytest.mark.gpu
def test_the_same_batch_unpacked(gpu_ctx, oracle, monkeypatch):
    five_ways(gpu_ctx, oracle, monkeypatch, limit_strings(), ev_t(), (16,), unpacked=True)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["w", "zero", "neg"])
def test_infinite_and_signed_zero_weights_on_pair_levels(gpu_ctx, oracle, monkeypatch, kind):
    strs = ladder_strings(kind)
    five_ways(gpu_ctx, oracle, monkeypatch, strs, ladder_t(kind), (len(strs),), min_pair_levels=30)
    paths = [analyse_string(oracle, s, ladder_t(kind))["path"] for s in strs]
    assert paths[0]["n_states"] == LADDER_L + 1 and len(paths[1]["arcs"]) == 0  # through V; through the unreached U: none
    if kind == "neg":
        signs = np.signbit(paths[0]["arcs"]["weight"])
        assert signs.any() and not signs.all()


@pytest.mark.gpu
def test_routes_of_8_and_9_strings(gpu_ctx, oracle, monkeypatch):
    strs = simple_strings() + chain_strings()[:1]
    run, pair, _, _ = predict(strs[:8], ev_t(), None, False)
    assert (run, pair) == (ZERO_RUN, ZERO_PAIR)  # scalar rows: neither the run nor the pair levels
    five_ways(gpu_ctx, oracle, monkeypatch, strs, ev_t(), (8, 9), min_pair_levels=10)
    five_ways(gpu_ctx, oracle, monkeypatch, strs, ev_t(), (8,), scalar="0", min_pair_levels=10)


@pytest.mark.gpu
def test_seeded_random_case(gpu_ctx, oracle, monkeypatch):
    shapes, widest = random_shapes()
    assert widest <= STR_LEVEL and all(shapes[s] >= 1 for s in RANDOM_SHAPES)
    t, strs = random_case()
    five_ways(gpu_ctx, oracle, monkeypatch, strs, t, (len(strs),), min_pair_levels=100)
