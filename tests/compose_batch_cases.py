"""Inputs and the routing restatement of tests/test_compose_batch.py (no tests here).  The generators that put a
composition ON a capacity of compose()'s arena are restated from tests/test_compose_limits.py, as is the status one launch
of the wave body reports; the routing of a LIST is include/wfst.h's rule for wfst_compose_batch, written out once."""
import functools
import json
import os

import numpy as np

from helpers import GOLDEN_DIR, _flat, analyse, empty_flat, finals_of, fst, random_fst_flat, string

WAVE = 64            # one level staged in LDS holds 64 arcs; the single call hands over at more than 64 new states
WIDE_STATES = 16384  # WIDE_COMPOSE_STATES
MIN_S, MIN_A = 64, 128  # make_caps' floor: what WFST_COMPOSE_BATCH_ARENA=min starts every item with
COUNTERS = ("launches", "items_in_kernel", "items_single", "items_no_start", "regrown_states", "regrown_arcs", "regrown_hash")
SIGNATURES = {
    "wfst_compose_batch": "wfst_ctx* ctx, const wfst_fst* const* fst1s, size_t n1, const wfst_fst* const* fst2s, size_t n2, "
                          "const wfst_compose_config* cfg, wfst_fst** outs, uint8_t* in_kernel",
    "wfst_ctx_get_compose_batch_counters": "wfst_ctx* ctx, " + ", ".join("uint64_t* " + k for k in COUNTERS),
}


def pow2(x):
    p = 1
    while p < x:
        p <<= 1
    return p


def compose_caps(n1, n2):
    s = 4 * max(min(n1, n2), 64) + 1024
    return s, 4 * s


def hash_slots(s):
    return pow2(2 * s + 128)


def has_start(f):
    return f["n_states"] > 0 and f["start"] is not None and f["start"] >= 0


# ================================================================ generators
@functools.lru_cache(maxsize=None)
def loop_t(n_labels):
    """one final state, an arc l:l back to it for every label 1..n_labels"""
    return fst([[(l, l, 0.0, 0) for l in range(1, n_labels + 1)]], [0.0])


def chain_t(n, par, extra=0):
    """n states in a chain, `par` parallel arcs (labels 1..par) per step, one more on the first `extra` steps"""
    rows = [[(l, l, ((i + l) % 4) / 4.0, i + 1) for l in range(1, par + 1 + (1 if i < extra else 0))] for i in range(n - 1)] + [[]]
    return fst(rows, finals_of(n, {n - 1: 0.25}))


def fan_case(k):
    """one level of k arcs into ONE state: hi + k + 64 against H"""
    rows = [[(l, l, (l % 8) / 4.0, 1) for l in range(1, k + 1)], []]
    return fst(rows, finals_of(2, {1: 0.0})), loop_t(k)


def new_states_case(m):
    """state 0 reaches m distinct final states in one level, each of which goes on to one sink"""
    rows = [[(j + 1, j + 1, (j % 7) / 4.0, 1 + j) for j in range(m)]]
    rows += [[(1 + j % 3, 1 + j % 3, (j % 5) / 512.0, m + 1)] for j in range(m)] + [[]]
    fin = {1 + j: (j % 4) / 4.0 for j in range(m)}
    fin[m + 1] = 0.0
    return fst(rows, finals_of(m + 2, fin)), loop_t(max(m, 3))


@functools.lru_cache(maxsize=None)
def ring_t(m):
    """a label loop over m states: state i goes to i + 1 (mod m) on label 1; every state final"""
    return fst([[(1, 1, (i % 4) / 4.0, (i + 1) % m)] for i in range(m)], finals_of(m, {i: (i % 3) / 4.0 for i in range(m)}))


@functools.lru_cache(maxsize=None)
def product_pair(m):
    """m x m full product: the first operand steps on label 1 and stands still on 2, the second the other way round"""
    a = fst([[(1, 1, 0.25, (i + 1) % m), (2, 2, 0.0, i)] for i in range(m)], finals_of(m, {m - 1: 0.0}))
    b = fst([[(1, 1, 0.0, i), (2, 2, 0.5, (i + 1) % m)] for i in range(m)], finals_of(m, {m - 1: 0.25}))
    return a, b


ARENA_CASES = {  # name -> (first operand, second operand): S_0 = 1280, A_0 = 5120, H_0 = 4096
    "S": lambda: (loop_t(6), chain_t(1280, 1)), "S+1": lambda: (loop_t(6), chain_t(1281, 1)),
    "A": lambda: (loop_t(6), chain_t(1025, 5)), "A+1": lambda: (loop_t(6), chain_t(1025, 5, 1)),
    "H": lambda: fan_case(4031), "H+1": lambda: fan_case(4032),
}


@functools.lru_cache(maxsize=None)
def arena_case(name):
    return ARENA_CASES[name]()


@functools.lru_cache(maxsize=None)
def arena_list():
    return [arena_case(k) for k in ARENA_CASES]


def _golden_rows(g):
    """{n_states, start, arcs [[state, ilabel, olabel, weight, nextstate] ...], finals [[state, w] ...]} with the word its
    rows' label order gives"""
    rows = [[] for _ in range(g["n_states"])]
    for st, il, ol, w, ns in g["arcs"]:
        rows[st].append((il, ol, w, ns))
    return _flat(g["n_states"], g["start"], rows, finals_of(g["n_states"], dict((st, w) for st, w in g["finals"])))


@functools.lru_cache(maxsize=None)
def known_pairs():
    """the K1 pair of tests/golden/k1_compose.json (with its expected result) and fst![1,2=>2,3] o fst![2,3=>3,4]"""
    with open(os.path.join(GOLDEN_DIR, "k1_compose.json")) as f:
        g = json.load(f)
    m1 = fst([[(1, 2, 0.0, 1)], [(2, 3, 0.0, 2)], []], finals_of(3, {2: 0.0}))
    m2 = fst([[(2, 3, 0.0, 1)], [(3, 4, 0.0, 2)], []], finals_of(3, {2: 0.0}))
    return [(_golden_rows(g["fst1"]), _golden_rows(g["fst2"])), (m1, m2)]


def k1_expected():
    with open(os.path.join(GOLDEN_DIR, "k1_compose.json")) as f:
        return _golden_rows(json.load(f)["expected"])


@functools.lru_cache(maxsize=None)
def random_pairs(count=40, seed=7100, lo=2, hi=30):
    """pairs of lo..hi states with input and output epsilons on both sides, weights on the 1/4 grid; the first operand is
    sorted on output labels, the second on input labels"""
    out = []
    for k in range(count):
        rng = np.random.default_rng(seed + k)
        n1, n2 = int(rng.integers(lo, hi + 1)), int(rng.integers(lo, hi + 1))
        a = random_fst_flat(rng, n1, 4, 3, p_eps_i=0.15, p_eps_o=0.2, p_final=0.5, sort="olabel", weight_grid=4, max_w=20, min_fanout=1)
        b = random_fst_flat(rng, n2, 4, 3, p_eps_i=0.2, p_eps_o=0.15, p_final=0.5, sort="ilabel", weight_grid=4, max_w=20, min_fanout=1)
        out.append((a, b))
    return out


@functools.lru_cache(maxsize=None)
def main_list():
    return known_pairs() + random_pairs()


@functools.lru_cache(maxsize=None)
def degenerate_list():
    """inside a list of ordinary pairs: no start state on side 1, on side 2, a zero-state FST, a composition that connect
    empties, a one-state final FST"""
    pairs = random_pairs()[:4]
    a, b = pairs[0]
    no_start = dict(a, start=None)
    dead = fst([[(1, 1, 0.25, 1)], []], finals_of(2, {}))  # no final state: connect leaves nothing
    one = fst([[]], [0.5])
    return [pairs[0], (no_start, b), pairs[1], (a, dict(b, start=None)), (empty_flat(a["props"]), b), pairs[2], (dead, loop_t(2)),
            (one, one), (one, loop_t(3)), pairs[3]]


@functools.lru_cache(maxsize=None)
def width_list():
    return [new_states_case(64), new_states_case(65), random_pairs()[0]]


@functools.lru_cache(maxsize=None)
def handover_list():
    """3 841 states on both sides: S_0 = 16388, the wide driver from the start; the 3 840-state string: S_0 = 16384, the
    kernel; the 80 x 80 product outgrows S_0 = 1344 and S_1 = 5376 and S_2 > 16384: the wide driver after two regrowths"""
    ring = ring_t(3841)
    return [(string([1] * 3840), ring), (string([1] * 3839), ring), product_pair(80), random_pairs()[1]]


@functools.lru_cache(maxsize=None)
def many_small(count=300):
    """2..20 states; every third item has a second operand of its own, the others share one"""
    pairs = random_pairs(count, 7500, 2, 20)
    shared = pairs[0][1]
    return [(a, b if k % 3 == 0 else shared) for k, (a, b) in enumerate(pairs)]


# ================================================================ the routing, restated
def wave_status(levels, s_cap, a_cap):
    """what one launch of the wave body reports for a composition with these levels (lo, hi, arcs emitted, new states) under
    these capacities, the width hand-over off.  Inside a level the arc guard is asked before the hash guard (n_arcs +
    emitted > A; hi + emitted + 64 > H), the state guard when the level is ranked."""
    h_cap, n_arcs = hash_slots(s_cap), 0
    for lo, hi, emitted, n_new in levels:
        over_a, over_h = emitted - (a_cap - n_arcs), emitted - (h_cap - 64 - hi)
        if over_a > 0 and over_h > 0:
            assert over_a >= over_h or over_h - over_a >= 1024, "arcs and hash guards too close to call"
            return "arcs" if over_a >= over_h else "hash"
        if over_a > 0:
            return "arcs"
        if over_h > 0:
            return "hash"
        if hi + n_new > s_cap:
            return "states"
        n_arcs += emitted
    return "ok"


def predict_list(oracle, pairs, flt=0, arena_min=False):
    """(in_kernel flags, the seven counters) of wfst_compose_batch on `pairs`, from the oracle's untrimmed compositions"""
    n = len(pairs)
    c, flags = dict.fromkeys(COUNTERS, 0), [1] * n
    live = [i for i, (a, b) in enumerate(pairs) if has_start(a) and has_start(b)]
    c["items_no_start"] = n - len(live)
    if len(live) == 1:
        flags[live[0]] = 0
    else:
        for i in live:
            a, b = pairs[i]
            s, cap_a = (MIN_S, MIN_A) if arena_min else compose_caps(a["n_states"], b["n_states"])
            levels, launches = analyse(oracle, a, b, flt)["levels"], 0
            while True:
                if s > WIDE_STATES:
                    flags[i] = 0
                    break
                launches += 1
                st = wave_status(levels, s, cap_a)
                if st == "ok":
                    break
                c["regrown_" + st] += 1
                s, cap_a = 4 * s, 4 * cap_a
            c["launches"] = max(c["launches"], launches)
    c["items_single"] = flags.count(0)
    c["items_in_kernel"] = flags.count(1)
    return flags, c
