"""The two kernels of compose.hip at every limit.  compose_wave_kernel and string_compose_sp_kernel are built from hand-offs
between a fast route and a slower one that returns the same FST: a wrong guard or a branch that never runs changes no
result, an off-by-one inside a branch does, but only on an input that sits exactly on the limit.  Every generator below
places an input ON a limit and its twin one beyond it; only the counters of wfst_ctx_get_compose_path_stats show which
route answered.

Without a GPU: the symbol, where every generator lands (from the oracle's untrimmed composition: its ids are first-touch
BFS order, so its levels are contiguous id ranges), and a Python restatement of the routing that predicts the counters of
every call made below.  On the device: every result against the oracle bit for bit (property word included), the canonical
path and the composed-arc count of the fused forms, and the counters against the prediction.

Weights are on the 1/4 grid (many ties) and the 1/512 grid (few): sums stay exact, so every state of a best path has a
predecessor that is tight in the hop count and the two-step counter is 0 — except in the one input built from 2^24 + 1.

relaunch_path is asserted 0 everywhere: the wave run's path buffer holds caps.S arcs per problem and a path has fewer arcs
than its composition has states (<= S); the string run's holds the sum of the strings' state counts and a path has
n_states - 1 arcs.  Neither can fill before 2^31 arcs.  A hash overflow needs hi + emitted + 64 > H >= 2 S + 128 while
n_arcs + emitted <= A: under the fused batch's caps (A = 2 S) that asks for hi > n_arcs + 64 states, and every state but the
first has an arc into it — it cannot occur there at any attempt; under compose()'s caps (A = 4 S) one level of 4032 arcs
into one state does it at S = 1280, H = 4096."""
import functools
import os

import numpy as np
import pytest

from rustfst_amd import synth

import helpers
from helpers import (FILTERS, NOT_I_LABEL_SORTED, NOT_O_LABEL_SORTED, ROOT, analyse, assert_flat_identical, empty_flat,
                     finals_of, fst, string, to_device)
import small_path_cases as spc
from string_cases import STR_LEVEL, STR_MAXS, STR_PACKED_MIN, STR_SLICES, ladder_t, string_slice

INF = float("inf")
# ---- the kernels' own limits (rustfst_amd/csrc/compose.hip), restated once
WAVE = 64               # :383 small = n_se <= 64; :396 items 64 at a time; :452 level_cnt + total > 64u; :780 / :1017 W = 64
WIDE_STATES = 16384     # :1016 WIDE_COMPOSE_STATES
STR_SCALAR_ARCS = 12    # :1146 fc <= 12u && fb + 12u <= f2_n_arcs
COUNTERS = ("string_answered", "string_handed_back", "wave_first", "relaunch_states", "relaunch_arcs", "relaunch_hash",
            "relaunch_path", "switched_wide", "two_step", "caps_states", "caps_arcs", "caps_hash")
ZERO = dict.fromkeys(COUNTERS, 0)
X = 1000  # the label the strings of the block transducer are made of


def pow2(x):
    p = 1
    while p < x:
        p <<= 1
    return p


def compose_caps(n1, n2):
    """compose() :1673 and make_caps :1367-1377"""
    s = 4 * max(min(n1, n2), 64) + 1024
    return s, 4 * s


def batch_caps(accs):
    """compose_shortest_path_batch_begin :1782-1783"""
    s = 4 * max([64] + [a["n_states"] for a in accs]) + 256
    return s, 2 * s


def hash_slots(s):
    return pow2(2 * s + 128)  # :1374


# ================================================================ generators
@functools.lru_cache(maxsize=None)
def loop_t(n_labels, doubled=0):
    """one final state, an arc l:l back to it for every label 1..n_labels; the first `doubled` labels carry a second arc
    l:l+1000 (weight 1/4): an item with such a label matches two arcs.  As a first operand: a looping acceptor."""
    rows = [[]]
    for l in range(1, n_labels + 1):
        rows[0].append((l, l, 0.0, 0))
        if l <= doubled:
            rows[0].append((l, l + 1000, 0.25, 0))
    return fst(rows, [0.0])


def level_case(counts, n_labels, doubled=0):
    """F o loop_t: state 0 fans out to len(counts) states, state 1 + j has counts[j] arcs (labels 1..counts[j]) into ONE final
    state: the second level emits sum(c + min(c, doubled)) arcs that all reach one destination"""
    k = len(counts)
    rows = [[(j + 1, j + 1, (j % 3) / 4.0, 1 + j) for j in range(k)]]
    rows += [[(l, l, ((l + j) % 5) / 4.0, k + 1) for l in range(1, c + 1)] for j, c in enumerate(counts)]
    rows.append([])
    return fst(rows, finals_of(k + 2, {k + 1: 0.5})), loop_t(n_labels, doubled)


def new_states_case(m, arcs=None):
    """state 0 reaches m distinct final states in one level (over `arcs` >= m arcs), each of which goes on to one sink"""
    arcs = arcs or m
    rows = [[(j + 1, j + 1, (j % 7) / 4.0, 1 + j % m) for j in range(arcs)]]
    rows += [[(1 + j % 3, 1 + j % 3, (j % 5) / 512.0, m + 1)] for j in range(m)] + [[]]
    fin = {1 + j: (j % 4) / 4.0 for j in range(m)}
    fin[m + 1] = 0.0
    return fst(rows, finals_of(m + 2, fin)), loop_t(max(arcs, 3))


def back_arcs_case(fan):
    """state 1 + j of the second level: an arc to the sink, one back to state 0 (an earlier level), one to its neighbour in
    the SAME level and a second one to the sink (a duplicate destination): 4 * fan arcs in that level, cyclic"""
    rows = [[(j + 1, j + 1, (j % 3) / 4.0, 1 + j) for j in range(fan)]]
    for j in range(fan):
        rows.append([(1, 1, 0.25, fan + 1), (2, 2, (j % 2) / 4.0, 0), (3, 3, 0.0 if j % 5 else np.inf, 1 + (j + 1) % fan),
                     (4, 4, 0.25, fan + 1)])
    rows.append([(1, 1, 0.5, fan + 1)])  # the sink loops on itself
    return fst(rows, finals_of(fan + 2, {fan + 1: 0.25, 1: 2.0})), loop_t(max(fan, 4))


def general_then_fast_case():
    """70 arcs into 10 states (the arena route: > 64 arcs), then 20 arcs (staged again)"""
    rows = [[(j + 1, j + 1, (j % 9) / 4.0, 1 + j % 10) for j in range(70)]]
    rows += [[(1, 1, 0.25, 11), (2, 2, (j % 3) / 4.0, 11)] for j in range(10)] + [[]]
    return fst(rows, finals_of(12, {11: 0.0})), loop_t(70)


TRIM_DEAD_CHAINS = (0, 30, 31)


def trim_case(n, dead=TRIM_DEAD_CHAINS):
    """n states: state 0 fans out to 32 parallel chains, level k = ids 1 + 32 (k - 1) ... ; a chain is dead when its last
    state is not final: chains 30, 31 and 0 put dead states at ids 63, 64, 65 and 127, 128"""
    ids = [[] for _ in range(32)]
    for s in range(1, n):
        ids[(s - 1) % 32].append(s)
    rows = [[] for _ in range(n)]
    rows[0] = [(j + 1, j + 1, (j % 4) / 4.0, ids[j][0]) for j in range(32)]
    fin = {}
    for j, chain in enumerate(ids):
        for a, b in zip(chain, chain[1:]):
            rows[a].append((1 + j % 5, 1 + j % 5, ((a + j) % 3) / 4.0, b))
        if j not in dead:
            fin[chain[-1]] = (j % 4) / 4.0
    return fst(rows, finals_of(n, fin)), loop_t(32)


def path_chain(h, shortcuts=False):
    """the best path has h hops: a chain of h arcs of weight 1/4; state 0 also leads to a dead state over a +inf arc.  With
    shortcuts every even state i also reaches i + 2 at weight 1 (dearer, fewer hops): levels are two states wide, arcs run
    inside a level, and the distances settle in the fix-up loop"""
    rows = [[(1 + i % 3, 1 + i % 3, 0.25, i + 1)] for i in range(h)] + [[], []]
    rows[0].append((9, 9, np.inf, h + 1))
    if shortcuts:
        for i in range(0, h - 1, 2):
            rows[i].append((8, 8, 1.0, i + 2))
            rows[i].sort(key=lambda a: a[0])
    return fst(rows, finals_of(h + 2, {h: 0.5})), loop_t(9)


def tie_case():
    """state s = 1 is first reached at (1, 1 hop) and passes (2^24 + 1 -> 2^24, 2 hops) on to t; then s improves to (1/2, 2
    hops) through x, and 2^24 + 1/2 rounds to 2^24 again: t keeps 2 hops and has no predecessor with 1: ST_TIE_ORDER"""
    rows = [[(1, 1, 1.0, 1), (2, 2, 0.25, 2)], [(1, 1, 16777216.0, 3)], [(1, 1, 0.25, 1)], [(1, 1, 0.0, 4)], []]
    return fst(rows, finals_of(5, {4: 0.0})), loop_t(2)


def cyclic_case(grid):
    """a ring with chords (cyclic, sorted by input label only: the second operand alone decides the matching side)"""
    return spc.ring_with_chords(np.random.default_rng(50 + grid), 40, 90, grid), loop_t(5)


def chain_t(n, par, extra=0):
    """n states in a chain, `par` parallel arcs (labels 1..par) per step, one more on the first `extra` steps"""
    rows = [[(l, l, ((i + l) % 4) / 4.0, i + 1) for l in range(1, par + 1 + (1 if i < extra else 0))] for i in range(n - 1)] + [[]]
    return fst(rows, finals_of(n, {n - 1: 0.25}))


def fan_case(k):
    """one level of k arcs into ONE state: hi + k + 64 against H"""
    rows = [[(l, l, (l % 8) / 4.0, 1) for l in range(1, k + 1)], []]
    return fst(rows, finals_of(2, {1: 0.0})), loop_t(k)


BLOCK_LAYOUTS = {"ends_at_63": (60, 64), "starts_at_63": (63, 67), "crosses_63_64": (62, 66), "ends_the_block": None}
BLOCK_SIZES = ((62, 63), (63, 64), (64, 65), (127, 129))  # (iterated arcs, searched arcs); items = iterated arcs + 1
BLOCK_MODES = ("both_first_iterates", "both_second_iterates", "input_only", "output_only")


def block_run(layout, n_se):
    """[a, b): where the run of equal labels lies in a searched block of n_se arcs (at least two arcs, clipped to the block)"""
    a, b = BLOCK_LAYOUTS[layout] or (n_se - 3, n_se)
    a = min(a, n_se - 2)
    return a, min(max(b, a + 2), n_se)


@functools.lru_cache(maxsize=None)
def block_pair(n_it, n_se, layout, mode, many=False, eps=False):
    """One composed state does all the work: the start states of the two operands have n_it and n_se arcs.  The searched
    block's labels are distinct and even (odd labels match nothing) except for one run of equal labels placed by `layout`;
    the iterated block holds labels that match 0, 1 and several (the run) arcs, among them the arcs at positions 61..64 and
    the last one, and its own LAST arc matches the searched block's last arc.  many: every iterated arc matches (> 64 arcs
    emitted: the arena route).  eps: the searched block begins with two real epsilon arcs and the iterated block with one
    epsilon arc (the EpsLoop and the real arcs behind it).  mode: which operand iterates, and whether both are sorted."""
    a, b = block_run(layout, n_se)
    se = [10 + 2 * p for p in range(n_se)]
    for p in range(a, b):
        se[p] = 10 + 2 * a
    if eps:
        se[0] = se[1] = 0
    top = se[-1]
    it = [se[p] for p in (2, 3, 61, 62, n_se - 1) if p < n_se] + [10 + 2 * a] * 2 + [top]
    it += [se[p] for p in (63, 64) if p < n_se]
    it = it[:n_it - (1 if eps else 0)]
    j = 0
    while len(it) < n_it - (1 if eps else 0):
        it.append((se[a] if j % 2 == 0 else se[2 + (j * 7) % (n_se - 2)]) if many else 11 + 2 * (j % max(1, n_se - 8)))
        j += 1
    it = ([0] if eps else []) + sorted(it)
    assert len(it) == n_it and it[-1] == top == max(se)
    first_iterates = mode in ("both_first_iterates", "input_only")
    # an arc of the first operand matches on its output label, one of the second on its input label
    def arcs(labels, first, n_dest, grid):
        return [((500 + k, l) if first else (l, 500 + k)) + ((k % 7) / grid, 1 + k % n_dest) for k, l in enumerate(labels)]
    rows_it = [arcs(it, first_iterates, 3, 4.0), [], [], []]
    rows_se = [arcs(se, not first_iterates, 2, 512.0), [], []]
    if mode in ("input_only", "output_only"):
        rows_it[0].reverse()  # the iterated operand is not sorted (and says so)
    f_it = fst(rows_it, finals_of(4, {1: 0.0, 2: 0.25, 3: 0.5}))
    f_se = fst(rows_se, finals_of(3, {1: 0.25, 2: np.inf if many else 0.0}))
    return (f_it, f_se) if first_iterates else (f_se, f_it)


# ---- the string kernel's second operands
def _block(size, matches, sink):
    """`size` arcs sorted by input label; the arcs at the (contiguous) positions of `matches` {pos: (dest, weight, olabel)}
    carry X, the ones before labels below X, the ones after labels above; non-matching arcs lead to `sink`"""
    pos = sorted(matches)
    assert pos == list(range(pos[0], pos[-1] + 1)) and pos[-1] < size
    out = []
    for p in range(size):
        if p in matches:
            d, w, ol = matches[p]
            out.append((X, ol, w, d))
        else:
            out.append((1 + p if p < pos[0] else X + 1 + p, 7, 0.25, sink))
    return out


@functools.lru_cache(maxsize=None)
def block_t(last):
    """a chain c0..c5 of ONE-match levels with blocks of 3, 12 (match at its last position: the last scalar row), 13 (match at
    position 12: one beyond), 64, 20 and 65 arcs (entered by one match: the early rows hold 64); the 65-arc block has ONE
    match in its first 64 arcs (at 63) and one behind them (at 64), to c6 and c6b; c6's 128 arcs have a run of two matches
    across 63 / 64; c6 and c6b reach d0, and d0 and d1 reach e, at the same distance (the earlier source stays); e's
    block of `last` arcs (12: starts exactly 12 arcs before the end of the arc array; 11: one short of what the scalar rows
    read) is the LAST of the array; every state but the sink is final, so every prefix of X^9 has a path"""
    c = list(range(7))
    c6b, d0, d1, e, f, sink = 7, 8, 9, 10, 11, 12
    rows = [_block(3, {1: (c[1], 0.25, 1)}, sink), _block(12, {11: (c[2], 0.5, 2)}, sink), _block(13, {12: (c[3], 0.25, 3)}, sink),
            _block(64, {63: (c[4], 0.0, 4)}, sink), _block(20, {0: (c[5], 0.25, 5)}, sink),
            _block(65, {63: (c[6], 0.75, 60), 64: (c6b, 0.75, 61)}, sink),
            _block(128, {63: (d0, 0.25, 70), 64: (d1, 0.25, 71)}, sink), _block(2, {0: (d0, 0.25, 72)}, sink),
            _block(2, {0: (e, 0.5, 80)}, sink), _block(2, {0: (e, 0.5, 81)}, sink),
            _block(last, {last - 1: (f, 0.25, 9)}, sink), [], []]
    t = fst(rows, finals_of(13, {s: (s % 4) / 4.0 for s in range(12)}))
    assert int(t["offsets"][e]) + last == len(t["arcs"])  # (e's block ends the arc array)
    return t


@functools.lru_cache(maxsize=None)
def tie_t():
    """a and b reach c at 3/4 both (the earlier source, a, stays); c has two equal arcs to d (the earlier position stays); the
    only way into e costs +inf: the string 1^4 has no path, 1^3 ends in d"""
    rows = [[(1, 7, 0.5, 1), (1, 8, 0.25, 2)], [(1, 7, 0.25, 3)], [(1, 8, 0.5, 3)], [(1, 5, 1.0, 4), (1, 6, 1.0, 4)],
            [(1, 9, np.inf, 5)], []]
    return fst(rows, finals_of(6, {4: 0.25, 5: 0.0}))


@functools.lru_cache(maxsize=None)
def len_t():
    """5 states, labels 1..3 everywhere with distinct output labels and weights, label 3 to two states: a label read from
    the wrong position of the string changes the path"""
    rows = [[(l, 10 * s + l, ((s + l) % 4) / 4.0, (2 * s + l) % 5) for l in (1, 2, 3)] + [(3, 10 * s + 4, ((s + 1) % 4) / 4.0, (s + 1) % 5)]
            for s in range(5)]
    return fst(rows, finals_of(5, {s: s / 512.0 for s in range(5)}))


STRING_LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129)


@functools.lru_cache(maxsize=None)
def length_strings():
    rng = np.random.default_rng(129)
    return [string(rng.integers(1, 4, n), 0.25 * (k % 2)) for k, n in enumerate(STRING_LENGTHS)]


@functools.lru_cache(maxsize=None)
def block_strings():
    """every prefix of X^10, and X^4 followed by a label c4 does not have (a chain that ends in a level with no match)"""
    return [string([X] * n) for n in range(11)] + [string([X] * 4 + [999])]  # (f has no arcs: X^10 finds no match at its end)


@functools.lru_cache(maxsize=None)
def tie_strings():
    return [string([1] * n) for n in (1, 2, 3, 4)]


SLICE_SHAPES = {512: (7, 73), 1024: (3, 341), 2048: (1, 2047)}  # slice -> (level width w, labels L): 1 + L * w == slice


@functools.lru_cache(maxsize=None)
def slice_batch(slice_, beyond):
    """a packed batch of 16: one long string that sets maxs and composes to exactly `slice_` states (beyond: one more),
    and 15 short ones.  2048 + 1 with a string the kernel still takes: 1024 labels against ladder_t(2)."""
    w, L = SLICE_SHAPES[slice_]
    if beyond and slice_ == 2048:
        w, L = 2, 1024
        long_ = string([1] * L)
    else:
        long_ = string([1] * (L - 1) + [2 if beyond else 1])
    return [long_] + [string([1] * (1 + k % 3)) for k in range(15)], ladder_t(w)


# ================================================================ what the oracle says about an input
def dead_states(cf):
    """ids of the untrimmed composition from which no final state is reached"""
    n, off, nx = cf["n_states"], cf["offsets"], cf["arcs"]["nextstate"]
    into = [[] for _ in range(n)]
    for s in range(n):
        for t in nx[off[s]:off[s + 1]]:
            into[int(t)].append(s)
    live = [bool(np.isfinite(cf["finals"][s])) for s in range(n)]
    todo = [s for s in range(n) if live[s]]
    while todo:
        for s in into[todo.pop()]:
            if not live[s]:
                live[s] = True
                todo.append(s)
    return [s for s in range(n) if not live[s]]


def needs_two_step(cf):
    """shortest_path.rs:214-272 with (distance, hops) labels in f32, relaxed in FIFO order: does a state of the best path lack
    a predecessor whose label is tight in the distance AND the hop count?  (Never with exact sums.)"""
    n, off = cf["n_states"], cf["offsets"]
    if n == 0:
        return False
    w, nx = cf["arcs"]["weight"].astype(np.float64).tolist(), cf["arcs"]["nextstate"].tolist()
    f32 = lambda x: float(np.float32(x))
    d, h, queue, inq = [INF] * n, [1 << 40] * n, [0], [False] * n
    d[0], h[0] = 0.0, 0
    while queue:
        s = queue.pop(0)
        inq[s] = False
        for k in range(int(off[s]), int(off[s + 1])):
            c = f32(d[s] + w[k]) + 0.0
            if c < INF and (c, h[s] + 1) < (d[nx[k]], h[nx[k]]):
                d[nx[k]], h[nx[k]] = c, h[s] + 1
                if not inq[nx[k]]:
                    inq[nx[k]] = True
                    queue.append(nx[k])
    best = min([(f32(d[s] + float(cf["finals"][s])), s) for s in range(n) if d[s] < INF and cf["finals"][s] < np.inf] + [(INF, -1)])
    if best[1] < 0:
        return False
    tight = [None] * n
    for s in range(n):
        for k in range(int(off[s]), int(off[s + 1])):
            if d[s] < INF and f32(d[s] + w[k]) + 0.0 == d[nx[k]] and h[s] + 1 == h[nx[k]] and tight[nx[k]] is None:
                tight[nx[k]] = s
    s = best[1]
    while h[s] > 0:
        if tight[s] is None:
            return True
        s = tight[s]
    return False


# ================================================================ the routing, restated
def has_start(f):
    return f["n_states"] > 0 and f["start"] is not None and f["start"] >= 0


def is_string(f):
    """fst_store.hip detect_string: linear from state 0, one epsilon-free acceptor arc per state, only the last state final"""
    n = f["n_states"]
    if n == 0 or f["start"] != 0 or len(f["arcs"]) != n - 1:
        return False
    a = f["arcs"]
    return (np.array_equal(f["offsets"][:n], np.arange(n)) and np.array_equal(a["nextstate"], np.arange(1, n))
            and np.array_equal(a["ilabel"], a["olabel"]) and not (a["ilabel"] == 0).any()
            and not np.isfinite(f["finals"][:n - 1]).any() and bool(np.isfinite(f["finals"][n - 1])))


def wave_status(levels, s_cap, a_cap, wide_width):
    """what one launch of compose_wave_kernel reports for a composition with these levels under these capacities"""
    h_cap, n_arcs, fast = hash_slots(s_cap), 0, True
    for lo, hi, emitted, n_new in levels:
        over_a, over_h = emitted - (a_cap - n_arcs), emitted - (h_cap - 64 - hi)  # > 0: that guard fires inside the level
        if over_a > 0 and over_h > 0:  # both would: the one whose room ends first (64 items at a time; arcs are asked first)
            assert abs(over_a - over_h) >= 1024 or over_a >= over_h, "arcs and hash guards too close to call"
            return "arcs" if over_a >= over_h else "hash"
        if over_a > 0:
            return "arcs"
        if over_h > 0:
            return "hash"
        if hi + n_new > s_cap:
            return "states"
        if not fast or emitted > WAVE:  # the arena route; a staged level (<= 64 arcs) cannot add more than 64 states
            if wide_width and n_new > wide_width:
                return "wide"
            fast = n_new <= WAVE
        n_arcs += emitted
    return "ok"


def predict_compose(an, pinned_wave):
    """the counters after compose(a, b): WFST_COMPOSE_PATH=wave pins the wave kernel"""
    c = dict(ZERO)
    if not (has_start(an["a"]) and has_start(an["b"])):
        return c
    s, a = compose_caps(an["a"]["n_states"], an["b"]["n_states"])
    first = True
    while True:
        c.update(caps_states=s, caps_arcs=a, caps_hash=hash_slots(s))
        st = wave_status(an["levels"], s, a, 0 if pinned_wave else WAVE)
        if st == "ok":
            c["wave_first"] += first
            return c
        if st == "wide":
            c["switched_wide"] += 1
            return c
        c["relaunch_" + st] += 1
        s, a, first = 4 * s, 4 * a, False
        if not pinned_wave and s > WIDE_STATES:
            c["switched_wide"] += 1
            return c


def predict_batch(oracle, accs, t, flt=0, string_kernel=True, unpacked=False):
    """the counters after compose_shortest_path_batch(accs, t)"""
    c = dict(ZERO)
    if not accs:
        return c
    ans = [analyse(oracle, a, t, flt) for a in accs]
    eligible = [string_kernel and flt in (0, 3) and len(t["arcs"]) > 0 and not (t["arcs"]["ilabel"] == 0).any()
                and is_string(a) and a["n_states"] <= STR_MAXS for a in accs]
    todo = []
    if any(eligible):
        maxs = string_slice(sum(eligible), max(a["n_states"] for a, e in zip(accs, eligible) if e), unpacked)
    for an, e in zip(ans, eligible):
        if not e:
            todo.append(an)
        elif max([0] + [lv[3] for lv in an["levels"]]) > STR_LEVEL or an["full"]["n_states"] > maxs:
            c["string_handed_back"] += 1
            todo.append(an)
        else:
            c["string_answered"] += 1
    s, a = batch_caps(accs)
    first = True
    while todo:
        c.update(caps_states=s, caps_arcs=a, caps_hash=hash_slots(s))
        again = []
        for an in todo:
            st = wave_status(an["levels"], s, a, 0) if has_start(an["a"]) and has_start(an["b"]) else "ok"
            if st == "ok" and needs_two_step(an["full"]):
                c["two_step"] += 1
            elif st == "ok":
                c["wave_first"] += first
            else:
                c["relaunch_" + st] += 1
                again.append(an)
        assert not (again and first and c["string_handed_back"] and len(todo) > c["string_handed_back"]), \
            "hand-backs join a general run that overflowed: relaunched once at the same capacities (not predicted here)"
        todo, s, a, first = again, 4 * s, 4 * a, False
    return c


# ================================================================ the named inputs of the wave kernel
LEVEL_CASES = {  # name -> (counts, labels of the loop, doubled labels, arcs the second level emits)
    "last_state_64": ((20, 20, 24), 64, 0, 64), "last_state_65": ((20, 20, 25), 64, 0, 65),
    "second_chunk_64": ((64,), 70, 0, 64), "second_chunk_65": ((65,), 70, 0, 65),
    "second_chunk_64_ballot": ((64,), 64, 0, 64), "next_state_65_ballot": ((64, 1), 64, 0, 65),  # 64 <= 64: F iterates, ballot
    "loop_iterates_65_items": ((65, 3), 64, 0, 67),  # 65 arcs > 64 labels: the loop iterates (65 items), F's 65 arcs are searched
    "first_state_64": ((32, 0, 0), 40, 32, 64), "first_state_65": ((33, 0, 0), 40, 32, 65),
}
TRIM_SIZES = (64, 65, 128, 129)
HOPS = (1, 2, 3, 4, 5, 63, 64, 65)
ARENA_CASES = {  # name -> (first operand, second operand): see test_arena_generators_sit_on_the_capacities
    "compose_S": lambda: (loop_t(6), chain_t(1280, 1)), "compose_S+1": lambda: (loop_t(6), chain_t(1281, 1)),
    "compose_A": lambda: (loop_t(6), chain_t(1025, 5)), "compose_A+1": lambda: (loop_t(6), chain_t(1025, 5, 1)),
    "batch_S": lambda: (loop_t(6), chain_t(512, 1)), "batch_S+1": lambda: (loop_t(6), chain_t(513, 1)),
    "batch_A": lambda: (loop_t(6), chain_t(257, 4)), "batch_A+1": lambda: (loop_t(6), chain_t(257, 4, 1)),
    "compose_H": lambda: fan_case(4031), "compose_H+1": lambda: fan_case(4032),
    "wide_after_two_relaunches": lambda: (loop_t(2), chain_t(5121, 1)),
}


@functools.lru_cache(maxsize=None)
def wave_case(name):
    kind, _, arg = name.partition(":")
    if kind == "level":
        counts, labels, doubled, _ = LEVEL_CASES[arg]
        return level_case(counts, labels, doubled)
    if kind == "new_states":
        return new_states_case(int(arg))
    if kind == "new_states_over_65_arcs":
        return new_states_case(int(arg), 65)
    if kind == "back_arcs":
        return back_arcs_case(int(arg))
    if kind == "general_then_fast":
        return general_then_fast_case()
    if kind == "trim":
        return trim_case(int(arg))
    if kind == "no_final":
        return trim_case(65, dead=tuple(range(32)))
    if kind == "hops":
        return path_chain(int(arg))
    if kind == "hops_shortcuts":
        return path_chain(int(arg), True)
    if kind == "tie":
        return tie_case()
    if kind == "cyclic":
        return cyclic_case(int(arg))
    if kind == "arena":
        return ARENA_CASES[arg]()
    raise KeyError(name)


LEVEL_NAMES = ["level:" + k for k in LEVEL_CASES]
OUTCOME_NAMES = ["new_states:64", "new_states:65", "new_states_over_65_arcs:64", "back_arcs:3", "back_arcs:30", "general_then_fast"]
TRIM_NAMES = ["trim:%d" % n for n in TRIM_SIZES] + ["no_final"]
PATH_NAMES = ["hops:%d" % h for h in HOPS] + ["hops_shortcuts:5", "hops_shortcuts:65", "cyclic:4", "cyclic:512", "tie"]
ARENA_NAMES = ["arena:" + k for k in ARENA_CASES]


def an_of(oracle, name):
    return analyse(oracle, *wave_case(name))


def same(got, exp, what):
    assert_flat_identical(got, exp, what, check_props=True)


# ================================================================ no GPU
def test_new_symbol_declared_exported_and_bound(wfst_lib):
    import rustfst_amd
    name = "wfst_ctx_get_compose_path_stats"
    header = helpers.check_counter_getter(wfst_lib, name, COUNTERS, rustfst_amd.Context.compose_path_stats)
    text = header[header.index("which route answered the problems of the last wfst_compose"):header.index("wfst_status " + name)]
    text = " ".join(text.replace("\n *", " ").split())
    for limit in ("at most 2048 states", "at most 12 arcs", "more than 64 states", "512 / 1024 / 2048", "2 * max_states + 64",
                  "at most 64 arcs", "items = arcs + 1", "4 * max(min(n1, n2), 64) + 1024", "A = 4 * S", "4 * max(max_states, 64) + 256",
                  "A = 2 * S", "2 * S + 128", "hi + emitted + 64 <= H", "S = 16384", "batches of at most 8", "at least 16"):
        assert limit in text, limit
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        assert name in f.read()


def test_null_ctx_is_ko(wfst_lib):
    helpers.null_ctx_is_ko(wfst_lib, "wfst_ctx_get_compose_path_stats", len(COUNTERS))


def test_capacity_formulas():
    assert compose_caps(1, 1281) == (1280, 5120) and hash_slots(1280) == 4096
    assert compose_caps(200, 300) == (1824, 7296) and compose_caps(4, 3) == (1280, 5120)
    assert batch_caps([dict(n_states=1)]) == (512, 1024) and hash_slots(512) == 2048
    assert batch_caps([dict(n_states=74), dict(n_states=3)]) == (552, 1104)
    assert [string_slice(16, m, False) for m in (74, 224, 225, 480, 481, 2048)] == [512, 512, 1024, 1024, 2048, 2048]
    assert string_slice(15, 74, False) == 2048 and string_slice(16, 74, True) == 2048


def test_block_generators_promise_their_degrees(oracle):
    """both operands' start states have exactly the arcs asked for, sortedness is stated truthfully, the run of equal labels
    lies where the layout says, and the iterated block matches 0, 1 and several arcs, the last item among the matching"""
    for n_it, n_se in BLOCK_SIZES:
        for layout in BLOCK_LAYOUTS:
            for mode in BLOCK_MODES:
                for many in (False, True):
                    f1, f2 = block_pair(n_it, n_se, layout, mode, many)
                    first_iterates = mode in ("both_first_iterates", "input_only")
                    it, se = (f1, f2) if first_iterates else (f2, f1)
                    deg = lambda f: int(f["offsets"][1])
                    assert (deg(it), deg(se)) == (n_it, n_se) and deg(it) + 1 in (63, 64, 65, 128)
                    # match_input :367: under MODE_BOTH the operand with FEWER arcs iterates (the first one on a tie)
                    assert (deg(f1) <= deg(f2)) == first_iterates
                    key_it = it["arcs"]["olabel" if first_iterates else "ilabel"][:n_it].astype(np.int64)
                    key_se = se["arcs"]["ilabel" if first_iterates else "olabel"][:n_se].astype(np.int64)
                    assert np.all(np.diff(key_se) >= 0)
                    o1, i2 = bool(f1["props"] & synth.O_LABEL_SORTED), bool(f2["props"] & synth.I_LABEL_SORTED)
                    assert (o1, i2) == {"input_only": (False, True), "output_only": (True, False)}.get(mode, (True, True))
                    assert bool(f1["props"] & NOT_O_LABEL_SORTED) != o1 and bool(f2["props"] & NOT_I_LABEL_SORTED) != i2
                    a, b = block_run(layout, n_se)
                    run = np.flatnonzero(key_se == key_se[a])
                    assert run.tolist() == list(range(a, b))
                    if layout == "ends_at_63" and n_se > 64:
                        assert run[-1] == 63 and key_se[64] != key_se[63]
                    if layout == "starts_at_63" and n_se > 64:
                        assert run[0] == 63 and len(run) >= 2
                    if layout == "crosses_63_64" and n_se > 64:
                        assert 63 in run and 64 in run
                    if layout == "ends_the_block":
                        assert run[-1] == n_se - 1 and len(run) == 3
                    hits = [int((key_se == l).sum()) for l in key_it]
                    assert 1 in hits and max(hits) == len(run) >= 2 and hits[int(np.argmax(key_it))] >= 1
                    assert (0 in hits) == (not many)
                    an = analyse(oracle, f1, f2)
                    assert an["levels"][0][2] == sum(hits) == int(an["full"]["offsets"][1])
                    assert (sum(hits) > WAVE) == many, (n_it, n_se, layout, mode, many, sum(hits))
    f1, f2 = block_pair(64, 65, "crosses_63_64", "both_first_iterates", False, True)
    assert f1["arcs"]["olabel"][0] == 0 and (f2["arcs"]["ilabel"][:3] == [0, 0, 14]).all()


def test_level_generators_emit_exactly_64_and_65(oracle):
    for name, (counts, labels, doubled, emitted) in LEVEL_CASES.items():
        an = an_of(oracle, "level:" + name)
        assert [lv[2] for lv in an["levels"]] == [len(counts) + min(len(counts), doubled), emitted, 0], name
        assert sum(min(c, labels) + min(c, doubled) for c in counts) == emitted  # (a label the loop lacks matches nothing)
        assert an["levels"][1][3] == 1  # ... which all reach ONE destination
        f, t = wave_case("level:" + name)
        assert [int(f["offsets"][2 + j] - f["offsets"][1 + j]) for j in range(len(counts))] == list(counts)
        assert len(t["arcs"]) == labels + doubled
    # where the 65th arrives: behind 40 staged arcs in the last state; in the item chunk [64, 128) of a lone state (items =
    # arcs + 1: arc 64 is item 65's, arc 63 is item 64, the first of the second chunk); in the first chunk of the first state
    assert LEVEL_CASES["last_state_65"][0][:2] == (20, 20) and LEVEL_CASES["second_chunk_65"][0] == (65,)
    assert LEVEL_CASES["second_chunk_64"][0] == (64,) and 64 + 1 > WAVE  # 64 arcs are 65 items: one item spills, 64 arcs emitted
    assert 2 * 32 == 64 and LEVEL_CASES["first_state_65"][0][0] + 1 <= WAVE  # 33 arcs + the loop item: one chunk, 65 arcs
    # the pairs sit on both sides of n1 <= n2 and of the 64-arc searched block
    assert LEVEL_CASES["loop_iterates_65_items"][:2] == ((65, 3), 64) and LEVEL_CASES["second_chunk_64_ballot"][:2] == ((64,), 64)


def test_outcome_generators(oracle):
    lv = an_of(oracle, "new_states:64")["levels"]
    assert lv[0][2:] == (64, 64) and lv[1][2:] == (64, 1)
    lv = an_of(oracle, "new_states:65")["levels"]
    assert lv[0][2:] == (65, 65) and lv[1][2:] == (65, 1)
    lv = an_of(oracle, "new_states_over_65_arcs:64")["levels"]  # the arena route (65 arcs) with exactly 64 new states
    assert lv[0][2:] == (65, 64) and lv[1][2:] == (64, 1)
    for fan in (3, 30):
        an = an_of(oracle, "back_arcs:%d" % fan)
        lo, hi, emitted, n_new = an["levels"][1]
        assert (lo, hi, emitted, n_new) == (1, 1 + fan, 4 * fan, 1) and (emitted > WAVE) == (fan == 30)
        nx = an["full"]["arcs"]["nextstate"][an["full"]["offsets"][lo]:an["full"]["offsets"][hi]]
        assert (nx == 0).sum() == fan and ((nx >= lo) & (nx < hi)).sum() == fan and (nx == hi).sum() == 2 * fan
        assert np.isposinf(an["full"]["arcs"]["weight"]).sum() >= 1
    lv = an_of(oracle, "general_then_fast")["levels"]
    assert [x[2:] for x in lv[:2]] == [(70, 10), (20, 1)]


def test_trim_generators_put_dead_states_around_the_boundaries(oracle):
    for n in TRIM_SIZES:
        an = an_of(oracle, "trim:%d" % n)
        dead = dead_states(an["full"])
        assert an["full"]["n_states"] == n and an["trim"]["n_states"] == n - len(dead) > 0
        want = [s for s in (63, 64, 65, 127, 128) if s < n] + ([32] if n in (64, 128) else [])
        want = {s for s in want if (s - 1) % 32 in TRIM_DEAD_CHAINS}
        assert {63} <= want and want <= set(dead), (n, dead)
        assert all(s not in dead for s in (62, 66, 126) if s < n)
    an = an_of(oracle, "no_final")  # no co-accessible state: the start state dies with every other
    assert an["full"]["n_states"] == 65 and an["trim"]["n_states"] == 0 and an["hops"] is None


def test_path_generators_have_their_hops(oracle):
    for h in HOPS:
        an = an_of(oracle, "hops:%d" % h)
        assert an["hops"] == h and an["full"]["n_states"] == h + 2 and not needs_two_step(an["full"])
    for h in (5, 65):
        an = an_of(oracle, "hops_shortcuts:%d" % h)
        assert an["hops"] == h and len(an["levels"]) < h and not needs_two_step(an["full"])  # fewer levels than hops
    for grid in (4, 512):
        an = an_of(oracle, "cyclic:%d" % grid)
        assert an["full"]["n_states"] == 40 and an["hops"] is not None and not needs_two_step(an["full"])
    an = an_of(oracle, "tie")
    assert needs_two_step(an["full"]) and an["hops"] == 4
    assert np.float32(16777216.0) + np.float32(1.0) == np.float32(16777216.0) + np.float32(0.5) == np.float32(16777216.0)


def test_arena_generators_sit_on_the_capacities(oracle):
    sizes = {k: (an_of(oracle, "arena:" + k)["full"]["n_states"], len(an_of(oracle, "arena:" + k)["full"]["arcs"])) for k in ARENA_CASES}
    s_c, a_c = compose_caps(1, 1280)
    s_b, a_b = batch_caps([loop_t(6)])
    assert (s_c, a_c, s_b, a_b) == (1280, 5120, 512, 1024)
    assert sizes["compose_S"] == (s_c, s_c - 1) and sizes["compose_S+1"] == (s_c + 1, s_c)
    assert sizes["compose_A"] == (1025, a_c) and sizes["compose_A+1"] == (1025, a_c + 1)
    assert sizes["batch_S"] == (s_b, s_b - 1) and sizes["batch_S+1"] == (s_b + 1, s_b)
    assert sizes["batch_A"] == (257, a_b) and sizes["batch_A+1"] == (257, a_b + 1)
    assert sizes["compose_H"] == (2, 4031) and sizes["compose_H+1"] == (2, 4032) and 1 + 4031 + 64 == hash_slots(s_c)
    assert sizes["wide_after_two_relaunches"] == (5121, 5120) and 4 * s_c < 5121 <= 16 * s_c and 16 * s_c > WIDE_STATES


def _c(**kw):
    return dict(ZERO, **kw)


def test_predicted_counters_of_the_wave_cases(oracle):
    """the restatement on both sides of every limit; all named inputs are predicted (the device tests use the same call)"""
    caps_c, caps_c4 = dict(caps_states=1280, caps_arcs=5120, caps_hash=4096), dict(caps_states=5120, caps_arcs=20480, caps_hash=16384)
    caps_b, caps_b4 = dict(caps_states=512, caps_arcs=1024, caps_hash=2048), dict(caps_states=2048, caps_arcs=4096, caps_hash=8192)
    want = {"compose_S": _c(wave_first=1, **caps_c), "compose_S+1": _c(relaunch_states=1, **caps_c4),
            "compose_A": _c(wave_first=1, **caps_c), "compose_A+1": _c(relaunch_arcs=1, **caps_c4),
            "compose_H": _c(wave_first=1, **caps_c), "compose_H+1": _c(relaunch_hash=1, **caps_c4),
            "batch_S": _c(wave_first=1, **caps_c), "batch_A+1": _c(wave_first=1, **caps_c)}
    for k, w in want.items():
        for pinned in (False, True):
            assert predict_compose(an_of(oracle, "arena:" + k), pinned) == w, k
    an = an_of(oracle, "arena:wide_after_two_relaunches")
    assert predict_compose(an, False) == _c(relaunch_states=2, switched_wide=1, **caps_c4)
    assert predict_compose(an, True) == _c(relaunch_states=2, caps_states=20480, caps_arcs=81920, caps_hash=65536)
    want = {"batch_S": _c(wave_first=1, **caps_b), "batch_S+1": _c(relaunch_states=1, **caps_b4),
            "batch_A": _c(wave_first=1, **caps_b), "batch_A+1": _c(relaunch_arcs=1, **caps_b4),
            "compose_S+1": _c(relaunch_states=1, **caps_b4), "compose_A": _c(relaunch_arcs=2, caps_states=8192, caps_arcs=16384, caps_hash=32768),
            "compose_H+1": _c(relaunch_arcs=1, **caps_b4)}  # (4032 > A = 1024 long before 1 + 4032 + 64 > H = 2048)
    for k, w in want.items():
        a, b = wave_case("arena:" + k)
        assert predict_batch(oracle, [a], b, string_kernel=False) == w, k
    # 65 new states: the wide driver by default, the arena route when pinned; 64: staged, answered at once
    an = an_of(oracle, "new_states:65")
    assert predict_compose(an, False) == _c(switched_wide=1, **caps_c) and predict_compose(an, True) == _c(wave_first=1, **caps_c)
    assert predict_compose(an_of(oracle, "new_states:64"), False) == _c(wave_first=1, **caps_c)
    assert predict_compose(an_of(oracle, "new_states_over_65_arcs:64"), False) == _c(wave_first=1, **caps_c)  # 64 is not > 64
    a, b = wave_case("tie")
    assert predict_batch(oracle, [a], b, string_kernel=False) == _c(two_step=1, **caps_b)
    assert predict_compose(an_of(oracle, "tie"), False) == _c(wave_first=1, **caps_c)
    for name in LEVEL_NAMES + OUTCOME_NAMES + TRIM_NAMES + PATH_NAMES:
        a, b = wave_case(name)
        p = predict_batch(oracle, [a], b, string_kernel=False)
        assert p["wave_first"] + p["two_step"] == 1 and sum(p[k] for k in COUNTERS[:2] + COUNTERS[3:8]) == 0, name
    empty = empty_flat()
    assert predict_compose(analyse(oracle, empty, loop_t(2)), False) == ZERO
    assert wave_status([(0, 1, 65, 65)], 1280, 5120, 64) == "wide" and wave_status([(0, 1, 64, 64), (1, 65, 64, 1)], 1280, 5120, 64) == "ok"
    assert wave_status([(0, 1, 10, 3)], 3, 128, 0) == "states" and wave_status([(0, 1, 10, 2)], 3, 128, 0) == "ok"


def test_string_generators_and_predicted_counters(oracle):
    t = block_t(12)
    off = t["offsets"]
    assert [int(off[s + 1] - off[s]) for s in range(13)] == [3, 12, 13, 64, 20, 65, 128, 2, 2, 2, 12, 0, 0]
    assert int(off[10]) + STR_SCALAR_ARCS == len(t["arcs"]) and int(block_t(11)["offsets"][10]) + 11 == len(block_t(11)["arcs"])
    where = [np.flatnonzero(t["arcs"]["ilabel"][off[s]:off[s + 1]] == X).tolist() for s in range(11)]
    assert where == [[1], [11], [12], [63], [0], [63, 64], [63, 64], [0], [0], [0], [11]]
    assert not is_string(t) and all(is_string(s) for s in block_strings() + length_strings() + tie_strings())
    assert [s["n_states"] - 1 for s in length_strings()] == list(STRING_LENGTHS)
    for last in (12, 11):
        tt = block_t(last)
        widths = [[lv[3] for lv in analyse(oracle, s, tt)["levels"]] for s in block_strings()]
        assert widths[9] == widths[10] == [1] * 5 + [2, 2, 1, 1, 0] and widths[11] == [1, 1, 1, 1, 0]
        ans = [analyse(oracle, s, tt) for s in block_strings()]
        assert [a["hops"] for a in ans] == list(range(10)) + [None, None]
        # c6 / c6b reach d0, and d0 / d1 reach e, at the same distance: the path keeps the earlier source (c6: 60, 70; d0: 80)
        assert ans[9]["path"]["arcs"]["olabel"].tolist()[:4] == [9, 80, 70, 60]
        for n in (1, 8, 9, 15, 16):
            batch = (block_strings() * 2)[:n]
            assert predict_batch(oracle, batch, tt) == _c(string_answered=n)
            assert predict_batch(oracle, batch, tt, string_kernel=False)["wave_first"] == n
    ans = [analyse(oracle, s, tie_t()) for s in tie_strings()]
    assert [a["hops"] for a in ans] == [None, None, 3, None] and ans[2]["path"]["arcs"]["olabel"].tolist() == [5, 7, 7]
    assert ans[3]["full"]["n_states"] == 6 and np.isposinf(ans[3]["full"]["arcs"]["weight"]).sum() == 1
    # a level of exactly 64 states, and 65
    wide = [string([1] * 5), string([1] * 4 + [2])]
    assert max(lv[3] for lv in analyse(oracle, wide[0], ladder_t(64))["levels"]) == STR_LEVEL
    assert max(lv[3] for lv in analyse(oracle, wide[1], ladder_t(64))["levels"]) == STR_LEVEL + 1
    assert predict_batch(oracle, wide, ladder_t(64)) == _c(string_answered=1, string_handed_back=1, wave_first=1, caps_states=512,
                                                           caps_arcs=1024, caps_hash=2048)
    # the slices
    for slice_ in STR_SLICES:
        for beyond in (False, True):
            accs, tt = slice_batch(slice_, beyond)
            n_max = max(a["n_states"] for a in accs)
            assert len(accs) == STR_PACKED_MIN and string_slice(16, n_max, False) == slice_ and accs[0]["n_states"] == n_max
            assert analyse(oracle, accs[0], tt)["full"]["n_states"] == slice_ + beyond
            assert all(analyse(oracle, a, tt)["full"]["n_states"] <= 64 for a in accs[1:])
            s = 4 * n_max + 256
            back = _c(string_answered=15, string_handed_back=1, wave_first=1, caps_states=s, caps_arcs=2 * s, caps_hash=hash_slots(s))
            assert predict_batch(oracle, accs, tt) == (back if beyond else _c(string_answered=16))
            assert predict_batch(oracle, accs, tt, unpacked=True) == (back if beyond and slice_ == 2048 else _c(string_answered=16))
    # 2048 states are a string case, 2049 are not
    yes, no = string([1] * 2047), string([1] * 2048)
    assert (yes["n_states"], no["n_states"]) == (STR_MAXS, STR_MAXS + 1)
    assert predict_batch(oracle, [yes, no], ladder_t(1)) == _c(string_answered=1, wave_first=1, caps_states=8452, caps_arcs=16904,
                                                               caps_hash=32768)
    # routing: filters other than Auto / Sequence, input epsilons in T, a first operand that is not a string
    assert predict_batch(oracle, tie_strings(), tie_t(), flt=5)["string_answered"] == 0
    assert predict_batch(oracle, tie_strings(), tie_t(), flt=3)["string_answered"] == 4
    eps_t = fst([[(0, 1, 0.25, 1), (1, 1, 0.5, 1)], []], finals_of(2, {1: 0.0}))
    assert predict_batch(oracle, tie_strings(), eps_t) == _c(wave_first=4, caps_states=512, caps_arcs=1024, caps_hash=2048)
    assert not is_string(trim_case(64)[0]) and not is_string(path_chain(3)[0])


# ================================================================ GPU
def _stats(ctx):
    st = ctx.compose_path_stats()
    assert tuple(st) == COUNTERS
    return st


def run_pair(ctx, oracle, a, b, monkeypatch, what, flt=0, fused=True):
    """compose(a, b) pinned to the wave kernel and by default, with and without connect, then the fused batch through the
    general kernel: results against the oracle, counters against the prediction"""
    import rustfst_amd
    from rustfst_amd import ComposeConfig, ComposeFilter
    an = analyse(oracle, a, b, flt)
    da, db = to_device(a, ctx), to_device(b, ctx)
    for pinned in (True, False):
        if pinned:
            monkeypatch.setenv("WFST_COMPOSE_PATH", "wave")
        else:
            monkeypatch.delenv("WFST_COMPOSE_PATH", raising=False)
        for connect in (False, True):
            got = da.compose(db, ComposeConfig(ComposeFilter(flt), connect=connect)).to_flat()
            st = _stats(ctx)
            print("%s pinned=%s connect=%s: %s" % (what, pinned, connect, st))
            same(got, an["trim" if connect else "full"], "%s pinned=%s connect=%s" % (what, pinned, connect))
            assert st == predict_compose(an, pinned), what
    if fused:
        monkeypatch.setenv("WFST_STRING_KERNEL", "0")
        outs, n_arcs = rustfst_amd.compose_shortest_path_batch([da], db, ComposeConfig(ComposeFilter(flt)))
        st = _stats(ctx)
        print("%s fused: %s" % (what, st))
        same(outs[0].to_flat(), an["path"], what + " fused")
        assert n_arcs == len(an["full"]["arcs"])
        assert st == predict_batch(oracle, [a], b, flt, string_kernel=False), what
        monkeypatch.delenv("WFST_STRING_KERNEL")
    return an


@pytest.mark.gpu
@pytest.mark.parametrize("mode", BLOCK_MODES)
@pytest.mark.parametrize("sizes", BLOCK_SIZES, ids=lambda s: "%dx%d" % s)
def test_wave_arc_blocks(gpu_ctx, oracle, monkeypatch, sizes, mode):
    """searched blocks of 63, 64, 65 and 129 arcs (ballot up to 64, binary search beyond), iterated blocks of 62, 63, 64 and
    127 arcs (63 arcs fill one chunk of items, 64 spill one), runs of equal labels around position 63 / 64 and at the end of
    the block; emitting <= 64 arcs (staged) and more (the arena route)"""
    for layout in BLOCK_LAYOUTS:
        for many in (False, True):
            a, b = block_pair(sizes[0], sizes[1], layout, mode, many)
            run_pair(gpu_ctx, oracle, a, b, monkeypatch, "blocks %s %s %s many=%s" % (sizes, mode, layout, many))


@pytest.mark.gpu
@pytest.mark.parametrize("flt", [0] + [f.value for f in FILTERS])
def test_wave_epsilon_item_with_real_epsilon_arcs(gpu_ctx, oracle, monkeypatch, flt):
    """the iterated block begins with an epsilon arc, the searched block with two: the matcher's EpsLoop first, the real arcs
    behind it, under every filter; the loop item (key 0) meets the same two arcs"""
    for sizes in ((63, 64), (64, 65)):
        for mode in BLOCK_MODES[:2]:
            a, b = block_pair(sizes[0], sizes[1], "crosses_63_64", mode, False, True)
            an = run_pair(gpu_ctx, oracle, a, b, monkeypatch, "eps %s %s filter %d" % (sizes, mode, flt), flt)
            assert an["full"]["n_states"] > 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", LEVEL_NAMES + OUTCOME_NAMES)
def test_wave_levels_at_64_arcs_and_their_outcomes(gpu_ctx, oracle, monkeypatch, name):
    """a level that emits exactly 64 arcs stays in LDS, its twin with 65 is redone through the arena — the 65th arriving in
    the first state, in the last state behind staged arcs, in the second chunk of one state; 64 / 65 new states (65: the
    wide driver by default), duplicates, arcs back into the level and before it, an arena level followed by a staged one"""
    run_pair(gpu_ctx, oracle, *wave_case(name), monkeypatch, name)
    if name == "new_states:65":
        monkeypatch.delenv("WFST_COMPOSE_PATH", raising=False)
        a, b = wave_case(name)
        to_device(a, gpu_ctx).compose(to_device(b, gpu_ctx))
        assert _stats(gpu_ctx)["switched_wide"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", TRIM_NAMES)
def test_wave_trim_around_the_64_boundaries(gpu_ctx, oracle, monkeypatch, name):
    an = run_pair(gpu_ctx, oracle, *wave_case(name), monkeypatch, name)
    assert (an["trim"]["n_states"] == 0) == (name == "no_final")


@pytest.mark.gpu
@pytest.mark.parametrize("name", PATH_NAMES)
def test_wave_fused_path(gpu_ctx, oracle, monkeypatch, name):
    """best paths of 1..5 and 63, 64, 65 hops (the mark pass doubles its span up to the hops), levels with arcs inside them
    and a cyclic composition (the fix-up loop), and the one input whose path has a state without a hop-tight predecessor"""
    run_pair(gpu_ctx, oracle, *wave_case(name), monkeypatch, name)
    assert _stats(gpu_ctx)["two_step"] == (1 if name == "tie" else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ARENA_NAMES)
def test_wave_arena_capacities(gpu_ctx, oracle, monkeypatch, name):
    """exactly S states, A arcs and H - 64 - hi arcs in a level, and one more of each: one relaunch under its own status"""
    run_pair(gpu_ctx, oracle, *wave_case(name), monkeypatch, name)


STRING_CONFIGS = ((1, "0", False), (1, "1", False), (8, None, False), (8, "0", False), (9, None, False), (9, "1", False),
                  (15, "0", False), (15, "1", False), (16, None, False), (16, "1", False), (16, "0", True), (16, "1", True))


def run_strings(ctx, oracle, strs, t, monkeypatch, what, configs=STRING_CONFIGS, flt=0):
    """the strings in batches of 1, 8, 9, 15 and 16, scalar rows on and off, packed and unpacked, then through the general
    kernel, all on the same handles"""
    import rustfst_amd
    dt, handles = to_device(t, ctx), rustfst_amd.DeviceFst.upload_many(strs, ctx)
    ans = [analyse(oracle, s, t, flt) for s in strs]

    def batch(idx, **kw):
        outs, n_arcs = rustfst_amd.compose_shortest_path_batch([handles[i] for i in idx], dt)
        st = _stats(ctx)
        for k, i in enumerate(idx):
            same(outs[k].to_flat(), ans[i]["path"], "%s %s string %d" % (what, kw, i))
        assert n_arcs == sum(len(ans[i]["full"]["arcs"]) for i in idx)
        want = predict_batch(oracle, [strs[i] for i in idx], t, flt, **kw)
        assert st == want, (what, kw, st, want)
        assert int(ctx.stats()["string_problems"]) == st["string_answered"]
        return st

    for n, scalar, unpacked in configs:
        for name, val in (("WFST_STRING_SCALAR", scalar), ("WFST_STRING_UNPACKED", "1" if unpacked else None)):
            if val is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, val)
        for first in range(0, len(strs), n):
            batch([(first + j) % len(strs) for j in range(n)], unpacked=unpacked)
    monkeypatch.delenv("WFST_STRING_SCALAR", raising=False)
    monkeypatch.delenv("WFST_STRING_UNPACKED", raising=False)
    monkeypatch.setenv("WFST_STRING_KERNEL", "0")
    st = batch(list(range(len(strs))), string_kernel=False)
    assert st["string_answered"] == 0
    monkeypatch.delenv("WFST_STRING_KERNEL")


@pytest.mark.gpu
def test_string_lengths_around_the_64_label_chunks(gpu_ctx, oracle, monkeypatch):
    run_strings(gpu_ctx, oracle, length_strings(), len_t(), monkeypatch, "lengths")


@pytest.mark.gpu
@pytest.mark.parametrize("last", [12, 11])
def test_string_arc_blocks_and_chains(gpu_ctx, oracle, monkeypatch, last):
    """blocks of 12 and 13 arcs with the match in their last row, the last block of T's arc array 12 and 11 arcs long, blocks
    of 64, 65 (behind one match) and 128 arcs with matches at 63 and 64, one-match chains of every length that end in a
    match, in two matches and in none"""
    run_strings(gpu_ctx, oracle, block_strings(), block_t(last), monkeypatch, "blocks(last %d)" % last)


@pytest.mark.gpu
def test_string_ties_and_infinite_way_in(gpu_ctx, oracle, monkeypatch):
    run_strings(gpu_ctx, oracle, tie_strings(), tie_t(), monkeypatch, "ties")


@pytest.mark.gpu
def test_string_level_of_64_and_65_states(gpu_ctx, oracle, monkeypatch):
    strs = [string([1] * 5), string([1] * 4 + [2]), string([1]), string([1, 2])]
    run_strings(gpu_ctx, oracle, strs, ladder_t(64), monkeypatch, "level width")
    import rustfst_amd
    rustfst_amd.compose_shortest_path_batch(rustfst_amd.DeviceFst.upload_many(strs[:2], gpu_ctx), to_device(ladder_t(64), gpu_ctx))
    assert _stats(gpu_ctx)["string_handed_back"] == 1 and _stats(gpu_ctx)["string_answered"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("beyond", [False, True], ids=["fits", "one_more"])
@pytest.mark.parametrize("slice_", STR_SLICES)
def test_string_slice_of_a_packed_batch(gpu_ctx, oracle, monkeypatch, slice_, beyond):
    """a packed batch of 16 whose longest string picks the slice: exactly `slice_` composed states are answered, one more is
    handed back; unpacked, both fit 2048 (but for 2049)"""
    accs, t = slice_batch(slice_, beyond)
    run_strings(gpu_ctx, oracle, accs, t, monkeypatch, "slice %d%s" % (slice_, "+1" if beyond else ""),
                configs=((16, None, False), (16, "1", False), (16, None, True)))
    assert _stats(gpu_ctx)["string_answered"] == 0


@pytest.mark.gpu
def test_string_of_2048_states_is_taken_and_2049_is_not(gpu_ctx, oracle, monkeypatch):
    run_strings(gpu_ctx, oracle, [string([1] * 2047), string([1] * 2048)], ladder_t(1), monkeypatch, "2048 / 2049 states",
                configs=((2, None, False), (2, "0", False)))


@pytest.mark.gpu
def test_begin_end_form_tallies_in_end(gpu_ctx, oracle, monkeypatch):
    """compose_shortest_path_batch_begin resets the counters, _end tallies them: the same values as the one-call form"""
    import rustfst_amd
    for name in ("WFST_STRING_SCALAR", "WFST_STRING_UNPACKED", "WFST_STRING_KERNEL", "WFST_COMPOSE_PATH"):
        monkeypatch.delenv(name, raising=False)
    strs, t = [string([1] * 5), string([1] * 4 + [2]), trim_case(64)[0]], ladder_t(64)
    handles, dt = [to_device(s, gpu_ctx) for s in strs], to_device(t, gpu_ctx)
    to_device(loop_t(6), gpu_ctx).compose(to_device(chain_t(1281, 1), gpu_ctx))
    assert _stats(gpu_ctx)["relaunch_states"] == 1
    job = rustfst_amd.compose_shortest_path_batch_begin(handles, dt, ctx=gpu_ctx)
    st = _stats(gpu_ctx)
    assert {k: st[k] for k in COUNTERS[:9]} == {k: 0 for k in COUNTERS[:9]}  # (the general run is in flight: its caps are known)
    outs, n_arcs = job.finish()
    want = predict_batch(oracle, strs, t)
    assert _stats(gpu_ctx) == want and (want["string_answered"], want["string_handed_back"], want["wave_first"]) == (1, 1, 2)
    for s, o in zip(strs, outs):
        same(o.to_flat(), analyse(oracle, s, t)["path"], "begin / end")
    assert n_arcs == sum(len(analyse(oracle, s, t)["full"]["arcs"]) for s in strs)
