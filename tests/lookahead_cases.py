"""Inputs of tests/test_lookahead_limits.py: pairs (first operand, second operand) that put the look-ahead composition of
compose_lookahead.hip ON one of its limits or one step beyond it, where each lands according to the oracle, and a Python
restatement of the driver's routing that predicts the counters of wfst_ctx_get_lookahead_stats.  No test lives here.

First operands carry output epsilons on the way, so that the look-ahead filter, pushed weights and pushed labels are live.
Second operands are mostly one final state that loops over a set of labels: the composition then has the shape of the first
operand, and its levels can be placed at will."""
import functools

import numpy as np

from oracle.model import to_oracle

from helpers import finals_of, fst

INF = float("inf")
NO_LABEL = 0xFFFFFFFF
# ---- the limits of rustfst_amd/csrc/compose_lookahead.hip and compose_wide.h, restated once
WAVE = 64                       # compose_lookahead.hip:381 items 64 at a time; :417 destinations interned 64 at a time
SWITCH_STATES = 2048            # :47 WIDE_SWITCH_STATES
SWITCH_WIDTH = 256              # :48 WIDE_SWITCH_WIDTH
SWITCH_STATES_ONE = 512         # :49 WIDE_SWITCH_STATES_ONE
SWITCH_WIDTH_ONE = 48           # :50 WIDE_SWITCH_WIDTH_ONE
CAP_S = 2 * SWITCH_STATES + 256  # :674 est_s
CAP_A = 4 * CAP_S               # :675 LaCaps{S, 4 S, pow2(2 S + 128)}
REGROW_S = 16 * SWITCH_STATES   # :727 the first arena of a composition redone under WFST_LOOKAHEAD_PATH=wave, x4 per attempt
KDELTA = 1.0 / 1024.0           # common.h
WIDE_MIN_S = 1 << 18            # compose_wide.h:555 the wide driver's arena begins at a quarter of a million states
WIDE_SHARDS = 64                # compose_wide.h:61 CUR_SHARDS: the arc arena is cut into 64 slices
WIDE_FIRST_BATCH = 4            # compose_wide.h:569 batch_cap: levels queued before the host's first look
COUNTERS = ("items", "items_no_start", "wave_answered", "handed_over_states", "handed_over_width", "overflow_arcs",
            "overflow_states", "wide_items", "wave_regrows", "wide_grows", "wide_hinted", "hint_fallbacks", "one_limits")
ZERO = dict.fromkeys(COUNTERS, 0)
PATHS = (None, "wave", "wide")


def pow2(x):
    p = 1
    while p < x:
        p <<= 1
    return p


CAP_H = pow2(2 * CAP_S + 128)


# ================================================================ second operands
def loop2(labels, weights=None, final=0.0):
    """one state (final unless final = INF) with an arc l:l back to it for every label"""
    labels = sorted(labels)
    rows = [[(l, l, 0.0 if weights is None else weights[k], 0) for k, l in enumerate(labels)]]
    return fst(rows, [final])


# ================================================================ first operands
def chain1(n):
    """n states in a row; every second arc is x:eps; labels cycle over 1..5, weights over the 1/4 grid"""
    rows = [[(1 + i % 3, 0 if i % 2 else 1 + i % 5, (i % 4) / 4.0, i + 1)] for i in range(n - 1)] + [[]]
    return fst(rows, finals_of(n, {n - 1: 0.25}))


CHAIN_LABELS = (1, 2, 3, 4, 5)


def star1(leaves, base=100, tail=True):
    """state 0 fans out to `leaves` states (labels base ..., every third arc x:eps), which all go on to ONE state through an
    x:eps arc, and that one to a final state: levels add leaves, 1 and 1 states.  Without the tail the leaves are final and
    the composition has leaves + 1 states."""
    n = leaves + 3
    rows = [[(7, 0 if j % 3 == 2 else base + j, (j % 4) / 4.0, 1 + j) for j in range(leaves)]]
    rows[0].sort(key=lambda a: a[1])
    if not tail:
        return fst(rows + [[] for _ in range(leaves)], finals_of(leaves + 1, {1 + j: (j % 3) / 4.0 for j in range(leaves)}))
    rows += [[(8, 0, 0.5, leaves + 1)] for _ in range(leaves)]
    rows += [[(9, 50, 0.25, leaves + 2)], []]
    return fst(rows, finals_of(n, {leaves + 2: 0.0}))


def star_labels(leaves, base=100):
    return [base + j for j in range(leaves) if j % 3 != 2] + [50]


def wide_chain1(leaves, length):
    """beyond both limits: the star's fan, then a chain of `length` states behind it"""
    n = leaves + 1 + length
    rows = [[(7, 0 if j % 3 == 2 else 100 + j, (j % 4) / 4.0, 1 + j) for j in range(leaves)]]
    rows[0].sort(key=lambda a: a[1])
    rows += [[(8, 0, 0.5, leaves + 1)] for _ in range(leaves)]
    for i in range(length - 1):
        rows.append([(1 + i % 3, 0 if i % 2 else 1 + i % 5, (i % 4) / 4.0, leaves + 2 + i)])
    rows.append([])
    return fst(rows, finals_of(n, {n - 1: 0.0}))


def parallel1(links, arcs=512, base=1000, one_more=False):
    """links + 1 states in a row; `arcs` parallel arcs (distinct labels, one destination) from each to the next, one of them
    x:eps: a composition of width 1 that emits links * arcs arcs — and with one_more one arc more, from the last link"""
    rows = []
    for i in range(links):
        row = [(1 + j % 3, base + j, ((i + j) % 8) / 8.0, i + 1) for j in range(arcs - 1)] + [(5, 0, 0.125, i + 1)]
        if one_more and i == links - 1:
            row.append((2, base + arcs - 1, 0.25, i + 1))
        row.sort(key=lambda a: a[1])
        rows.append(row)
    rows.append([])
    return fst(rows, finals_of(links + 1, {links: 0.0}))


def parallel_labels(arcs=512, base=1000):
    return [base + j for j in range(arcs - 1)]


# ---------------------------------------------------------------- items of one composed state
ITEM_ARCS = (62, 63, 64, 65, 127, 128)
ITEM_SIDES = ("first", "second", "tie")
FILL = 9000  # labels the first operand never emits


def items_pair(n_it, side, multi_item=None):
    """The start pair: the iterated side has n_it arcs (items = n_it + 1: 63 arcs fill one chunk of 64 items, 64 start a
    second).  side: 'first' = the first operand has fewer arcs (n_it against n_it + 7) and iterates, 'second' = the second
    one has fewer, 'tie' = both have n_it and the first iterates.  Both rows are sorted and duplicate-free, so every item
    emits at most one arc — unless multi_item = j: item j (arc j - 1 of the iterated row) then meets three arcs of the other
    side.  The first operand's row holds x:eps arcs (one when the second operand iterates: item 0, the loop item, collects
    them).  Every arc leads to one of three final states."""
    n1 = n_it + 7 if side == "second" else n_it
    n2 = n_it + 7 if side == "first" else n_it
    eps1 = [0] if side == "second" else list(range(0, n1, 10))
    out1 = [0 if j in eps1 else 100 + j for j in range(n1)]
    lab1 = [l for l in out1 if l]
    if side == "second":
        in2 = lab1[:n2]
    else:
        in2 = lab1 + [FILL + k for k in range(n2 - len(lab1))]
    if multi_item is not None:
        if side == "second":  # three arcs of the first operand emit the label of the second operand's arc multi_item - 1
            l = sorted(in2)[multi_item - 1]
            spare = [j for j in range(n1) if out1[j] not in in2 and out1[j]][:2]
            for j in spare:
                out1[j] = l
        else:  # three arcs of the second operand read the label of the first operand's arc multi_item - 1
            l = sorted(out1)[multi_item - 1]
            assert l != 0
            k = [i for i, x in enumerate(in2) if x >= FILL][:2]
            for i in k:
                in2[i] = l
    rows1 = [sorted([(1 + j % 3, out1[j], (j % 5) / 4.0, 1 + j % 3) for j in range(n1)], key=lambda a: a[1]), [], [], []]
    f1 = fst(rows1, [INF, 0.0, 0.25, 0.5])
    rows2 = [sorted([(l, 300 + k, (k % 3) / 8.0, 0) for k, l in enumerate(in2)], key=lambda a: a[0])]
    return f1, fst(rows2, [0.125])


def item_counts(an, q=0):
    """arcs each item of composed state q emits, from the relabelled rows (compose_lookahead.hip eval_item :282-326 where no
    label is owed and every pair passes the filter): item 0 meets the other side's epsilons, an epsilon of the iterated side
    meets the epsilon loop, a label meets the arcs that carry it"""
    s1, s2 = int(an["tuples"][q][0]), int(an["tuples"][q][1])
    assert an["tuples"][q][4] == NO_LABEL
    row1 = an["r1"]["arcs"]["olabel"][an["r1"]["offsets"][s1]:an["r1"]["offsets"][s1 + 1]].astype(np.int64)
    row2 = an["r2"]["arcs"]["ilabel"][an["r2"]["offsets"][s2]:an["r2"]["offsets"][s2 + 1]].astype(np.int64)
    it, se = (row1, row2) if len(row1) <= len(row2) else (row2, row1)
    return [int((se == 0).sum())] + [1 if l == 0 else int((se == l).sum()) for l in it]


# ---------------------------------------------------------------- one level's destinations, 64 at a time
INTERN_ARCS = (63, 64, 65, 128, 129)
INTERN_FOLDS = ("one", "distinct", "border", "earlier")


def intern_pair(n_arcs, fold):
    """state 0 reaches a hub through an x:eps arc (the look-ahead pushes the hub's best weight, 0), and the hub's n_arcs arcs
    are ONE level's emission, in label order.  fold: 'one' = one destination; 'distinct' = n_arcs destinations; 'border' =
    distinct, but arcs 63 and 64 — the last of chunk 0 and the first of chunk 1 — name the same state; 'earlier' = distinct,
    but arcs 5, 63 and 64 go back to the hub, whose tuple was interned a level before."""
    def dest(j):
        if fold == "one":
            return 2
        if fold == "border" and j == 64:
            return 2 + 63
        if fold == "earlier" and j in (5, 63, 64):
            return 1
        return 2 + j
    hub = [(1 + j % 3, 100 + j, (j % 4) / 4.0, dest(j)) for j in range(n_arcs)]
    n = 2 + n_arcs
    rows = [[(4, 0, 0.5, 1)], hub] + [[] for _ in range(n_arcs)]
    fin = {2 + j: (j % 3) / 4.0 for j in range(n_arcs)}
    return fst(rows, finals_of(n, fin)), loop2([100 + j for j in range(n_arcs)] + [FILL, FILL + 1], final=0.0)


TWINS = ("weight", "label", "alt")


def twin_pair(kind):
    """Two arcs of one chunk reach the same pair of states under different filter states: the probe finds the first word of
    its key in the table, not the second, and moves on.  The hub has 70 arcs; arc 10 (x:eps) and arc 20 (x:y) both lead to
    state T.  The x:y arc arrives under the start filter state.  The x:eps arc arrives with: 'weight' = a pushed weight (T
    reads two labels of the second operand, the cheaper at 1/2); 'label' = a pushed label (T reads one label and is not
    final: the prefix); 'alt' = AltSequence state 1 (the second operand has an input epsilon, T is final and reads nothing)."""
    n_arcs, t = 70, 2
    hub = [(1 + j % 3, 0 if j == 10 else 100 + j, (j % 4) / 4.0, t if j in (10, 20) else 3 + j) for j in range(n_arcs)]
    hub.sort(key=lambda a: a[1])
    rows = [[(4, 90, 0.5, 1)], hub, []] + [[] for _ in range(n_arcs)]
    fin = {3 + j: (j % 3) / 4.0 for j in range(n_arcs)}
    labels = [90] + [100 + j for j in range(n_arcs) if j != 10]
    weights = {}
    if kind == "weight":
        rows[t] = [(1, 400, 0.0, 3), (2, 401, 0.0, 4)]
        labels += [400, 401]
        weights = {400: 0.5, 401: 0.75}
    elif kind == "label":
        rows[t] = [(1, 400, 0.0, 3)]
        labels += [400]
    else:
        fin[t] = 0.0
    f1 = fst(rows, finals_of(3 + n_arcs, fin))
    row2 = [(l, l, weights.get(l, 0.0), 0) for l in sorted(labels)]
    if kind == "alt":
        row2 = [(0, 77, 0.25, 1)] + row2
        return f1, fst([row2, []], [0.0, 0.0])
    return f1, fst([row2], [0.0])


# ---------------------------------------------------------------- lookahead_fst (:140-192): both ways to find what is reachable
BRANCH_K = 6
BRANCH_LABELS = [10 + i for i in range(2 * BRANCH_K)]
BRANCH_EVEN, BRANCH_ODD = BRANCH_LABELS[0::2], BRANCH_LABELS[1::2]


@functools.lru_cache(maxsize=None)
def branch1():
    """State 0 reaches P, A, B and A2 through x:eps arcs.  P emits 2 K labels; A emits every other one of them, B the rest: the
    relabelling numbers them in P's order, so A's interval set has K disjoint entries and so has B's.  A2 is A with an x:eps
    arc to the final state on top: the final label is reachable from it."""
    sink = 5
    rows = [[(1, 0, 0.0, 1), (2, 0, 0.25, 2), (3, 0, 0.5, 3), (4, 0, 0.75, 4)],
            [(1, l, 0.0, sink) for l in BRANCH_LABELS],
            [(1, l, (i % 3) / 4.0, sink) for i, l in enumerate(BRANCH_EVEN)],
            [(1, l, 0.25, sink) for l in BRANCH_ODD],
            [(2, 0, 0.125, sink)] + [(1, l, (i % 2) / 4.0, sink) for i, l in enumerate(BRANCH_EVEN)],
            []]
    return fst(rows, finals_of(6, {sink: 0.0}))


def branch2(labels, final, weights=None):
    """a start state with one arc per entry of `labels` (repeats allowed) to a final state without arcs"""
    weights = weights or [0.5 + k / 8.0 for k in range(len(labels))]
    row = sorted([(l, 500 + k, weights[k], 1) for k, l in enumerate(labels)], key=lambda a: a[0])
    return fst([row, []], [0.0 if final else INF, 0.25])


E, O = BRANCH_EVEN, BRANCH_ODD
BRANCH_SECONDS = {
    "n0": ([], False), "n0_final": ([], True),
    "n1_prefix": ([E[2]], False),                  # exactly one reachable arc, no reachable final: prefix, pushed label
    "n1_final": ([E[2]], True),                    # one reachable arc plus a reachable final (from A2)
    "n1_other": ([O[1]], False),                   # reachable from B and P only
    "n2": ([E[0], E[5]], False),                   # 2 n < K: fst2's arcs are scanned
    "n2_same_label": ([E[3], E[3]], False),        # two reachable arcs with the same label
    "n2_same_label_final": ([E[3], E[3]], True),
    "n3": ([E[1], O[2], E[4]], False),             # 2 n == K: the intervals are walked
    "n3_final": ([O[0], E[4], E[5]], True),
    "n4": ([E[0], O[0], E[1], O[5]], False),       # 2 n > K
    "n12": (BRANCH_LABELS, True),
    "n2_unread": ([FILL, FILL + 1], False),        # nothing reachable: every x:eps arc is refused
}


def branches_taken(an, intervals):
    """(arcs scanned, intervals walked): how often each branch of lookahead_fst (:150) runs in this composition — for every
    composed state that owes no label, every x:eps arc of the first operand's state looks ahead from its destination at the
    second operand's state (la_filter :203-228; the second operands here have no input epsilons, so AltSequence refuses
    nothing)"""
    r1, r2 = an["r1"], an["r2"]
    assert not (r2["arcs"]["ilabel"] == 0).any()
    scan = walk = 0
    for s1, s2, _, _, flabel in an["tuples"]:
        if flabel != NO_LABEL:
            continue
        n = int(r2["offsets"][s2 + 1] - r2["offsets"][s2])
        for a in r1["arcs"][r1["offsets"][s1]:r1["offsets"][s1 + 1]]:
            if a["olabel"] == 0:
                if 2 * n < len(intervals[int(a["nextstate"])]):
                    scan += 1
                else:
                    walk += 1
    return scan, walk


# ---------------------------------------------------------------- the pushed weight's quantization (la_filter :233)
@functools.lru_cache(maxsize=None)
def quant1():
    """0 -x:eps-> 1, which reads two labels on its way to the final state 2: the look-ahead from state 1 sees two arcs of the
    second operand (no prefix) and pushes the smaller weight, quantized to KDELTA"""
    return fst([[(1, 0, 0.25, 1)], [(2, 10, 0.5, 2), (3, 11, 0.125, 2)], []], [INF, INF, 0.0])


def quant2(w, other=None):
    """the two arcs the look-ahead sees: weight w and a larger one; then a final state"""
    other = np.float32(w) + np.float32(1.0) if other is None else other
    return fst([[(10, 20, w, 1), (11, 21, other, 1)], []], [INF, 0.5])


def f32(x):
    return float(np.float32(x))


def quant_weights():
    """lweight exactly on (k + 1/2) KDELTA and one ulp either side (k = 3, 700 and -5: all exact in binary32), negative weights,
    2^20 and the two zeros"""
    out = {}
    for k in (3, 700, -5):
        mid = np.float32((k + 0.5) * KDELTA)
        assert float(mid) == (k + 0.5) * KDELTA
        out["half_%d" % k] = float(mid)
        out["half_%d_below" % k] = float(np.nextafter(mid, np.float32(-np.inf)))
        out["half_%d_above" % k] = float(np.nextafter(mid, np.float32(np.inf)))
    out.update(negative=-1.25, negative_small=-3 * KDELTA / 4, big=float(2 ** 20), big_half=float(2 ** 20) + 0.5,
               zero=0.0, minus_zero=-0.0)
    return out


def quantize(w):
    """semiring.rs:132-145 on a finite binary32 weight: floor(w / delta + 1/2) * delta, every step in binary32"""
    w, d = np.float32(w), np.float32(KDELTA)
    return np.float32(np.floor(np.float32(w / d) + np.float32(0.5))) * d


# ---------------------------------------------------------------- one first operand, many second operands
HUB_CHAIN, HUB_LINKS, HUB_LEAVES = 2060, 110, 300
HUB_C, HUB_P, HUB_T = 1, 2, 50


@functools.lru_cache(maxsize=None)
def hub1():
    """One first operand whose second operand picks the shape.  The start state has an arc C:C into a chain of HUB_CHAIN states
    (every second arc x:eps, every other arc a label of its own: a loop over the first k of them follows the chain that far),
    an arc P:P into HUB_LINKS links of 512 parallel arcs, and HUB_LEAVES arcs with labels of their own to leaves that go on
    (x:eps) to one state, which reads HUB_T on its way to the final state: a loop over k leaf labels and HUB_T gives levels
    of k, 1 and 1 new states."""
    rows = [[(1, HUB_C, 0.25, 1), (2, HUB_P, 0.5, 1 + HUB_CHAIN)] + [(3, l, (j % 4) / 4.0, 0) for j, l in enumerate(hub_leaf_labels(HUB_LEAVES))]]
    for i in range(HUB_CHAIN - 1):
        rows.append([(1 + i % 3, 0 if i % 2 else hub_chain_label(i), (i % 4) / 4.0, 2 + i)])
    rows.append([])
    p0 = len(rows)
    assert p0 == 1 + HUB_CHAIN
    labs = parallel_labels()
    for i in range(HUB_LINKS):
        row = [(1 + j % 3, l, ((i + j) % 8) / 8.0, p0 + i + 1) for j, l in enumerate(labs)] + [(5, 0, 0.125, p0 + i + 1)]
        rows.append(sorted(row, key=lambda a: a[1]))
    rows.append([])
    l0 = len(rows)
    t1 = l0 + HUB_LEAVES
    rows[0] = rows[0][:2] + [(il, ol, w, l0 + j) for j, (il, ol, w, _) in enumerate(rows[0][2:])]
    rows += [[(8, 0, 0.5, t1)] for _ in range(HUB_LEAVES)]
    rows += [[(9, HUB_T, 0.25, t1 + 1)], []]
    rows[0].sort(key=lambda a: a[1])
    return fst(rows, finals_of(len(rows), {HUB_CHAIN: 0.25, p0 + HUB_LINKS: 0.0, t1 + 1: 0.0}))


def hub_chain_label(i):
    return 20000 + i


def hub_leaf_labels(k):
    return [100 + j for j in range(k)]


def hub_chain2(states):
    """follows the chain until the composition has `states` states (odd: the start pair, then the chain's states two at a
    time — an x:eps arc is only taken when the label behind it can be read)"""
    labels = [HUB_C] + [hub_chain_label(i) for i in range(0, states - 2, 2)]
    return loop2(labels)


def hub_star2(leaves, pad=0):
    return loop2(hub_leaf_labels(leaves) + [HUB_T] + [FILL + k for k in range(pad)])


def hub_parallel2():
    return loop2([HUB_P] + parallel_labels())


# ================================================================ where a pair lands
_AN = {}


def analyse(oracle, f1, f2):
    """The oracle's look-ahead composition of the pair with its BFS levels.  Its ids are first-touch BFS order, so a level is a
    contiguous id range: levels[k] = (lo, hi, arcs emitted, new states).  tuples[q] = (s1, s2, AltSequence state, bits of the
    pushed weight, pushed label); r1, r2 = the relabelled operands as the kernel sees them; items[q] = arcs on the iterated
    side + 1 (compose_lookahead.hip:272 / :380: the side with fewer arcs iterates, the first on a tie)."""
    key = (id(f1), id(f2))
    if key not in _AN:
        if f2["start"] is None:  # (helpers.empty_flat(): an operand without a start state)
            out = to_oracle(oracle, f1).compose_lookahead(oracle.OracleFst())
            _AN[key] = dict(f1=f1, f2=f2, flat=out.to_flat(), levels=[], n_states=0, n_arcs=0, start=False)
            return _AN[key]
        out, r1, r2 = to_oracle(oracle, f1).compose_lookahead(to_oracle(oracle, f2), want_relabeled=True)
        tuples = oracle.OracleFst.last_lookahead_tuple_list()
        cf, r1, r2 = out.to_flat(), r1.to_flat(), r2.to_flat()
        n, off, nx = cf["n_states"], cf["offsets"].astype(np.int64), cf["arcs"]["nextstate"].astype(np.int64)
        assert len(tuples) == n
        if len(nx):  # first-touch order: an arc names a state seen before, or the next new one
            seen = np.maximum.accumulate(np.concatenate([[0], nx]))
            assert np.all(np.diff(seen) <= 1), "the oracle's ids are not first-touch order"
        levels, lo, hi = [], 0, min(n, 1)
        while lo < hi:
            e0, e1 = int(off[lo]), int(off[hi])
            new_hi = max(hi, int(nx[e0:e1].max()) + 1 if e1 > e0 else 0)
            levels.append((lo, hi, e1 - e0, new_hi - hi))
            lo, hi = hi, new_hi
        assert hi == n
        d1, d2 = np.diff(r1["offsets"].astype(np.int64)), np.diff(r2["offsets"].astype(np.int64))
        n1, n2 = d1[tuples[:, 0]], d2[tuples[:, 1]]
        _AN[key] = dict(f1=f1, f2=f2, flat=cf, r1=r1, r2=r2, tuples=tuples, levels=levels, n_states=n, n_arcs=len(nx), start=True,
                        n1=n1, n2=n2, first_iterates=n1 <= n2, items=np.minimum(n1, n2) + 1, degree=np.diff(off))
    return _AN[key]


# ================================================================ the routing, restated
def wave_outcome(an, switch_states, switch_width, cap_s=CAP_S, cap_a=CAP_A):
    """compose_lookahead_kernel on one composition, level by level (:369-485): 'ok', 'overflow_arcs' (:395 a chunk's arcs pass A),
    'overflow_states' (:454 a level's new states pass S), 'states' / 'width' (:480 LA_SWITCH_WIDE after a level that found new
    states, told apart by n_states as the host does).  switch_states None: pinned to the wave, it never switches."""
    arcs = 0
    for lo, hi, emitted, new in an["levels"]:
        arcs += emitted
        if arcs > cap_a:
            return "overflow_arcs"
        if hi + new > cap_s:
            return "overflow_states"
        if switch_states is not None and new > 0 and (hi + new > switch_states or new > switch_width):
            return "states" if hi + new > switch_states else "width"
    return "ok"


def wide_group(f1, f2):
    """lanes per composed state in the wide kernels (compose_wide.h:691, items_hint = 1 + the smaller mean out-degree)"""
    d = [len(f["arcs"]) / max(f["n_states"], 1) for f in (f1, f2)]
    hint = 1.0 + min(d)
    return 2 if hint <= 2.5 else 4 if hint <= 4.0 else 8 if hint <= 8.0 else 16 if hint <= 16.0 else 64


def wide_grows(an, est_s, est_a):
    """Growths of the wide driver's arena, from a restatement of run_wide_g's host loop (compose_wide.h:545-666).  The arc arena
    is cut into 64 slices; the states of a level go to waves 64 / G at a time in id order, and wave w reserves its states'
    arcs in slice w % 64 (:203, :243), whether they fit or not.  The host queues a batch of levels per look at the control
    block; a level that did not fit grows the arena (x4) and is emitted again, and after a look the arena also grows AHEAD of a
    level that the foresight of :638-664 expects not to fit.  The grid has at least 256 waves (:612), so a level of at most
    256 waves' states lands as described; a wider one is answered only where everything is queued before the first look and
    fits a single slice.  Anything else: None (no case may need it)."""
    s = max(est_s, WIDE_MIN_S)
    a = max(est_a, 4 * s)
    levels, degree = an["levels"], an["degree"]
    spw = WAVE // wide_group(an["r1"], an["r2"])
    if len(levels) <= WIDE_FIRST_BATCH and an["n_arcs"] <= a // WIDE_SHARDS and an["n_states"] <= s:
        return 0
    if any(hi - lo > 256 * spw for lo, hi, _, _ in levels):
        return None
    per, cur, lo_part, k, batch_cap, grows, aps, w_prev = a // WIDE_SHARDS, [0] * WIDE_SHARDS, 0, 0, WIDE_FIRST_BATCH, 0, 4.0, 0

    def grow(lo):
        nonlocal s, a, per, cur, lo_part, grows
        grows += 1
        assert grows <= 24
        g = 2 if s >= (1 << 20) else 4
        a_old = a
        s, a = g * s, g * a
        per, cur, lo_part = (a - a_old) // WIDE_SHARDS, [0] * WIDE_SHARDS, lo

    while True:
        lo, hi = (levels[k][0], levels[k][1]) if k < len(levels) else (an["n_states"],) * 2
        width = hi - lo
        fits = True
        for _ in range(min(batch_cap, 8 if width < 8192 else 4)):
            if k >= len(levels):
                break
            l0, h0, _, new = levels[k]
            if h0 + new > s:
                fits = False
                break
            for r in range(0, h0 - l0, spw):
                cur[(r // spw) % WIDE_SHARDS] += int(degree[l0 + r:min(l0 + r + spw, h0)].sum())
            if max(cur) > per:
                fits = False
                break
            w_prev = h0 - l0
            k += 1
        lo, hi = (levels[k][0], levels[k][1]) if k < len(levels) else (an["n_states"],) * 2
        if not fits:
            grow(lo)
            continue
        if k >= len(levels):
            return grows
        if lo > lo_part:
            aps = max(1.0, sum(cur) / (lo - lo_part))
        r = min(8.0, max(1.0, (hi - lo) / w_prev)) if w_prev else 3.0
        slack = float(per - max(cur))
        while True:
            states, wl, room, n = float(hi), float(hi - lo), slack, 0
            while n < 8:
                arcs_shard, new_states = aps * wl / WIDE_SHARDS, min(1.25 * r, aps) * wl
                if states + new_states > s or 1.5 * arcs_shard + 64.0 > room:
                    break
                states += new_states
                room -= arcs_shard
                wl *= r
                n += 1
            batch_cap = n
            if batch_cap:
                break
            a_old = a
            grow(lo)
            slack = float((a - a_old) // WIDE_SHARDS)


class Handle:
    """What a look-ahead handle remembers between calls (compose_lookahead.hip:587-621: the last wide result sizes the next wide
    arena when the second operands' arc counts are within a factor of two), and with it the prediction of a call's counters."""

    def __init__(self, f1):
        self.f1 = f1
        self.last = None  # (states, arcs, arcs of the second operand) of the last wide run

    def _wide(self, an, p):
        f1, f2 = self.f1, an["f2"]
        ws = 8 * max(min(f1["n_states"], f2["n_states"]), 4096)  # :758
        est_s, est_a = ws, 4 * ws
        if self.last is not None:
            ls, lw, li = self.last
            n_in = len(f2["arcs"])
            if ls != 0 and n_in <= 2 * li + 16 and li <= 2 * n_in + 16:
                est_s, est_a = max(est_s, ls + ls // 8 + 1024), max(est_a, lw + lw // 4 + 65536)
        p["wide_items"] += 1
        p["wide_hinted"] += int((est_s, est_a) != (ws, 4 * ws))
        g = wide_grows(an, est_s, est_a)
        assert g is not None, "no restatement of the wide driver's growth for this shape"
        p["wide_grows"] += g
        self.last = (an["n_states"], an["n_arcs"], len(f2["arcs"]))

    def predict(self, ans, path=None):
        """the counters of one call whose items are `ans` (analyse() dicts), under WFST_LOOKAHEAD_PATH=path"""
        p = dict(ZERO, items=len(ans))
        todo = [an for an in ans if an["start"]]
        p["items_no_start"] = len(ans) - len(todo)
        m = len(todo)
        if path == "wide" or not m:
            for an in todo:
                self._wide(an, p)
            return p
        one = m == 1
        p["one_limits"] = int(one and path != "wave")
        limits = (None, None) if path == "wave" else ((SWITCH_STATES_ONE, SWITCH_WIDTH_ONE) if one else (SWITCH_STATES, SWITCH_WIDTH))
        redo = []
        for an in todo:
            what = wave_outcome(an, *limits)
            if what == "ok":
                p["wave_answered"] += 1
                continue
            p[{"states": "handed_over_states", "width": "handed_over_width"}.get(what, what)] += 1
            redo.append(an)
        for an in redo:
            if path == "wave":
                s = REGROW_S
                while True:
                    p["wave_regrows"] += 1
                    if wave_outcome(an, None, None, s, 4 * s) == "ok":
                        break
                    s *= 4
                p["wave_answered"] += 1
            else:
                self._wide(an, p)
        return p
