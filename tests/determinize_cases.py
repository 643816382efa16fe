"""Input families of determinize that more than one test module uses."""
import collections
import functools

import numpy as np

from rustfst_amd._lib import TR_DTYPE

from oracle import model
from oracle.model import ACCEPTOR, F32, INF, KDELTA
import inputs
from helpers import random_fst_flat


def random_acceptor(rng, n, fanout, sigma, **kw):
    f = random_fst_flat(rng, n, fanout, sigma, **kw)
    f["arcs"]["olabel"] = f["arcs"]["ilabel"]
    f["props"] |= ACCEPTOR
    return f


def f32_weights(rng, f):
    f["arcs"]["weight"] = rng.random(len(f["arcs"])).astype(np.float32) * np.float32(3.0)
    fin = f["finals"]
    f["finals"] = np.where(np.isfinite(fin), rng.random(len(fin)).astype(np.float32), np.inf).astype(np.float32)
    return f


def parity_inputs():
    """(name, flat, delta) — acyclic DAGs with small alphabets, epsilon labels, cyclic unweighted, integer and arbitrary
    f32 weights, non-default deltas"""
    rng = np.random.default_rng(1515)
    out = []
    for k in range(6):
        n = int(rng.integers(2, 40))
        out.append((f"dag{k}", random_acceptor(rng, n, 4, 2 + k % 2, acyclic=True), KDELTA))
    for k in range(3):
        out.append((f"eps{k}", random_acceptor(rng, 30, 3, 3, p_eps_i=0.3, acyclic=True), KDELTA))
    for k in range(4):
        out.append((f"cyclic_unweighted{k}", random_acceptor(rng, 25 + 10 * k, 3, 3, max_w=1, p_eps_i=0.1), KDELTA))
    for k in range(3):
        out.append((f"int{k}", random_acceptor(rng, 40, 4, 3, weight_grid=1, max_w=5, acyclic=True), KDELTA))
    for k in range(3):
        out.append((f"f32_{k}", f32_weights(rng, random_acceptor(rng, 40, 4, 3, acyclic=True)), KDELTA))
    for k, d in enumerate((0.5, 0.1, 1.0 / 3.0)):
        out.append((f"delta{k}", random_acceptor(rng, 40, 4, 3, acyclic=True), d))
    out.append(("empty", dict(n_states=0, start=None, offsets=np.zeros(1, np.uint32), arcs=np.zeros(0, TR_DTYPE),
                              finals=np.zeros(0, np.float32), props=ACCEPTOR), KDELTA))
    return out


def collision_level(S=64, M=200, seed=7):
    """a start state with S arcs (distinct labels) into states 1..S; each of those has M labels, every label with one
    arc into A (weight 0) and one into B (weight k * KDELTA, k random in 0..12): the second level holds S * M candidates
    with the same state set {A, B} and weights a KDELTA apart"""
    rng = np.random.default_rng(seed)
    A, B, F = S + 1, S + 2, S + 3
    rows = [[(j + 1, j + 1, 0.0, j + 1) for j in range(S)]]
    for s in range(S):
        r = []
        for i in range(M):
            r += [(i + 1, i + 1, 0.0, A), (i + 1, i + 1, float(rng.integers(0, 13)) * KDELTA, B)]
        rows.append(r)
    rows += [[(1, 1, 0.0, F)], [(1, 1, 0.0, F)], []]
    arcs = np.array([x for r in rows for x in r], dtype=TR_DTYPE)
    offsets = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint32)
    fin = np.full(S + 4, np.inf, np.float32)
    fin[F] = 0.0
    return dict(n_states=S + 4, start=0, offsets=offsets, arcs=arcs, finals=fin, props=ACCEPTOR)


def det_levels(flat, delta=KDELTA, reverse_ties=False):
    """test_determinize_batch.determinize_with_distance_ref (the same construction, statement by statement) that returns
    dict(fst, tuples, level_of, figs, reach): figs[i] = (states, raw candidates, new states, new elements, valid arcs, m) of
    breadth-first level i, m = the most new states of the level that share one state-id sequence; level_of[s] = the level
    state s belongs to (it was created while level_of[s] - 1 was expanded); reach[i] = the levels of the states that
    candidates of level i found among the states numbered before the level began (ph_lookup's C_EXIST).
    reverse_ties: candidates of equal (label, dest) in reverse arrival order (what a sort that is not stable may do)."""
    assert flat["props"] & ACCEPTOR and flat["start"] is not None
    off, arcs, fin = flat["offsets"], flat["arcs"], flat["finals"]
    tuples = [((int(flat["start"]), F32(0.0)),)]
    by_states = {(int(flat["start"]),): [0]}
    level_of = [0]
    rows, finals, offsets = [], [], [0]
    figs, reach = [], []
    s, lo, hi = 0, 0, 1
    n_raw = n_valid = 0
    found = set()
    while s < len(tuples):
        cand = [(int(a["ilabel"]), int(a["nextstate"]), model.times(w, F32(a["weight"])))
                for q, w in tuples[s] for a in arcs[off[q]:off[q + 1]]]
        assert not any(c[2] == 0 and np.signbit(c[2]) for c in cand), "a raw candidate of weight -0.0"
        n_raw += len(cand)
        if reverse_ties:
            cand.reverse()
        cand.sort(key=lambda c: (c[0], c[1]))  # stable
        fw = INF
        for q, w in tuples[s]:
            fw = model.plus(fw, model.times(w, F32(fin[q])))
        i = 0
        while i < len(cand):
            j, weight = i, INF
            while j < len(cand) and cand[j][0] == cand[i][0]:
                weight = model.plus(weight, cand[j][2])
                j += 1
            merged = []
            for _, q, w in cand[i:j]:
                if merged and merged[-1][0] == q:
                    merged[-1][1] = model.plus(merged[-1][1], w)
                else:
                    merged.append([q, w])
            t = tuple((q, model.quantize(F32(w - weight), delta)) for q, w in merged)
            ids = by_states.setdefault(tuple(q for q, _ in t), [])
            dest = next((k for k in ids if all(model.approx_eq(w, v) for (_, w), (_, v) in zip(t, tuples[k]))), None)
            if dest is None:
                dest = len(tuples)
                ids.append(dest)
                tuples.append(t)
                level_of.append(len(figs) + 1)
            elif dest < hi:
                found.add(level_of[dest])
            rows.append((cand[i][0], cand[i][0], weight, dest))
            n_valid += 1
            i = j
        offsets.append(len(rows))
        finals.append(fw)
        s += 1
        if s == hi:  # the states created while this level was expanded are the next one
            new = tuples[hi:]
            share = collections.Counter(tuple(q for q, _ in t) for t in new)
            figs.append((hi - lo, n_raw, len(new), sum(len(t) for t in new), n_valid, max(share.values(), default=0)))
            reach.append(found)
            lo, hi, n_raw, n_valid, found = hi, len(tuples), 0, 0, set()
    a = np.zeros(len(rows), TR_DTYPE)
    for k, r in enumerate(rows):
        a[k] = r
    fst = dict(n_states=len(tuples), start=0, offsets=np.array(offsets, np.uint32), arcs=a,
               finals=np.array(finals, np.float32), props=model.determinize_props(flat["props"], True))
    return dict(fst=fst, tuples=tuples, level_of=level_of, figs=figs, reach=reach)


def flat_of_rows(rows, fin):
    arcs = np.array([x for r in rows for x in r], dtype=TR_DTYPE) if any(rows) else np.zeros(0, TR_DTYPE)
    offsets = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint32)
    return dict(n_states=len(rows), start=0, offsets=offsets, arcs=arcs, finals=np.asarray(fin, np.float32), props=ACCEPTOR)


def layered(spec, back=None, weighted=True):
    """A layered acceptor whose subsets are single states, so its level figures are known by construction.  spec[i] =
    (valid, raw, new) of level i: its states (one at level 0, else new of the level before) carry `valid` arcs with
    distinct labels per state, dealt round robin; arc j of the level goes to state j % new of the next level; raw - valid
    more copies of arc 0 (same label and destination, appended out of label order: duplicates that merge) bring the raw
    candidates to `raw`.  back[i] = [(level j <= i, n), ...] adds n arcs from level i to states of level j (labels from
    1000): states that exist when the level is expanded.  Returns (flat, figs)."""
    back = back or {}
    width = [1] + [new for _, _, new in spec]
    assert width[-1] == 0 and all(v >= new and raw >= v and (v > 0 or raw == 0) for v, raw, new in spec)
    base = np.concatenate([[0], np.cumsum(width)]).astype(np.int64)
    rows = [[] for _ in range(int(base[-1]))]
    figs = []
    for i, (valid, raw, new) in enumerate(spec):
        w = width[i]
        for j in range(valid):
            wt = ((7 * j + i) % 5) * 0.25 if weighted else 0.0
            rows[base[i] + j % w].append((j // w + 1, j // w + 1, wt, int(base[i + 1] + j % new)))
        extra = 0
        for j, n in back.get(i, ()):
            for t in range(n):
                rows[base[i] + t % w].append((1000 + 100 * j + t // w, 1000 + 100 * j + t // w, 0.0, int(base[j] + 3 * t % width[j])))
            extra += n
        if raw > valid:
            first = rows[base[i]][0]
            rows[base[i]] += [(first[0], first[1], first[2] + 0.5, first[3])] * (raw - valid)
        figs.append((w, raw + extra, new, new, valid + extra, 1 if new else 0))
    fin = np.full(len(rows), np.inf, np.float32)
    fin[::3] = 0.5 if weighted else 0.0
    fin[base[len(spec) - 1]:] = 0.0
    return flat_of_rows(rows, fin), figs


def pair_states(rows, src, label, a, b, k):
    """two arcs `label` of src, into a (weight 0) and b (weight k * KDELTA): the subset {(a, 0), (b, k * KDELTA)}"""
    rows[src] += [(label, label, 0.0, a), (label, label, k * KDELTA, b)]


def lowest_id_chain(same_level):
    """Subsets over {A, B} with residuals 3 and 5 KDELTA (no match: 2 KDELTA apart), created in different levels by s1 and
    s2 — or, same_level, both by s1 under labels 1 and 3 — and later a candidate with 4 KDELTA that approx-matches both
    (k15_determinize.json non_transitive_3_4_5): it must take the older, lower id."""
    s0, s1, s2, s3, A, B, F = range(7)
    rows = [[] for _ in range(7)]
    rows[s0].append((2, 2, 0.0, s1))
    pair_states(rows, s1, 1, A, B, 3)
    rows[s1].append((2, 2, 0.0, s2))
    if same_level:
        pair_states(rows, s1, 3, A, B, 5)
        pair_states(rows, s2, 1, A, B, 4)
    else:
        pair_states(rows, s2, 1, A, B, 5)
        rows[s2].append((2, 2, 0.0, s3))
        pair_states(rows, s3, 1, A, B, 4)
    rows[A].append((1, 1, 0.0, F))
    rows[B].append((1, 1, 1.0, F))
    fin = [np.inf] * 6 + [0.0]
    return flat_of_rows(rows, fin)


def chain_across_growth(fan=1100):
    """Two states over {A, B} on one chain when the state arrays grow, the newer one in the level whose check forces the
    growth.  s1 creates O = {A, B: 3 KDELTA}; s2, one level later, N = {A, B: 5 KDELTA} (no match: the chain is N -> O) and
    s3.  The level {.., N, s3} asks for `fan` + 4 candidates on top of 7 states: the states grow, hnext[N] is among the
    entries of the level itself.  In that level s3 then asks for {A, B: 2 KDELTA}, and in the next one (the fan: wide in
    auto) a fan state for {A, B: 3 KDELTA}: both match O alone, which is found only through hnext[N]."""
    s0, s1, s2, s3, A, B, F = range(7)
    rows = [[] for _ in range(7 + fan)]
    rows[s0].append((2, 2, 0.0, s1))
    pair_states(rows, s1, 1, A, B, 3)
    rows[s1].append((2, 2, 0.0, s2))
    pair_states(rows, s2, 1, A, B, 5)
    rows[s2].append((2, 2, 0.0, s3))
    pair_states(rows, s3, 1, A, B, 2)
    for j in range(fan):
        rows[s3].append((10 + j, 10 + j, 0.0, 7 + j))
        rows[7 + j].append((1, 1, float(j % 3), F))
    pair_states(rows, 7, 2, A, B, 3)
    rows[A].append((1, 1, 0.0, F))
    rows[B].append((1, 1, 1.0, F))
    fin = [np.inf] * 6 + [0.0] + [np.inf] * fan
    return flat_of_rows(rows, fin)


def rounds_level(n_ab, n_cd, sources=12):
    """one level whose candidates over {A, B} need n_ab leaders (residuals 0, 2, 4, ... KDELTA: none matches another) and
    those over {C, D} n_cd, every residual several times and out of order"""
    A, B, Cc, D, F = (sources + 1 + k for k in range(5))
    rows = [[] for _ in range(sources + 6)]
    for j in range(sources):
        rows[0].append((j + 1, j + 1, 0.0, j + 1))
        pair_states(rows, j + 1, 1, A, B, 2 * ((j + 1) % n_ab))
        pair_states(rows, j + 1, 2, Cc, D, 2 * ((3 * j + 2) % n_cd))
    for q in (A, B, Cc, D):
        rows[q].append((1, 1, 0.0, F))
    fin = [np.inf] * (sources + 5) + [0.0]
    return flat_of_rows(rows, fin)


SORT_WIDTHS = (1, 2, 15, 16, 17, 31, 32, 33, 100)


def sort_widths():
    """Level 1 holds one two-element subset {P_i, Q_i} per width n in SORT_WIDTHS with exactly n raw candidates: P_i has
    ceil(n / 2) arcs and Q_i floor(n / 2), over 5 labels (one >= 2^31) and 6 destinations in DESCENDING (label, dest)
    order, so Q_i's arcs repeat keys of P_i's and every key arrives out of order.  Weights: small integers, 0.0 and -0.0
    (ties), and +inf on arcs whose key a finite arc shares."""
    n_w = len(SORT_WIDTHS)
    P = [1 + 2 * i for i in range(n_w)]
    Q = [2 + 2 * i for i in range(n_w)]
    T0 = 1 + 2 * n_w
    rows = [[] for _ in range(T0 + 6)]
    labels = (1, 2, 7, 0x80000005, 0xFFFFFFFE)
    cycle = (0.0, -0.0, 1.0, 0.0, 2.0, -0.0, np.inf)
    for i, n in enumerate(SORT_WIDTHS):
        rows[0] += [(i + 1, i + 1, 0.0, P[i]), (i + 1, i + 1, 0.5, Q[i])]
        for src, deg, salt in ((P[i], (n + 1) // 2, 0), (Q[i], n // 2, 1)):
            out = []
            for k in range(deg):  # (arc k - 5 has the same label and, 5 places back in the cycle of 7, a finite weight)
                wt = cycle[(k + 3 * salt + i) % 7]
                lab = labels[k % 5]
                out.append((lab, lab, wt if k >= 5 or wt != np.inf else 1.5, T0 + (k * 5 + i + salt) % 6))
            rows[src] = sorted(out, key=lambda r: (r[0], r[3]), reverse=True)
    fin = [np.inf] * T0 + [0.0, 1.0, -0.0, 0.25, np.inf, 3.0]
    return flat_of_rows(rows, fin)


def fan_then_chain(fan, chain):
    """a start state with `fan` arcs into states that all lead to one chain head, then `chain` states in a row"""
    n = 1 + fan + chain
    deg = np.concatenate([[fan], np.ones(fan + chain - 1, np.int64), [0]])
    arcs = np.zeros(2 * fan + chain - 1, TR_DTYPE)
    arcs["ilabel"][:fan] = np.arange(1, fan + 1)
    arcs["nextstate"][:fan] = np.arange(1, fan + 1)
    arcs["ilabel"][fan:] = 1
    arcs["nextstate"][fan:2 * fan] = fan + 1
    arcs["nextstate"][2 * fan:] = np.arange(fan + 2, n)
    arcs["weight"] = (np.arange(len(arcs)) % 4).astype(np.float32)
    arcs["olabel"] = arcs["ilabel"]
    fin = np.full(n, np.inf, np.float32)
    fin[-1] = 0.0
    flat = dict(n_states=n, start=0, offsets=np.concatenate([[0], np.cumsum(deg)]).astype(np.uint32), arcs=arcs, finals=fin,
                props=ACCEPTOR)
    figs = [(1, fan, fan, fan, fan, 1), (fan, fan, 1, 1, fan, 1)] + [(1, 1, 1, 1, 1, 1)] * (chain - 1) + [(1, 0, 0, 0, 0, 0)]
    return flat, figs


def chain_spec(n):
    return [(1, 1, 1)] * (n - 1) + [(0, 0, 0)]


TAIL = [(3, 3, 1), (1, 1, 1), (0, 0, 0)]
# name -> (spec, back arcs, weighted): layered inputs
LAYERED = {
    # regime switch by states: 1 -> 256 | 257 -> 3 -> 1 -> 1
    "states_256": ([(256, 256, 256), (256, 256, 3)] + TAIL, None, True),
    "states_257": ([(257, 257, 257), (257, 257, 3)] + TAIL, None, True),
    # the host's own choice (the kernel's limit above is met inside a launch): the level after a wide one has 256 | 257 states
    "after_wide_256": ([(257, 257, 257), (257, 257, 256), (256, 256, 3)] + TAIL, None, True),
    "after_wide_257": ([(257, 257, 257), (257, 257, 257), (257, 257, 3)] + TAIL, None, True),
    # regime switch by candidates: 64 states of 128 arcs, and one of them with 129
    "cands_8192": ([(64, 64, 64), (8192, 8192, 3)] + TAIL, None, True),
    "cands_8193": ([(64, 64, 64), (8193, 8193, 3)] + TAIL, None, True),
    # reuse across regimes: 1 -> 2 -> 300 -> 2 -> 2; the level of 300 (wide in auto) reaches levels 0 and 1 (seed, narrow),
    # the levels after it (narrow) reach the two states it created and those of the narrow level before it
    "reuse_regimes": ([(2, 2, 2), (300, 300, 300), (300, 300, 2), (2, 2, 2), (0, 0, 0)],
                      {2: [(1, 50), (0, 7)], 3: [(3, 4), (2, 30), (1, 2)], 4: [(3, 6), (2, 9), (4, 2)]}, False),
    # reuse across a growth: level 1 (600 states, 720 candidates on top of 601 states) grows the states and is re-hashed,
    # then reaches levels 0 and 1; level 2 reaches level 1 as well
    "reuse_growth": ([(600, 600, 600), (600, 600, 5), (5, 5, 1), (0, 0, 0)],
                     {1: [(1, 100), (0, 20)], 2: [(1, 10), (2, 5)], 3: [(1, 3), (0, 1)]}, False),
    # the same inside the narrow kernel: 200 states, 950 candidates on top of 201 states
    "reuse_growth_narrow": ([(200, 200, 200), (900, 900, 5), (5, 5, 1), (0, 0, 0)],
                            {1: [(1, 50)], 2: [(1, 10), (0, 1)], 3: [(1, 3)]}, False),
    # capacities.  states: hi + K = 2 + 1022 = 1024 | 1025
    "cap_states_fit": ([(1, 1, 1), (1022, 1022, 1), (1, 1, 1), (0, 0, 0)], None, True),
    "cap_states_over": ([(1, 1, 1), (1023, 1023, 1), (1, 1, 1), (0, 0, 0)], None, True),
    # states, in a level that is wide in auto: hi + K = 342 + 341 * 2 = 1024 | 1025
    "cap_states_wide_fit": ([(341, 341, 341), (682, 682, 2), (2, 2, 1), (0, 0, 0)], None, True),
    "cap_states_wide_over": ([(341, 341, 341), (683, 683, 2), (2, 2, 1), (0, 0, 0)], None, True),
    # elements: level 1 asks for hi + K + 1 = 4097 states (-> 8192) and n_elts + K = 4096 elements (stay); then
    # n_elts + K = 3 + 4093 = 4096 | 4097 with n_arcs + K = 2 + 4094 = 4096 still fitting
    "cap_elts_fit": ([(1, 1023, 1), (1, 4094, 1), (1, 4093, 1), (0, 0, 0)], None, True),
    "cap_elts_over": ([(1, 1023, 1), (1, 4094, 1), (1, 4094, 1), (0, 0, 0)], None, True),
    # arcs: four levels of 1000 arcs into one state, then n_arcs + K = 4000 + 96 = 4096 | 4097
    "cap_arcs_fit": ([(1000, 1000, 1)] * 4 + [(96, 96, 1), (0, 0, 0)], None, True),
    "cap_arcs_over": ([(1000, 1000, 1)] * 4 + [(97, 97, 1), (0, 0, 0)], None, True),
    # candidates: level 1 (K = 4096) takes states, elements and arcs to 8192 and leaves 4096 candidates; then K = 4096 | 4097
    "cap_cands_fit": ([(1, 1023, 1), (1, 4096, 1), (1, 4096, 1), (0, 0, 0)], None, True),
    "cap_cands_over": ([(1, 1023, 1), (1, 4096, 1), (1, 4097, 1), (0, 0, 0)], None, True),
    # level budget
    "chain_300": (chain_spec(300), None, True),
    # the batch kernel's LDS scratch: the widest level at 496 | 497 raw candidates, and levels on both sides in turn
    "lds_496": ([(1, 1, 1), (496, 496, 5), (5, 5, 1), (0, 0, 0)], None, True),
    "lds_497": ([(1, 1, 1), (497, 497, 5), (5, 5, 1), (0, 0, 0)], None, True),
    "lds_alternating": ([(1, 1, 1), (600, 600, 4), (10, 10, 1), (100, 497, 2), (496, 496, 3), (3, 3, 1), (500, 500, 1),
                         (0, 0, 0)], None, True),
}
# name -> builder of a flat whose figures come from det_levels
OTHER = {
    "diamond_300": lambda: inputs.diamond_chain(300),
    "lowest_id_levels": lambda: lowest_id_chain(False),
    "lowest_id_same_level": lambda: lowest_id_chain(True),
    "chain_across_growth": chain_across_growth,
    "sort_widths": sort_widths,
    "collision_8_40": lambda: collision_level(8, 40),
    "collision_16_100": lambda: collision_level(16, 100, seed=9),
    "rounds_3_4": lambda: rounds_level(3, 4),
    "rounds_5_2": lambda: rounds_level(5, 2),
    "rounds_1_2": lambda: rounds_level(1, 2),
}
BUDGET_FAN, BUDGET_CHAIN = 140_000, 65_540


@functools.lru_cache(maxsize=None)
def case(name):
    """(flat, figs) of a named input; never modified"""
    if name in LAYERED:
        spec, back, weighted = LAYERED[name]
        return layered(spec, back, weighted)
    if name == "budget_real":
        return fan_then_chain(BUDGET_FAN, BUDGET_CHAIN)
    flat = OTHER[name]()
    return flat, analysis(name)["figs"]


@functools.lru_cache(maxsize=None)
def analysis(name):
    flat = OTHER[name]() if name in OTHER else case(name)[0]
    return det_levels(flat)
