"""push.hip at its limits: rows longer than the 16 lanes a state gets, frontier searches whose depth sits on the edges of the
round batching, grids small enough to stride (WFST_PUSH_MAX_BLOCKS), and reductions that cross waves and blocks — each
compared bit for bit with the restatement of reweight.rs / push.rs in oracle/model/push.py over the oracle's distances, and
with wfst_ctx_get_push_stats saying which route ran.

The structural facts are checked three ways: numpy graph_facts and the oracle's own depth-first visit (OracleFst.
dfs_properties) must agree on every input before the device is asked; the device's answer is read from the word of a
reweight result whose input word is 0 (every bit of a DFS pair that survives the later masks must be the fact's) and from
the start branch it takes.

The expected rounds and reads of a search come from the round rule of DESIGN.md §3.7, restated here as round_rule(), and
the number E of rounds after which a frontier is empty, which for a chain is its length (test_generators_reach_every_case
checks the closed forms against the level-by-level count used for every other graph).

All generated weights lie on the 1/512 grid, so every sum the device and the restatement form is exact; the one exception
is a final weight that brings a total weight to 1/2048, inside the reference's KDELTA of one."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from rustfst_amd._lib import TR_DTYPE
from oracle import model
from oracle.model import graph_facts, push_ref, reverse_len_rule, reweight_ref, to_flat
import helpers
from helpers import _oracle_dist, assert_same, to_device, to_oracle

ROOT = helpers.ROOT
F32, INF = np.float32, np.float32(np.inf)
COUNTERS = ("searches", "rounds", "reads", "rounds_max", "bfs_blocks", "arcs_blocks", "total_blocks", "structural",
            "start_branch", "removed")
# documented in include/wfst.h and DESIGN.md §3.7; test_constants_are_the_kernels compares them with push.hip
ROUNDS_PER_CHECK = 16
BFS_BLOCKS_PER_CU, ARCS_BLOCKS_PER_CU, TOTAL_BLOCKS_PER_CU = 8, 32, 4
GRID = 512
KNOB = "WFST_PUSH_MAX_BLOCKS"


# ---------------------------------------------------------------- builders
def make_flat_fst(rows, finals, start, props=0):
    """rows[s] = [(ilabel, olabel, weight, nextstate), ..]; finals[s] = weight or None"""
    n = len(rows)
    off = np.zeros(n + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(r) for r in rows])
    arcs = np.array([tuple(a) for r in rows for a in r], dtype=TR_DTYPE) if off[-1] else np.zeros(0, dtype=TR_DTYPE)
    fin = np.array([np.inf if f is None else f for f in finals], dtype=np.float32)
    return dict(n_states=n, start=start, offsets=off, arcs=arcs, finals=fin, props=props)


def grid(rng, lo, hi, size=None):
    """weights on the 1/512 grid in [lo, hi)"""
    v = rng.integers(int(lo * GRID), int(hi * GRID), size) / GRID
    return float(v) if size is None else v


def renumber(flat, perm):
    """state s becomes perm[s]; the order of arcs inside a state stays"""
    n = flat["n_states"]
    off, arcs = flat["offsets"], flat["arcs"]
    rows, finals = [None] * n, [None] * n
    for s in range(n):
        rows[perm[s]] = [(int(a["ilabel"]), int(a["olabel"]), float(a["weight"]), int(perm[a["nextstate"]]))
                         for a in arcs[off[s]:off[s + 1]]]
        finals[perm[s]] = None if not np.isfinite(flat["finals"][s]) else float(flat["finals"][s])
    return make_flat_fst(rows, finals, None if flat["start"] is None else int(perm[flat["start"]]), flat["props"])


LADDER_DEGREES = (0, 1, 15, 16, 17, 31, 32, 33, 100)
LADDER_PARALLEL = (16, 20, 3)  # rows made only of parallel arcs to one target


def ladder(variant, seed=11):
    """out-degrees 0, 1, 15, 16, 17, 31, 32, 33, 100 and three rows of parallel arcs, in shuffled state order.
    cyclic: random targets, a self-loop on the start and on the row of 33; the state without arcs is not final (so not every
    state reaches a final one).  acyclic: targets above the source.  middle: the cyclic one with its start moved.
    Arc 16 and the last arc of every random row of 17 or more arcs lead to a final state of their own at the top of the id
    range, which nothing else reaches: a trip of a 16-lane loop that is left out loses that state.  The highest of them
    hangs on arc 16 of the start, so the forward length shows its loss; the peeling of the acyclic ladder shows the loss of
    any of them as a cycle.  isolated: the acyclic one, with a final start state of its own without arcs behind it — the
    one shape whose reweight result keeps the CYCLIC / ACYCLIC and ACCESSIBLE pairs the searches found."""
    rng = np.random.default_rng(seed)
    kinds = [(d, False) for d in LADDER_DEGREES] + [(d, True) for d in LADDER_PARALLEL] + [(2, False), (2, False)]
    n = len(kinds)
    order = list(rng.permutation(n))
    kinds = [kinds[i] for i in order]
    isolated, variant = variant == "isolated", "acyclic" if variant == "isolated" else variant
    start = n // 2 if variant == "middle" else 0
    i17, i0 = kinds.index((17, False)), kinds.index((0, False))
    kinds[start], kinds[i17] = kinds[i17], kinds[start]  # the start has a row of 17: two trips of the 16-lane loop
    if variant == "acyclic":
        i0 = kinds.index((0, False))
        kinds[n - 1], kinds[i0] = kinds[i0], kinds[n - 1]
    rows = []
    for s, (deg, parallel) in enumerate(kinds):
        if variant == "acyclic":
            deg = deg if s + 1 < n else 0
            pick = lambda k: rng.integers(s + 1, n, k)  # noqa: E731
        else:
            pick = lambda k: rng.integers(0, n, k)  # noqa: E731
        tg = np.full(deg, pick(1)[0]) if parallel and deg else pick(deg)
        if variant != "acyclic" and (s == start or deg == 33):
            tg[int(rng.integers(0, 16))] = s
        rows.append([(int(rng.integers(1, 9)), int(rng.integers(1, 9)), grid(rng, 0, 5), int(t)) for t in tg])
    for s in [s for s in range(n) if s != start] + [start]:
        for idx in sorted({16, len(rows[s]) - 1}, reverse=True) if len(rows[s]) >= 17 and not kinds[s][1] else ():
            rows[s][idx] = rows[s][idx][:3] + (len(rows),)
            rows.append([])
    finals = [grid(rng, 0, 5) if rng.random() < 0.4 or s >= n else None for s in range(len(rows))]
    n = len(rows)
    sink = [s for s in range(n) if not rows[s]][0]
    finals[sink] = grid(rng, 0, 5) if variant == "acyclic" else None
    if variant != "acyclic":
        for s in range(n):
            if s != sink and all(finals[t] is None for t in range(n) if t != sink):
                finals[s] = 1.5
                break
    if isolated:
        rows.append([])
        finals.append(0.75)
        start = n
    return make_flat_fst(rows, finals, start)


CHAIN_DEPTHS = (1, 2, 15, 16, 17, 31, 32, 33, 48, 49)
CHAIN_FORMS = ("open", "to_start", "to_1")


def chain(d, form, flipped, seed=23):
    """d states in a line from the start; the last one is final; closed by an arc from the last state to the start or to the
    second state.  flipped: the same chain with state i numbered d - 1 - i, so that the search runs downwards."""
    rng = np.random.default_rng(seed + d)
    rows = [[(1 + s % 7, 1 + s % 5, grid(rng, 0, 5), s + 1)] if s + 1 < d else [] for s in range(d)]
    if form == "to_start":
        rows[d - 1].append((3, 3, grid(rng, 0, 5), 0))
    elif form == "to_1":
        assert d >= 2
        rows[d - 1].append((3, 3, grid(rng, 0, 5), 1))
    finals = [None] * (d - 1) + [grid(rng, 0, 5)]
    f = make_flat_fst(rows, finals, 0)
    return renumber(f, np.arange(d)[::-1]) if flipped else f


def tree(back_arc, seed=31):
    """a root with 100 children, each with 3 children (401 states), ids shuffled; the leaves are final.  back_arc: one leaf
    leads back to the root."""
    rng = np.random.default_rng(seed)
    rows = [[(1 + c % 9, 1, grid(rng, 0, 5), 1 + c) for c in range(100)]]
    rows += [[(1 + k, 2, grid(rng, 0, 5), 101 + 3 * c + k) for k in range(3)] for c in range(100)]
    rows += [[] for _ in range(300)]
    if back_arc:
        rows[400].append((5, 5, 0.5, 0))
    finals = [None] * 101 + [grid(rng, 0, 5) for _ in range(300)]
    return renumber(make_flat_fst(rows, finals, 0), rng.permutation(401))


def random_cyclic(n, seed):
    rng = np.random.default_rng(seed)
    rows = [[(int(rng.integers(1, 9)), int(rng.integers(1, 9)), grid(rng, 0, 5), int(rng.integers(0, n)))
             for _ in range(int(rng.integers(0, 5)))] for _ in range(n)]
    finals = [grid(rng, 0, 5) if rng.random() < 0.3 else None for _ in range(n)]
    return make_flat_fst(rows, finals, 0)


def acyclic_dist(rows, n):
    """distances from state 0 when every arc goes upwards (exact: grid weights)"""
    d = [INF] * n
    d[0] = F32(0)
    for s in range(n):
        if d[s] != INF:
            for (_, _, w, t) in rows[s]:
                d[t] = min(d[t], F32(d[s] + F32(w)))
    return d


def reduction_fst(n, seed, a, b, total="pos", b_new="weighted", b_eps=False):
    """An acyclic FST (every arc goes upwards, start 0) for push to final with remove_total_weight:
      a  the one state that attains the total weight (+)_s dist[s] (x) final[s]; it has no arcs of its own;
      b  the highest-numbered final state whose weight before or after the division is weighted — every final state above
         it cannot be reached, so both its weights are zero; b_new says whether b's weight after the division is weighted
         (total + 1.5) or one (the total itself, with b_eps 1/2048 more).  b == a: a decides, its new weight is one.
    total: pos (0.75), neg (below every other sum, negative arc and final weights), zero (0, with b_eps 1/2048: remove is
    skipped), inf (no final state can be reached: the total is zero, remove is skipped)."""
    rng = np.random.default_rng(seed)
    lo, hi = (-2, 2) if total == "neg" else (1, 4)
    fixed = {0, a, b}
    unreach = {int(s) for s in rng.choice(np.arange(1, n), size=min(n - 1, n // 16 + 2), replace=False)} - fixed
    unreach |= {s for s in (b + 1, n - 1) if b < s < n and s not in fixed}
    reach = [s for s in range(n) if s not in unreach]
    rows = [[] for _ in range(n)]
    inner = [s for s in reach if s not in (a, b) or s == 0]  # states that may have arcs
    for s in reach[1:]:
        parents = [p for p in inner if p < s]
        rows[int(rng.choice(parents))].append((1 + s % 9, 1 + s % 4, grid(rng, lo, hi), s))
    for s in inner + sorted(unreach):
        ups = [t for t in reach if t > s]
        for _ in range(int(rng.integers(0, 3)) if ups else 0):
            rows[s].append((int(rng.integers(1, 9)), 1, grid(rng, lo, hi), int(rng.choice(ups))))
    finals = [None] * n
    for s in unreach:
        finals[s] = grid(rng, lo, hi) if rng.random() < 0.6 or s > b else None
    if total != "inf":
        for s in inner[1:]:
            if s < b and rng.random() < 0.3:
                finals[s] = grid(rng, lo, hi)
        d = acyclic_dist(rows, n)
        others = [float(d[s]) + finals[s] for s in reach if finals[s] is not None]
        if total == "neg":
            direct = min([float(d[a]) if d[a] != INF else 0.0, 0.0] + others) - 4.0
            fa = -1.0
        else:
            direct = 0.25
            fa = 0.5 if total == "pos" else -0.25 + (1 / 2048 if b_eps else 0.0)
        rows[0].append((9, 9, direct, a))
        finals[a] = fa
        t = direct + fa
        if b != a:
            db = float(acyclic_dist(rows, n)[b])
            finals[b] = t + (1.5 if b_new == "weighted" else (1 / 2048 if b_eps else 0.0)) - db
    return make_flat_fst(rows, finals, 0)


REDUCTION_SIZES = (63, 64, 65, 255, 256, 257, 600)


def positions(n, per_state_lanes=1):
    """a state in the first wave, in the last wave of block 0, in block 1 and in the last, partly filled block of a launch
    that gives each state per_state_lanes lanes of a 256-thread block (never state 0, the start); fewer where n is small"""
    per_block, per_wave = 256 // per_state_lanes, 64 // per_state_lanes
    out = [min(per_wave - 1, n - 1, 2)]
    out.append(min(n, per_block) - 1)
    if n > per_block:
        out.append(min(per_block + per_wave + 5, n - 1))
        out.append(n - 1)
    return sorted(set(out))


# ---------------------------------------------------------------- the round rule
def round_rule(n, e):
    """(rounds, reads) of a frontier search over n states whose frontier is first empty after e >= 1 rounds: the host reads
    the frontier size after round R when R is a multiple of 16 or R = n + 1, and stops at the first read that finds it
    empty, or at R = n + 1"""
    rounds = min(n + 1, ROUNDS_PER_CHECK * -(-e // ROUNDS_PER_CHECK))
    reads = rounds // ROUNDS_PER_CHECK + (1 if rounds == n + 1 and rounds % ROUNDS_PER_CHECK else 0)
    return rounds, reads


def _rows_of(off, nxt, fr):
    cnt = off[fr + 1] - off[fr]
    idx = np.repeat(off[fr] - np.cumsum(np.r_[0, cnt[:-1]]), cnt) + np.arange(cnt.sum())
    return nxt[idx]


def empty_after(off, nxt, frontier, mark, peel):
    """E: the first R >= 1 such that frontier R is empty, level by level as the rounds form them (frontier 0 given)"""
    fr, r = np.asarray(frontier, dtype=np.int64), 0
    mark = mark.copy()
    while fr.size:
        r += 1
        t = _rows_of(off, nxt, fr)
        if peel:
            np.subtract.at(mark, t, 1)
            t = np.unique(t)
            fr = t[mark[t] == 0]
        else:
            t = np.unique(t)
            fr = t[mark[t] == 0]
            mark[fr] = 1
    return max(r, 1)


def reversed_graph(flat):
    """reverse(f) as the searches see it: n + 1 states, 0 -> s + 1 for every final s, t + 1 -> s + 1 for every arc s -> t"""
    n = flat["n_states"]
    off, nxt = model.csr_next(flat)
    roff, rsrc = model.transpose(n, off, nxt)
    fin = np.nonzero(np.isfinite(flat["finals"]))[0]
    return n + 1, np.r_[0, roff + fin.size], np.r_[fin + 1, rsrc + 1]


def search_forward_len(flat):
    n, s0 = flat["n_states"], flat["start"]
    off, nxt = model.csr_next(flat)
    mark = np.zeros(n, dtype=np.int64)
    mark[s0] = 1
    return n, empty_after(off, nxt, [s0], mark, False)


def search_reverse_len(flat):
    m, off, nxt = reversed_graph(flat)
    mark = np.zeros(m, dtype=np.int64)
    mark[0] = 1
    return m, empty_after(off, nxt, [0], mark, False)


def searches_structural(flat):
    """the four searches of structural_bits: from the start, from state 0 of the reversed FST, the peeling, and from the
    start with the start left unvisited"""
    n, s0 = flat["n_states"], flat["start"]
    off, nxt = model.csr_next(flat)
    indeg = np.bincount(nxt, minlength=n).astype(np.int64)
    return [search_forward_len(flat), search_reverse_len(flat),
            (n, empty_after(off, nxt, np.nonzero(indeg == 0)[0], indeg, True)),
            (n, empty_after(off, nxt, [s0], np.zeros(n, dtype=np.int64), False))]


def search_counters(searches):
    rr = [round_rule(n, e) for n, e in searches]
    return dict(searches=len(rr), rounds=sum(r for r, _ in rr), reads=sum(k for _, k in rr),
                rounds_max=max([r for r, _ in rr] + [0]),
                bfs_blocks=(searches[-1][0] + 15) // 16 if searches else 0)


# ---------------------------------------------------------------- what a call is expected to do
def total_weight(flat, dist, to_final):
    """compute_total_weight (push.rs:120-142) of the input, for sorting the cases into their categories"""
    if not to_final:
        s0 = flat["start"]
        return F32(dist[s0]) if s0 is not None and s0 < len(dist) else INF
    return min([INF] + [model.times(d, f) for d, f in zip(dist, flat["finals"]) if np.isfinite(f)])


def start_branch_of(flat, pot, facts):
    """0 not taken, 1 in place, 2 new start state; and whether the four facts have to be searched"""
    s0 = flat["start"]
    d = F32(pot[s0]) if s0 is not None and s0 < len(pot) else INF
    if s0 is None or model.is_one(d) or model.is_zero(d):
        return 0, False
    known = flat["props"] & (model.INITIAL_CYCLIC | model.INITIAL_ACYCLIC)
    cyclic = bool(flat["props"] & model.INITIAL_CYCLIC) if known else facts[3]
    return (2 if cyclic else 1), not known


def expected_counters(flat, call, pot, facts, cap=None):
    """every counter of one call, from the input alone.  pot: the potentials of a reweight or the distances of a push"""
    blocks = lambda want: max(1, want if cap is None else min(want, cap))  # noqa: E731
    n = flat["n_states"]
    exp = dict.fromkeys(COUNTERS, 0)
    if call[0] == "len":
        exp.update(search_counters([search_reverse_len(flat) if call[1] else search_forward_len(flat)]))
    else:
        branch, searched = start_branch_of(flat, pot, facts)
        if searched:
            exp.update(search_counters(searches_structural(flat)))
        exp.update(start_branch=branch, structural=int(searched))
        exp["arcs_blocks"] = blocks((n + 15) // 16) if len(flat["arcs"]) else 0
        if call[0] == "push" and call[2]:
            t = total_weight(flat, pot, call[1] == 1)
            exp["removed"] = 1 if model.is_one(t) or model.is_zero(t) else 2
            exp["total_blocks"] = blocks((n + 255) // 256) if call[1] == 1 else 0
    if exp["bfs_blocks"]:
        exp["bfs_blocks"] = blocks(exp["bfs_blocks"])
    return exp


def potentials(rng, n, k, start, force):
    pot = grid(rng, -8, 8, k).astype(np.float32)
    pot[rng.random(k) < 0.2] = np.inf
    if force is not None and start is not None and start < k:
        pot[start] = force
    return pot


def calls_of(flat, seed):
    """the calls every case of (a) and (b) is put through: reweight of both types with potentials of length 0, 1, n - 1, n
    and n + 3 (some entries +inf; the start's potential in turn 2.5, random, and one), push of both types with and without
    remove, and both distance lengths"""
    rng = np.random.default_rng(seed)
    n = flat["n_states"]
    out, i = [], 0
    for k in sorted({0, 1, max(n - 1, 0), n, n + 3}):
        for rt in (0, 1):
            out.append(("reweight", rt, potentials(rng, n, k, flat["start"], (2.5, None, 0.0, 2.5)[i % 4])))
            i += 1
    out += [("push", rt, remove) for rt in (0, 1) for remove in (False, True)]
    out += [("len", False), ("len", True)]
    return out


def structural_calls(flat):
    """reweight with finite potentials and a start potential that is neither one nor zero: on a word of 0 the four facts are
    searched and the start branch follows INITIAL_CYCLIC"""
    n = flat["n_states"]
    pot = (np.arange(n) % 7).astype(np.float32) / 4
    pot[flat["start"]] = 2.5
    return [("reweight", rt, pot) for rt in (0, 1)]


def oracle_dist(oracle, flat, to_final):
    return _oracle_dist(oracle, flat, to_final)


def restate(oracle, flat, call, facts):
    """(expected result as flat arrays or a length, the potentials / distances the call works with)"""
    if call[0] == "len":
        if call[1]:
            return reverse_len_rule(flat), None
        off, nxt = model.csr_next(flat)
        return int(np.nonzero(model.reach(flat["n_states"], off, nxt, [flat["start"]]))[0].max()) + 1, None
    if call[0] == "reweight":
        return to_flat(reweight_ref(flat, list(call[2]), call[1] == 1, facts)), call[2]
    dist = oracle_dist(oracle, flat, call[1] == 1)
    return to_flat(push_ref(flat, dist, call[1] == 1, call[2], facts)), dist


def dfs_facts(oracle, flat):
    """the two references of the structural facts, which must agree before anything else is asked"""
    facts = graph_facts(flat)
    word = to_oracle(oracle, flat).dfs_properties()
    assert word == model.dfs_bits(facts), f"graph_facts {facts} but the oracle's DFS says {word:#x}"
    return facts


# ---------------------------------------------------------------- the case list
@functools.lru_cache(maxsize=None)
def case(name):
    kind, *args = name.split(":")
    if kind == "ladder":
        return ladder(args[0])
    if kind == "chain":
        return chain(int(args[0]), args[1], args[2] == "down")
    if kind == "tree":
        return tree(args[0] == "back")
    if kind == "random":
        return random_cyclic(int(args[0]), 41)
    if kind == "reduce":
        n, a, b, total, b_new, eps = args
        return reduction_fst(int(n), 57 + int(n), int(a), int(b), total, b_new, eps == "e")
    raise KeyError(name)


LADDER_CASES = ["ladder:cyclic", "ladder:acyclic", "ladder:middle", "ladder:isolated"]


def chain_cases(d):
    return [f"chain:{d}:{form}:{way}" for form in CHAIN_FORMS if not (form == "to_1" and d < 2) for way in ("up", "down")]


def reduction_cases(n):
    """(name, what the case is for)"""
    out = []
    last_reachable = n - 2
    for i, p in enumerate(positions(n)):
        other = 1 if p != 1 else 3
        out.append((f"reduce:{n}:{p}:{last_reachable if p != last_reachable else other}:pos:weighted:x", "total_pos"))
        out.append((f"reduce:{n}:{p}:{last_reachable if p != last_reachable else other}:neg:weighted:x", "total_neg"))
        out.append((f"reduce:{n}:{other}:{p}:pos:weighted:x", "decider_weighted"))
        out.append((f"reduce:{n}:{other}:{p}:pos:one:{'e' if i % 2 else 'x'}", "decider_one"))
        out.append((f"reduce:{n}:{other}:{p}:neg:one:{'x' if i % 2 else 'e'}", "decider_one"))
    out.append((f"reduce:{n}:{positions(n)[-1]}:1:zero:weighted:x", "total_one"))
    out.append((f"reduce:{n}:{positions(n)[-1]}:1:zero:weighted:e", "total_one"))
    out.append((f"reduce:{n}:1:2:inf:weighted:x", "total_zero"))
    return out


STRIDE_CASES = ["tree:plain", "tree:back"]
ALL_GRAPHS = LADDER_CASES + [c for d in CHAIN_DEPTHS for c in chain_cases(d)] + STRIDE_CASES + ["random:700"] + \
    [c for n in REDUCTION_SIZES for c, _ in reduction_cases(n)] + ["reduce:1000:900:998:pos:weighted:x"]


def decider(mid, total):
    """remove_weight at the final states (push.rs:155-162): the highest final state whose weight before or after the division
    is weighted, and whether the one after is — the set_final call that leaves WEIGHTED as the result has it"""
    best = None
    for s, f in enumerate(mid["finals"]):
        if f is not None:
            new = model.divide(f, total)
            if model.weighted(f) or model.weighted(new):
                best = (s, model.weighted(new))
    return best


# facts of the word that reweight_marks may clear: NOT_STRING and NOT_COACCESSIBLE go with any set_final, and with an arc
# through set_weight_unchecked everything but the arc-relevant bits
FACTS_WORD = model.NOT_STRING | model.NOT_COACCESSIBLE | model.ACCESSIBLE | model.ACYCLIC | model.INITIAL_ACYCLIC | model.I_LABEL_SORTED


def facts_cases(n, seed=71):
    """reweight towards the initial state on a random FST whose word is FACTS_WORD, with every potential zero but:
      arc    those of one state s and of one target t of it: only the arcs s -> t go through set_weight_unchecked;
      final  that of one final state s: only its weight goes through set_final;
      none   nothing: the word comes back as it is.
    s sits in the first wave, the last wave of block 0, block 1 and the last block of the kernel concerned."""
    rng = np.random.default_rng(seed + n)
    rows = [[(int(rng.integers(1, 9)), 1, grid(rng, 0, 5), int(rng.choice([t for t in range(1, n) if t != s] or [0])))
             for _ in range(int(rng.integers(1, 4)))] for s in range(n)]
    finals = [grid(rng, 0, 5) if s % 3 == 0 else None for s in range(n)]
    out = []
    inf = np.full(n, np.inf, dtype=np.float32)
    out.append(("none", make_flat_fst(rows, finals, 0, FACTS_WORD), inf))
    for s in positions(n, 16):
        r, f = [list(x) for x in rows], list(finals)
        t = r[s][0][3]
        f[s] = f[t] = None
        r[t] = [a for a in r[t] if a[3] not in (s, t)] or [(1, 1, 0.5, 0)]
        pot = inf.copy()
        pot[s], pot[t] = 1.25, -0.75
        out.append((f"arc@{s}", make_flat_fst(r, f, 0, FACTS_WORD), pot))
    for s in positions(n):
        f = list(finals)
        f[s] = 0.5
        pot = inf.copy()
        pot[s] = 1.25
        out.append((f"final@{s}", make_flat_fst(rows, f, 0, FACTS_WORD), pot))
    return out


# ================================================================ no GPU
def test_symbol_declared_and_bound(wfst_lib):
    import rustfst_amd
    name = "wfst_ctx_get_push_stats"
    header = helpers.check_counter_getter(wfst_lib, name, COUNTERS, rustfst_amd.Context.push_stats)
    assert KNOB in header and "unspecified" in header.split("wfst_status " + name)[0].rsplit("/* ----", 1)[1]
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        assert name in f.read()


def test_null_ctx_is_ko(wfst_lib):
    helpers.null_ctx_is_ko(wfst_lib, "wfst_ctx_get_push_stats", len(COUNTERS))


def test_constants_are_the_kernels():
    with open(os.path.join(ROOT, "rustfst_amd", "csrc", "push.hip")) as f:
        src = f.read()
    for name, value in (("ROUNDS_PER_CHECK", ROUNDS_PER_CHECK), ("BFS_BLOCKS_PER_CU", BFS_BLOCKS_PER_CU),
                        ("ARCS_BLOCKS_PER_CU", ARCS_BLOCKS_PER_CU), ("TOTAL_BLOCKS_PER_CU", TOTAL_BLOCKS_PER_CU)):
        m = re.findall(r"constexpr uint32_t " + name + r" = (\d+);", src)
        assert m == [str(value)], name
    # each factor is used by the launch of its kernel, and by nothing else
    for name, kernel in (("BFS_BLOCKS_PER_CU", "bfs_round_kernel"), ("ARCS_BLOCKS_PER_CU", "reweight_arcs_kernel"),
                         ("TOTAL_BLOCKS_PER_CU", "total_weight_kernel")):
        uses = re.findall(r"blocks = strided_grid\(ctx, [^;]*, " + name + r"\);[^\n]*\n\s*(?:[^\n<]*\n\s*){0,6}?(\w+)<<<blocks, 256",
                          src)
        assert uses == [kernel], (name, uses)
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = f.read()
    assert f"`ROUNDS_PER_CHECK` = {ROUNDS_PER_CHECK}" in design
    with open(os.path.join(ROOT, "include", "wfst.h")) as f:
        header = f.read()
    doc = header.split("wfst_status wfst_ctx_get_push_stats")[0].rsplit("/* ----", 1)[1]
    assert f"multiple of\n *      {ROUNDS_PER_CHECK} or R = n + 1" in doc
    assert f"at most {BFS_BLOCKS_PER_CU} blocks per" in doc and f"at most {ARCS_BLOCKS_PER_CU} per compute unit" in doc
    assert f"at most {TOTAL_BLOCKS_PER_CU} per compute unit" in doc


def test_round_rule_by_hand():
    """the rule written out for the chain lengths of (b): a chain of d states searched from its first state has its first
    empty frontier after d rounds"""
    by_hand = {1: (2, 1), 2: (3, 1), 15: (16, 1), 16: (16, 1), 17: (18, 2), 31: (32, 2), 32: (32, 2), 33: (34, 3),
               48: (48, 3), 49: (50, 4)}
    assert set(by_hand) == set(CHAIN_DEPTHS)
    for d, exp in by_hand.items():
        assert round_rule(d, d) == exp, d
    assert round_rule(100, 1) == (16, 1) and round_rule(5, 1) == (6, 1) and round_rule(15, 3) == (16, 1)


def _entry_points(lib):
    from rustfst_amd import _lib
    out = C.c_void_p()
    cfg = _lib.ShortestDistanceConfig(1, 1e-6)
    return (("wfst_reweight", lambda: lib.wfst_reweight(None, None, None, 0, 1, C.byref(out))),
            ("wfst_push_weights", lambda: lib.wfst_push_weights(None, None, 0, None, C.byref(out))),
            ("wfst_shortest_distance_with_config",
             lambda: lib.wfst_shortest_distance_with_config(None, None, C.byref(cfg), None, None)))


BAD_KNOB = ("0", "-1", "x", "3x", " 3", "+3", "1.5", "00", "4294967296000")
GOOD_KNOB = ("", "1", "3", "07", "100000")


def test_knob_validation_without_gpu(wfst_lib, monkeypatch):
    for value in BAD_KNOB:
        monkeypatch.setenv(KNOB, value)
        for name, call in _entry_points(wfst_lib):
            msg = helpers.ko_message(call())
            assert KNOB in msg and f"'{value}'" in msg, (name, value, msg)
    for value in GOOD_KNOB:
        monkeypatch.setenv(KNOB, value)
        for name, call in _entry_points(wfst_lib):
            assert "null" in helpers.ko_message(call()), (name, value)
    monkeypatch.delenv(KNOB)
    for name, call in _entry_points(wfst_lib):
        assert "null" in helpers.ko_message(call()), name


def test_restatement_agrees_with_the_oracle_dfs(oracle):
    seen = set()
    for name in ALL_GRAPHS:
        seen.add(dfs_facts(oracle, case(name)))
    for n in REDUCTION_SIZES:
        for _, flat, _ in facts_cases(n):
            dfs_facts(oracle, flat)
    for i in range(4):
        assert {f[i] for f in seen} == {True, False}, f"fact {i} is never {'true' if seen else 'false'}"
    # without a start state nothing is visited
    none = dict(case("ladder:cyclic"), start=None)
    assert to_oracle(oracle, none).dfs_properties() == model.dfs_bits((True, True, False, False))


def test_generators_reach_every_case(oracle):
    """the restatement alone over the whole case list: every category a device test claims to cover is there"""
    reached = set()
    # (a), (b): start branches, removal, structural facts
    for name in LADDER_CASES + [c for d in CHAIN_DEPTHS for c in chain_cases(d)] + STRIDE_CASES:
        flat = case(name)
        facts = dfs_facts(oracle, flat)
        for i, f in enumerate(facts):
            reached.add(("fact", i, f))
        for call in calls_of(flat, 5) + structural_calls(flat):
            exp, pot = restate(oracle, flat, call, facts)
            if call[0] == "len":
                continue
            st = expected_counters(flat, call, pot, facts)
            reached.add(("start_branch", call[1], st["start_branch"]))
            assert st["start_branch"] == (0 if exp["n_states"] == flat["n_states"] and not st["structural"] else
                                          2 if exp["n_states"] > flat["n_states"] else 1)
            if call[0] == "push":
                reached.add(("removed", call[1], st["removed"]))
    for rt in (0, 1):
        for v in (0, 1, 2):
            assert ("start_branch", rt, v) in reached, (rt, v)
    for i in range(4):
        assert ("fact", i, True) in reached and ("fact", i, False) in reached, i
    # the rows of the ladder: every degree, parallel rows, self-loops, one of them on the start
    for name in LADDER_CASES:
        flat = case(name)
        deg = np.diff(flat["offsets"].astype(np.int64))
        acyclic = name in ("ladder:acyclic", "ladder:isolated")
        assert set(LADDER_DEGREES) <= set(deg), name
        src = np.repeat(np.arange(flat["n_states"]), deg)
        loops = set(src[flat["arcs"]["nextstate"] == src])
        if not acyclic:
            assert flat["start"] in loops and len(loops) >= 2
        else:
            assert not loops and np.all(flat["arcs"]["nextstate"] > src)
        par = [s for s in range(flat["n_states"]) if deg[s] >= 16 and
               len(set(flat["arcs"]["nextstate"][flat["offsets"][s]:flat["offsets"][s + 1]])) == 1]
        assert par, name
        # states of their own behind arc 16 and behind the last arc of the long rows
        pos = np.arange(len(src)) - flat["offsets"].astype(np.int64)[src]
        indeg = np.bincount(flat["arcs"]["nextstate"], minlength=flat["n_states"])
        own = [(int(deg[src[i]]), int(pos[i])) for i in range(len(src)) if indeg[flat["arcs"]["nextstate"][i]] == 1 and
               pos[i] >= 16 and np.isfinite(flat["finals"][flat["arcs"]["nextstate"][i]])]
        assert {(17, 16), (31, 16), (31, 30), (32, 16), (32, 31), (33, 16), (33, 32), (100, 16), (100, 99)} <= set(own), (name, own)
        top = int(flat["arcs"]["nextstate"].max())  # the highest state there is hangs on arc 16 of the start alone
        into = np.nonzero(flat["arcs"]["nextstate"] == top)[0]
        if name != "ladder:isolated":
            assert top == flat["n_states"] - 1 and len(into) == 1 and (src[into[0]], pos[into[0]]) == (flat["start"], 16), name
    iso = case("ladder:isolated")
    assert iso["start"] == iso["n_states"] - 1 and np.isfinite(iso["finals"][iso["start"]])
    assert graph_facts(iso) == (False, True, False, False) and not np.diff(iso["offsets"].astype(np.int64))[iso["start"]]
    assert np.array_equal(iso["arcs"], case("ladder:acyclic")["arcs"])
    assert case("ladder:middle")["start"] not in (0, case("ladder:middle")["n_states"] - 1)
    # (b): the closed forms of the chains against the level-by-level count
    for d in CHAIN_DEPTHS:
        for way in ("up", "down"):
            flat = case(f"chain:{d}:open:{way}")
            assert search_forward_len(flat) == (d, d) and search_reverse_len(flat) == (d + 1, d + 1)
            assert searches_structural(flat) == [(d, d), (d + 1, d + 1), (d, d), (d, d)]
            closed = case(f"chain:{d}:to_start:{way}")  # nothing to peel; the second start search comes round once
            assert searches_structural(closed) == [(d, d), (d + 1, d + 1), (d, 1), (d, d + 1)]
            assert graph_facts(closed) == (True, True, True, True)
            if d >= 2:
                lasso = case(f"chain:{d}:to_1:{way}")  # the peeling takes the start and stops
                assert searches_structural(lasso) == [(d, d), (d + 1, d + 1), (d, 1), (d, d)]
                assert graph_facts(lasso) == (True, True, True, False)
    assert case("chain:17:open:down")["start"] == 16
    # (c): widths against the capped grids
    for name in STRIDE_CASES:
        flat = case(name)
        off, nxt = model.csr_next(flat)
        kids = _rows_of(off, nxt, np.array([flat["start"]]))
        assert flat["n_states"] == 401 and kids.size == 100 and _rows_of(off, nxt, kids).size == 300
    assert graph_facts(case("tree:plain"))[2:] == (False, False) and graph_facts(case("tree:back"))[2:] == (True, True)
    # (d): the totals, where they are attained, and who decides WEIGHTED
    want = dict(total_pos=0, total_neg=0, decider_weighted=0, decider_one=0, total_one=0, total_zero=0)
    for n in REDUCTION_SIZES + (1000,):
        for name, what in reduction_cases(n) if n != 1000 else [("reduce:1000:900:998:pos:weighted:x", "total_pos")]:
            flat = case(name)
            _, a, b, *_ = (int(x) if x.isdigit() else x for x in name.split(":")[1:])
            src = np.repeat(np.arange(n), np.diff(flat["offsets"].astype(np.int64)))
            assert np.all(flat["arcs"]["nextstate"] > src), name
            dist = oracle_dist(oracle, flat, True)
            sums = [model.times(d, f) for d, f in zip(dist, flat["finals"])] + [INF] * (n - len(dist))
            total = total_weight(flat, dist, True)
            mid = reweight_ref(flat, dist, True, graph_facts(flat))
            out = push_ref(flat, dist, True, True, graph_facts(flat))
            dec = decider(mid, total)
            removed = not (model.is_one(total) or model.is_zero(total))
            if what in ("total_pos", "total_neg"):
                assert [s for s in range(n) if sums[s] == total] == [a] and removed, name
                assert (total > 0) == (what == "total_pos") and abs(total) > 0.5, (name, total)
                if what == "total_neg":
                    assert (flat["arcs"]["weight"] < 0).any() and (flat["finals"] < 0).any()
            elif what == "total_one":
                assert not removed and abs(total) <= 1 / 2048 and np.isfinite(total), (name, total)
                assert (total != 0) == name.endswith(":e")
            elif what == "total_zero":
                assert total == INF and np.isfinite(flat["finals"]).any(), name
            else:
                assert removed and dec is not None and dec[0] == b, (name, dec)
                assert dec[1] == (what == "decider_weighted"), (name, dec)
                assert bool(out["props"] & model.WEIGHTED) == dec[1], name
                above = [s for s in range(b + 1, n) if np.isfinite(flat["finals"][s])]
                assert above or b == n - 1, name  # final states above the decider: their weights are zero before and after
                if what == "decider_one" and b >= 64:  # another wave would have said WEIGHTED
                    assert any(f is not None and model.weighted(model.divide(f, total)) for f in mid["finals"][:64]), name
            want[what] += 1
            for rt in (0, 1):
                st = expected_counters(flat, ("push", rt, True), dist if rt else oracle_dist(oracle, flat, False),
                                       graph_facts(flat))
                reached.add(("removed", rt, st["removed"]))
    assert all(v >= len(REDUCTION_SIZES) for v in want.values()), want
    for rt in (0, 1):
        for v in (0, 1, 2):
            assert ("removed", rt, v) in reached, (rt, v)
    spots = {n: positions(n) for n in REDUCTION_SIZES}
    assert spots[600] == [2, 255, 325, 599] and spots[257] == [2, 255, 256] and spots[63] == [2, 62] and spots[256] == [2, 255]
    assert positions(600, 16) == [2, 15, 25, 599] and positions(65, 16) == [2, 15, 25, 64]
    # the facts of reweight: the three words differ, and only the chosen arc / final weight is touched
    for n in REDUCTION_SIZES:
        words = {}
        for what, flat, pot in facts_cases(n):
            exp = to_flat(reweight_ref(flat, list(pot), False, graph_facts(flat)))
            changed_arcs = np.nonzero(exp["arcs"]["weight"].view(np.uint32) != flat["arcs"]["weight"].view(np.uint32))[0]
            changed_fin = np.nonzero(exp["finals"].view(np.uint32) != flat["finals"].view(np.uint32))[0]
            kind, _, s = what.partition("@")
            src = np.repeat(np.arange(n), np.diff(flat["offsets"].astype(np.int64)))
            if kind == "arc":
                assert changed_arcs.size and set(src[changed_arcs]) == {int(s)} and not changed_fin.size, what
            elif kind == "final":
                assert list(changed_fin) == [int(s)] and not changed_arcs.size, what
            else:
                assert not changed_arcs.size and not changed_fin.size
            words.setdefault(kind, set()).add(exp["props"])
        assert words["none"] == {FACTS_WORD} and len(words["arc"]) == 1 and len(words["final"]) == 1
        assert len(words["none"] | words["arc"] | words["final"]) == 3


# ================================================================ GPU
def run_call(dev, call):
    import rustfst_amd
    if call[0] == "len":
        return dev.shortest_distance_with_len(reverse=call[1])
    if call[0] == "reweight":
        return dev.reweight(call[2], rustfst_amd.ReweightType(call[1])).to_flat()
    cfg = rustfst_amd.PushWeightsConfig(remove_total_weight=call[2])
    return dev.push_weights(rustfst_amd.ReweightType(call[1]), cfg).to_flat()


def describe(call):
    return f"{call[0]} {call[1]} {call[2] if call[0] == 'push' else len(call[2]) if call[0] == 'reweight' else ''}"


def check_call(gpu_ctx, oracle, flat, dev, call, facts, what, cap=None):
    """one call on the device against the restatement, and its counters against the input"""
    exp, pot = restate(oracle, flat, call, facts)
    got = run_call(dev, call)
    stats = gpu_ctx.push_stats()
    what = f"{what}: {describe(call)}"
    if call[0] == "len":
        dist, ln = got
        assert ln == exp, what
        assert np.all(np.isinf(dist[ln:])), what
        full = to_oracle(oracle, flat).reverse().shortest_distance()[1:] if call[1] else to_oracle(oracle, flat).shortest_distance()
        full = np.r_[full, np.full(flat["n_states"] - len(full), np.inf, dtype=np.float32)][:flat["n_states"]]
        np.testing.assert_array_equal(dist[:ln].view(np.uint32), full[:ln].astype(np.float32).view(np.uint32), err_msg=what)
    else:
        assert_same(got, exp, what)
    assert stats == expected_counters(flat, call, pot, facts, cap), what
    return got, stats


def check_structural(gpu_ctx, oracle, flat, dev, facts, what, cap=None):
    """the device's four facts, as far as a reweight result shows them: the start branch follows INITIAL_CYCLIC, and every
    DFS pair that survives the later masks carries the fact"""
    pairs = ((model.ACCESSIBLE, model.NOT_ACCESSIBLE), (model.COACCESSIBLE, model.NOT_COACCESSIBLE), (model.CYCLIC, model.ACYCLIC),
             (model.INITIAL_CYCLIC, model.INITIAL_ACYCLIC))
    for call in structural_calls(flat):
        got, stats = check_call(gpu_ctx, oracle, flat, dev, call, facts, what, cap)
        assert stats["structural"] == 1 and stats["searches"] == 4, what
        assert stats["start_branch"] == (2 if facts[3] else 1), what
        for (yes, no), fact in zip(pairs, facts):
            if got["props"] & (yes | no):
                assert bool(got["props"] & yes) == fact and bool(got["props"] & no) != fact, (what, hex(got["props"]))


def check_case(gpu_ctx, oracle, name):
    flat = case(name)
    facts = dfs_facts(oracle, flat)
    dev = to_device(flat, gpu_ctx)
    for call in calls_of(flat, 5):
        check_call(gpu_ctx, oracle, flat, dev, call, facts, name)
    check_structural(gpu_ctx, oracle, flat, dev, facts, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", LADDER_CASES)
def test_row_ladder(gpu_ctx, oracle, monkeypatch, name):
    """(a) rows of 0 .. 100 arcs: the 16-lane loops of bfs_round_kernel and reweight_arcs_kernel take up to seven trips"""
    monkeypatch.delenv(KNOB, raising=False)
    check_case(gpu_ctx, oracle, name)
    if name == "ladder:isolated":  # the pairs the searches found are in the word: a lost arc of the peeling would say CYCLIC
        dev = to_device(case(name), gpu_ctx)
        pairs = model.CYCLIC | model.ACYCLIC | model.ACCESSIBLE | model.NOT_ACCESSIBLE | model.INITIAL_CYCLIC | model.INITIAL_ACYCLIC
        for call in structural_calls(case(name)):
            assert run_call(dev, call)["props"] & pairs == model.ACYCLIC | model.NOT_ACCESSIBLE | model.INITIAL_ACYCLIC


@pytest.mark.gpu
@pytest.mark.parametrize("d", CHAIN_DEPTHS)
def test_depth_edges(gpu_ctx, oracle, monkeypatch, d):
    """(b) chains whose searches end on, one before and one after a read of the frontier size, and at the n + 1 stop"""
    monkeypatch.delenv(KNOB, raising=False)
    for name in chain_cases(d):
        check_case(gpu_ctx, oracle, name)
    # the rule by hand for the open chain: the forward length search, and the reversed one over d + 1 states
    dev = to_device(case(f"chain:{d}:open:up"), gpu_ctx)
    for reverse, n in ((False, d), (True, d + 1)):
        assert dev.shortest_distance_with_len(reverse=reverse)[1] == d
        st = gpu_ctx.push_stats()
        rounds, reads = round_rule(n, n)
        assert (st["searches"], st["rounds"], st["reads"], st["rounds_max"]) == (1, rounds, reads, rounds), (d, reverse, st)


@pytest.mark.gpu
@pytest.mark.parametrize("cap", (1, 3))
def test_grid_stride(gpu_ctx, oracle, monkeypatch, cap):
    """(c) WFST_PUSH_MAX_BLOCKS = 1 and 3: frontiers of 100 and 300 states over 16 and 48 state slots, 700 states over the
    same, a total over 1000 states in 256 and 768 lanes; the same results as without the cap"""
    import rustfst_amd
    to_final, remove = rustfst_amd.ReweightType.REWEIGHT_TO_FINAL, rustfst_amd.PushWeightsConfig(remove_total_weight=True)
    for name in STRIDE_CASES:
        flat = case(name)
        facts = dfs_facts(oracle, flat)
        dev = to_device(flat, gpu_ctx)
        for call in [("len", False), ("len", True)] + structural_calls(flat):
            monkeypatch.delenv(KNOB, raising=False)
            free = run_call(dev, call)
            assert gpu_ctx.push_stats()["bfs_blocks"] >= 26
            monkeypatch.setenv(KNOB, str(cap))
            got, st = check_call(gpu_ctx, oracle, flat, dev, call, facts, f"{name}, {cap} blocks", cap)
            assert st["bfs_blocks"] == cap and 16 * st["bfs_blocks"] < 100
            if call[0] == "len":
                assert got[1] == free[1] and np.array_equal(got[0].view(np.uint32), free[0].view(np.uint32))
            else:
                assert_same(got, free, f"{name}: capped against uncapped")
        check_structural(gpu_ctx, oracle, flat, dev, facts, f"{name}, {cap} blocks", cap)
    # reweight_arcs_kernel: 700 states, 16 per block and trip
    flat = case("random:700")
    facts = dfs_facts(oracle, flat)
    dev = to_device(flat, gpu_ctx)
    rng = np.random.default_rng(3)
    calls = [("reweight", rt, potentials(rng, 700, 700, 0, 2.5)) for rt in (0, 1)] + [("push", 0, True), ("push", 1, False)]
    for call in calls:
        monkeypatch.delenv(KNOB, raising=False)
        free = run_call(dev, call)
        assert gpu_ctx.push_stats()["arcs_blocks"] == 44
        monkeypatch.setenv(KNOB, str(cap))
        got, st = check_call(gpu_ctx, oracle, flat, dev, call, facts, f"random 700, {cap} blocks", cap)
        assert st["arcs_blocks"] == cap and 16 * st["arcs_blocks"] < 700
        assert_same(got, free, "random 700: capped against uncapped")
    # total_weight_kernel: 1000 states, the total attained at state 900
    flat = case("reduce:1000:900:998:pos:weighted:x")
    facts = dfs_facts(oracle, flat)
    dev = to_device(flat, gpu_ctx)
    monkeypatch.delenv(KNOB, raising=False)
    free = dev.push_weights(to_final, remove).to_flat()
    assert gpu_ctx.push_stats()["total_blocks"] == 4
    monkeypatch.setenv(KNOB, str(cap))
    got, st = check_call(gpu_ctx, oracle, flat, dev, ("push", 1, True), facts, f"total 1000, {cap} blocks", cap)
    assert st["total_blocks"] == cap and 256 * st["total_blocks"] < 1000 and st["removed"] == 2
    assert_same(got, free, "total 1000: capped against uncapped")


@pytest.mark.gpu
@pytest.mark.parametrize("n", REDUCTION_SIZES)
def test_reductions_across_waves_and_blocks(gpu_ctx, oracle, monkeypatch, n):
    """(d) push to final with remove: the total's minimum and the deciding set_final call in every wave position; the two
    facts bits of reweight from one arc or one final weight in every position"""
    monkeypatch.delenv(KNOB, raising=False)
    for name, what in reduction_cases(n):
        flat = case(name)
        facts = dfs_facts(oracle, flat)
        dev = to_device(flat, gpu_ctx)
        got, st = check_call(gpu_ctx, oracle, flat, dev, ("push", 1, True), facts, f"{name} ({what})")
        assert st["removed"] == (1 if what in ("total_one", "total_zero") else 2), name
        assert st["total_blocks"] == (n + 255) // 256
        if what.startswith("decider"):
            assert bool(got["props"] & model.WEIGHTED) == (what == "decider_weighted"), name
        check_call(gpu_ctx, oracle, flat, dev, ("push", 0, True), facts, name)
    for what, flat, pot in facts_cases(n):
        facts = dfs_facts(oracle, flat)
        dev = to_device(flat, gpu_ctx)
        for rt in (0, 1):
            check_call(gpu_ctx, oracle, flat, dev, ("reweight", rt, pot), facts, f"facts {n} {what}")


@pytest.mark.gpu
def test_counters_on_refusal_and_reuse(gpu_ctx, oracle, monkeypatch):
    """(e) a refused argument leaves every counter 0; a second call on the same handle, which finds the reversed FST cached,
    reports what the first did"""
    import rustfst_amd
    from rustfst_amd import _lib
    monkeypatch.delenv(KNOB, raising=False)
    zero = dict.fromkeys(COUNTERS, 0)
    flat = case("ladder:cyclic")
    facts = dfs_facts(oracle, flat)
    lib, out = _lib.lib(), C.c_void_p()
    busy = structural_calls(flat)[0]

    def fresh():
        dev = to_device(flat, gpu_ctx)
        run_call(dev, busy)
        assert gpu_ctx.push_stats()["searches"] == 4
        return dev
    dev = fresh()
    assert "reweight_type" in helpers.ko_message(lib.wfst_reweight(gpu_ctx._h, dev._h, None, 0, 2, C.byref(out)))
    assert gpu_ctx.push_stats() == zero
    dev = fresh()
    assert "potentials" in helpers.ko_message(lib.wfst_reweight(gpu_ctx._h, dev._h, None, 3, 0, C.byref(out)))
    assert gpu_ctx.push_stats() == zero
    dev = fresh()
    assert "reweight_type" in helpers.ko_message(lib.wfst_push_weights(gpu_ctx._h, dev._h, 7, None, C.byref(out)))
    assert gpu_ctx.push_stats() == zero
    dev = fresh()
    cfg = _lib.ShortestDistanceConfig(1, float("nan"))
    assert "delta" in helpers.ko_message(lib.wfst_shortest_distance_with_config(gpu_ctx._h, dev._h, C.byref(cfg), None, None))
    assert gpu_ctx.push_stats() == zero
    dev = fresh()
    assert "null" in helpers.ko_message(lib.wfst_reweight(gpu_ctx._h, None, None, 0, 0, C.byref(out)))
    assert gpu_ctx.push_stats() == zero
    for value in BAD_KNOB[:4]:
        dev = fresh()
        monkeypatch.setenv(KNOB, value)
        with pytest.raises(rustfst_amd.WfstError, match=KNOB):
            dev.push_weights(rustfst_amd.ReweightType.REWEIGHT_TO_INITIAL)
        assert gpu_ctx.push_stats() == zero
        monkeypatch.delenv(KNOB)
    # reuse: the first call of each kind builds the reversed handle, the second finds it
    for call in (("len", True), ("push", 0, True), busy):
        dev = to_device(flat, gpu_ctx)
        first, st1 = check_call(gpu_ctx, oracle, flat, dev, call, facts, "first call")
        second, st2 = check_call(gpu_ctx, oracle, flat, dev, call, facts, "second call")
        assert st1 == st2 and st1["searches"] >= 1
        if call[0] == "len":
            assert first[1] == second[1] and np.array_equal(first[0].view(np.uint32), second[0].view(np.uint32))
        else:
            assert_same(second, first, "second call against the first")
