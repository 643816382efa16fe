"""The meaning of an FST, by brute force: its weighted relation, for every pair of strings (x, y) the least total weight
of a successful path that reads x and writes y once epsilons are dropped; the specification of every operation as a
statement about relations; and the seeded input families those specifications are checked on.  A helper module: it
imports numpy, oracle.model and helpers, never a test module and never the library under test.  Nothing here knows of
filters, queues, state numbering or property words (the families state a word, because the device trusts it; the
evaluator never reads it).

The exactness rule.  Every arc weight and final weight of every input built here is a multiple of 1/4 of magnitude below
4 (assert_exact, called on every input), and no compared path has more than 2^16 arcs.  Every partial sum is then an
integer multiple of 1/4 of magnitude below 2^24 / 4, which f32 and f64 both hold exactly: sums are exact in any order,
and so are the differences that push_weights, reweight and the weight division take.  The grid step is 256 times KDELTA
(1/1024), so approx_eq never merges two different weights.  Hence every comparison of relations is == on float64
values, with no tolerance, and Python's -0.0 == 0.0 is what is wanted."""
import collections
import functools
import itertools

import numpy as np

from oracle.model import ACCEPTOR, ALL, content_word_of_flat
from oracle.model.props import NOT_I_LABEL_SORTED, NOT_O_LABEL_SORTED
from helpers import P, TR_DTYPE, random_fst_flat

INF = float("inf")
GRID = 4            # weights are multiples of 1 / GRID
MAX_ARCS = 1 << 16  # the longest path the exactness rule covers
EPS = ()


# ================================================================ the evaluator
def strings(sigma, L):
    """all label tuples over 1..sigma of length at most L, shortest first"""
    return [t for k in range(L + 1) for t in itertools.product(range(1, sigma + 1), repeat=k)]


S = strings(2, 3)  # 15 strings, 225 pairs


class _Trie:
    """the prefixes of a set of strings: node 0 is the empty prefix; step[a] = (nodes with a child by a, those children)"""

    def __init__(self, strs):
        nodes = sorted({tuple(s[:k]) for s in strs for k in range(len(s) + 1)}, key=lambda t: (len(t), t))
        self.index = {t: i for i, t in enumerate(nodes)}
        self.size = len(nodes)
        step = collections.defaultdict(lambda: ([], []))
        for t, i in self.index.items():
            if t:
                step[t[-1]][0].append(self.index[t[:-1]])
                step[t[-1]][1].append(i)
        self.step = {a: (np.array(f), np.array(t)) for a, (f, t) in step.items()}
        self.step[0] = (np.arange(self.size), np.arange(self.size))


@functools.lru_cache(maxsize=None)
def _trie(strs):
    return _Trie(strs)


def _has_no_start(flat):
    return flat["n_states"] == 0 or flat["start"] is None or flat["start"] < 0


def relation(flat, xs=S, ys=S):
    """{(x, y): weight} over xs x ys in float64, finite entries only.  Bellman-Ford to a fixed point over the nodes
    (state, prefix of some x read, prefix of some y written): an arc advances the input prefix by its ilabel (0: stays),
    the output prefix by its olabel.  Cycles, epsilon cycles and any state numbering are fine; negative weights only on
    acyclic inputs (the fixed point is asserted to be reached)."""
    if _has_no_start(flat):
        return {}
    tx, ty = _trie(tuple(map(tuple, xs))), _trie(tuple(map(tuple, ys)))
    n, off = flat["n_states"], flat["offsets"]
    arcs = []
    for s in range(n):
        for a in flat["arcs"][off[s]:off[s + 1]]:
            il, ol = int(a["ilabel"]), int(a["olabel"])
            if il in tx.step and ol in ty.step and np.isfinite(a["weight"]):
                fi, ti = tx.step[il]
                fo, to = ty.step[ol]
                arcs.append((s, int(a["nextstate"]), float(a["weight"]), np.ix_(fi, fo), np.ix_(ti, to)))
    d = np.full((n, tx.size, ty.size), INF)
    d[int(flat["start"]), 0, 0] = 0.0
    for _ in range(n * tx.size * ty.size + 2):
        changed = False
        for s, ns, w, src, dst in arcs:
            cand = d[s][src] + w
            cur = d[ns][dst]
            if (cand < cur).any():
                d[ns][dst] = np.minimum(cand, cur)
                changed = True
        if not changed:
            break
    else:
        raise AssertionError("no fixed point: a negative cycle")
    tot = (d + flat["finals"].astype(np.float64)[:, None, None]).min(axis=0)
    return {(tuple(x), tuple(y)): float(tot[tx.index[tuple(x)], ty.index[tuple(y)]]) for x in xs for y in ys
            if np.isfinite(tot[tx.index[tuple(x)], ty.index[tuple(y)]])}


class Machine:
    """what weight_of walks: start, arcs(state) -> [(ilabel, olabel, weight, nextstate)], final(state); states hashable"""

    def __init__(self, flat):
        self.start = None if _has_no_start(flat) else int(flat["start"])
        off, a = flat["offsets"], flat["arcs"]
        cols = [a["ilabel"].tolist(), a["olabel"].tolist(), a["weight"].astype(np.float64).tolist(), a["nextstate"].tolist()]
        self.rows = [list(zip(*[c[off[s]:off[s + 1]] for c in cols])) for s in range(flat["n_states"])]
        self.finals = flat["finals"].astype(np.float64).tolist()

    def arcs(self, s):
        return self.rows[s]

    def final(self, s):
        return self.finals[s]


class Product:
    """naive_product without building it: the same three rules, arcs made when asked for (for operands too large to
    multiply out)"""

    def __init__(self, a, b):
        self.a, self.b = as_machine(a), as_machine(b)
        self.start = None if self.a.start is None or self.b.start is None else (self.a.start, self.b.start)
        self._by_ilabel = {}

    def _match(self, sb):
        m = self._by_ilabel.get(sb)
        if m is None:
            m = collections.defaultdict(list)
            for arc in self.b.arcs(sb):
                m[arc[0]].append(arc)
            self._by_ilabel[sb] = m
        return m

    def arcs(self, s):
        sa, sb = s
        mb = self._match(sb)
        out = [(0, ol, w, (sa, ns)) for _, ol, w, ns in mb.get(0, ())]
        for il, c, w, ns in self.a.arcs(sa):
            if c == 0:
                out.append((il, 0, w, (ns, sb)))
            else:
                out.extend((il, ol, w + w2, (ns, ns2)) for _, ol, w2, ns2 in mb.get(c, ()))
        return out

    def final(self, s):
        return self.a.final(s[0]) + self.b.final(s[1])


def as_machine(m):
    return Machine(m) if isinstance(m, dict) else m


def weight_of(m, x, y):
    """relation(m, [x], [y]) for one pair, on a flat FST or a Machine, visiting only the nodes the pair reaches (a
    label-correcting search; non-negative weights where the machine is cyclic).  For inputs too large for all pairs."""
    m = as_machine(m)
    if m.start is None:
        return INF
    x, y = tuple(x), tuple(y)
    nx, ny = len(x), len(y)
    dist = {(m.start, 0, 0): 0.0}
    queue, queued = collections.deque(dist), set(dist)
    best, steps = INF, 0
    while queue:
        node = queue.popleft()
        queued.discard(node)
        s, i, j = node
        d = dist[node]
        xi = x[i] if i < nx else -1
        yj = y[j] if j < ny else -1
        for il, ol, w, ns in m.arcs(s):
            if (il == 0 or il == xi) and (ol == 0 or ol == yj) and w != INF:
                t = (ns, i + (il != 0), j + (ol != 0))
                v = d + w
                if v < dist.get(t, INF):
                    dist[t] = v
                    if t not in queued:
                        queued.add(t)
                        queue.append(t)
        steps += 1
        assert steps < 50_000_000, "weight_of does not settle: a negative cycle?"
    for (s, i, j), d in dist.items():
        if i == nx and j == ny:
            best = min(best, d + m.final(s))
    return best


def distances(flat, reverse=False):
    """float64 Bellman-Ford on the machine itself: the distance from the start state to every state (reverse: from every
    state to the final states), +inf where there is no path"""
    n = flat["n_states"]
    d = np.full(n, INF)
    if n == 0:
        return d
    src = np.repeat(np.arange(n), np.diff(flat["offsets"].astype(np.int64)))
    dst = flat["arcs"]["nextstate"].astype(np.int64)
    w = flat["arcs"]["weight"].astype(np.float64)
    if reverse:
        d = flat["finals"].astype(np.float64).copy()
        src, dst = dst, src
    elif _has_no_start(flat):
        return d
    else:
        d[int(flat["start"])] = 0.0
    for _ in range(n + 1):
        new = d.copy()
        np.minimum.at(new, dst, d[src] + w)
        if np.array_equal(new, d):
            return d
        d = new
    raise AssertionError("no fixed point: a negative cycle")


def best_total(flat):
    """the least weight of any successful path: min over states of d[s] + final[s]"""
    if _has_no_start(flat):
        return INF
    return float((distances(flat) + flat["finals"].astype(np.float64)).min())


def make(n, start, rows, finals, props=0):
    """flat FST from rows[s] = [(ilabel, olabel, weight, nextstate)]"""
    off = np.zeros(n + 1, np.uint32)
    off[1:] = np.cumsum([len(r) for r in rows]) if n else []
    flat_rows = [tuple(a) for r in rows for a in r]
    arcs = np.array(flat_rows, dtype=TR_DTYPE) if flat_rows else np.zeros(0, TR_DTYPE)
    finals = np.asarray(finals, np.float32).reshape(n)
    return dict(n_states=n, start=start, offsets=off, arcs=arcs, finals=finals, props=props)


def naive_product(a, b):
    """Composition by definition, no filter and no matcher, over the states (sa, sb) the start pair reaches: an arc of
    `a` with olabel 0 moves alone and writes 0; an arc of `b` with ilabel 0 moves alone and reads 0; an arc of `a` with
    olabel c != 0 pairs with every arc of `b` with ilabel c.  Weights and final weights are added in float64 (and stored
    as f32, which the exactness rule makes lossless).  Redundant epsilon paths are harmless: min is idempotent."""
    p = Product(a, b)
    if p.start is None:
        return make(0, None, [], [])
    ids, order, rows = {p.start: 0}, [p.start], []
    k = 0
    while k < len(order):
        row = []
        for il, ol, w, t in p.arcs(order[k]):
            if t not in ids:
                ids[t] = len(order)
                order.append(t)
            row.append((il, ol, w, ids[t]))
        rows.append(row)
        k += 1
    return make(len(order), 0, rows, [p.final(s) for s in order])


# ================================================================ the specifications
def shifted(R, c):
    return {k: w - c for k, w in R.items()}


def reversed_rel(R):
    return {(x[::-1], y[::-1]): w for (x, y), w in R.items()}


def inverted_rel(R):
    return {(y, x): w for (x, y), w in R.items()}


def projected_rel(R, output):
    """{(x, x): min over y of R(x, y)} (output: over x, on y), from a relation whose other side is long enough"""
    out = {}
    for (x, y), w in R.items():
        k = y if output else x
        out[(k, k)] = min(w, out.get((k, k), INF))
    return out


def union_rel(*Rs):
    out = {}
    for R in Rs:
        for k, w in R.items():
            out[k] = min(w, out.get(k, INF))
    return out


def _splits(x, y):
    return [((x[:i], y[:j]), (x[i:], y[j:])) for i in range(len(x) + 1) for j in range(len(y) + 1)]


def concat_rel(Ra, Rb, strs=S):
    """min over all splits x = x1 x2, y = y1 y2 of Ra(x1, y1) + Rb(x2, y2); strs is closed under prefix and suffix"""
    out = {}
    for x in strs:
        for y in strs:
            w = min((Ra[l] + Rb[r] for l, r in _splits(x, y) if l in Ra and r in Rb), default=INF)
            if w != INF:
                out[(x, y)] = w
    return out


def closure_rel(R, star, strs=S):
    """plus: P(x, y) = min(R(x, y), min over splits with both parts != (eps, eps) of R(x1, y1) + P(x2, y2)), filled in
    order of len(x) + len(y); star: P with (eps, eps) -> 0.0.  Non-negative weights (a turn that reads and writes nothing
    cannot help)."""
    assert all(w >= 0 for w in R.values())
    P_ = {}
    for x, y in sorted(((x, y) for x in strs for y in strs), key=lambda k: len(k[0]) + len(k[1])):
        w = R.get((x, y), INF)
        for l, r in _splits(x, y):
            if l != (EPS, EPS) and r != (EPS, EPS) and l in R and r in P_:
                w = min(w, R[l] + P_[r])
        if w != INF:
            P_[(x, y)] = w
    if star:
        P_[(EPS, EPS)] = 0.0
    return P_


def projection_spec(flat, output):
    """the relation project(flat) must have over S x S: {(x, x): min over every y of R(x, y)} (output: over every x, on
    y).  The minimum over a side of any length is taken by brute force on the input with that side's tape ignored (its
    labels read as 0), which is exact on cyclic inputs too."""
    f = dict(flat, arcs=flat["arcs"].copy())
    f["arcs"]["ilabel" if output else "olabel"] = 0
    R = relation(f, [EPS], S) if output else relation(f, S, [EPS])
    return {((y, y) if output else (x, x)): w for (x, y), w in R.items()}


def path_of(flat):
    """(weight left-folded in f32 as float, ilabels stripped, olabels stripped) of a result of shortest_path(n = 1): one
    linear path from the start state to a final state; None for the empty FST"""
    if _has_no_start(flat):
        assert flat["n_states"] == 0 or not np.isfinite(flat["finals"]).any()
        return None
    m = Machine(flat)
    s, w, x, y, seen = m.start, np.float32(0.0), [], [], set()
    while True:
        assert s not in seen, "the path result has a cycle"
        seen.add(s)
        row = m.arcs(s)
        if np.isfinite(flat["finals"][s]):
            assert not row, "the path goes on behind its final state"
            w = np.float32(w + flat["finals"][s])
            break
        assert len(row) == 1, "a path result has one arc per state"
        il, ol, aw, ns = row[0]
        w = np.float32(w + np.float32(aw))
        x += [il] if il else []
        y += [ol] if ol else []
        s = ns
    assert len(seen) == flat["n_states"], "states beside the path"
    return float(w), tuple(x), tuple(y)


def check_shortest_path(result, inp, what=""):
    """shortest_path (n = 1): the empty result iff best_total is +inf; otherwise one path whose left-folded weight is
    best_total(input) and whose own label strings have that weight in the input"""
    total = best_total(inp)
    p = path_of(result)
    if total == INF:
        assert p is None, f"{what}: a path where the input accepts nothing"
        return
    assert p is not None, f"{what}: no path, the input's best is {total}"
    w, x, y = p
    assert w == total, f"{what}: path weight {w}, best total {total}"
    got = weight_of(inp, x, y)
    assert got == w, f"{what}: the input gives {x} / {y} weight {got}, the path says {w}"


# ---------------------------------------------------------------- properties of a result alone
def no_eps_eps_arc(flat):
    a = flat["arcs"]
    return not np.any((a["ilabel"] == 0) & (a["olabel"] == 0))


def input_deterministic(flat, eps_is_label=False):
    """no state has two arcs with one ilabel, and none with ilabel 0: every string is accepted along one path.
    eps_is_label: 0 counts as a label like any other, as determinize itself reads it on an input with epsilons"""
    off = flat["offsets"]
    for s in range(flat["n_states"]):
        il = flat["arcs"]["ilabel"][off[s]:off[s + 1]]
        if len(set(il.tolist())) != len(il) or (np.any(il == 0) and not eps_is_label):
            return False
    return True


def top_sorted(flat):
    src = np.repeat(np.arange(flat["n_states"]), np.diff(flat["offsets"].astype(np.int64)))
    return bool(np.all(flat["arcs"]["nextstate"].astype(np.int64) > src))


def connected(flat):
    """every state accessible and coaccessible, by a plain BFS both ways"""
    n = flat["n_states"]
    if n == 0:
        return True
    if _has_no_start(flat):
        return False
    off, nxt = flat["offsets"], flat["arcs"]["nextstate"]
    fwd = [[int(t) for t in nxt[off[s]:off[s + 1]]] for s in range(n)]
    bwd = [[] for _ in range(n)]
    for s in range(n):
        for t in fwd[s]:
            bwd[t].append(s)

    def bfs(seeds, adj):
        seen, queue = set(seeds), collections.deque(seeds)
        while queue:
            for t in adj[queue.popleft()]:
                if t not in seen:
                    seen.add(t)
                    queue.append(t)
        return seen
    finals = [s for s in range(n) if np.isfinite(flat["finals"][s])]
    return len(bfs([int(flat["start"])], fwd)) == n and len(bfs(finals, bwd)) == n


def pushed_to_initial(flat, at_start=0.0):
    """at every state that reaches a final state, min(out-arc weights into such states, final weight) == 0.0; at the start
    state == at_start"""
    rd = distances(flat, reverse=True)
    off = flat["offsets"]
    for s in range(flat["n_states"]):
        if rd[s] == INF:
            continue
        a = flat["arcs"][off[s]:off[s + 1]]
        ws = [float(w) for w, t in zip(a["weight"], a["nextstate"]) if rd[int(t)] != INF]
        if min(ws + [float(flat["finals"][s])]) != (at_start if s == flat["start"] else 0.0):
            return False
    return True


# ================================================================ the input families
def assert_exact(flat):
    """the exactness rule on one input: every arc and final weight a multiple of 1/4 of magnitude below 4"""
    for w in (flat["arcs"]["weight"].astype(np.float64), flat["finals"].astype(np.float64)):
        w = w[np.isfinite(w)]
        assert np.all(w * GRID == np.round(w * GRID)) and np.all(np.abs(w) < 4), "off the quarter grid"
    assert not np.any(np.isnan(flat["finals"])) and np.all(np.isfinite(flat["arcs"]["weight"]))
    assert flat["n_states"] < MAX_ARCS
    return flat


def _label_sort_word(flat):
    off = flat["offsets"]
    rows = [flat["arcs"][off[s]:off[s + 1]] for s in range(flat["n_states"])]
    il = all(np.all(np.diff(r["ilabel"].astype(np.int64)) >= 0) for r in rows)
    ol = all(np.all(np.diff(r["olabel"].astype(np.int64)) >= 0) for r in rows)
    return (P.I_LABEL_SORTED if il else NOT_I_LABEL_SORTED) | (P.O_LABEL_SORTED if ol else NOT_O_LABEL_SORTED)


def with_word(flat, acyclic):
    """the property word: computed from the content on acyclic inputs (every pair known), label sortedness alone on
    cyclic ones (what random_fst_flat states)"""
    flat["props"] = content_word_of_flat(flat) & ALL if acyclic else _label_sort_word(flat)
    return flat


def negate_some(rng, flat):
    """the same machine with every weight redrawn from {-8/4 .. 11/4} (acyclic inputs only)"""
    f = dict(flat, arcs=flat["arcs"].copy(), finals=flat["finals"].copy())
    f["arcs"]["weight"] = rng.integers(-8, 12, len(f["arcs"])) / GRID
    fin = np.isfinite(f["finals"])
    f["finals"][fin] = rng.integers(-8, 12, int(fin.sum())) / GRID
    return f


# Measured on the input side by the brute force alone (24 seeds each; the tests assert the bounds: at least 60 % of a
# family with 3 pairs or more, an empty relation and one with (eps, eps) in every family, a non-empty product for at
# least half of the compose pairs):
#   family        >= 3 pairs   empty   with (eps, eps)      compose pairs with a non-empty product
#   cyclic            83 %        2         12                   71 %
#   acyclic           71 %        1         15                   96 %
#   acceptor          71 %        1         13
#   acyclic_neg       83 %        1         17                   88 %
#   acceptor_neg      67 %        1         15
#   cyclic_oeps       75 %        2         13
FAMILIES = ("cyclic", "acyclic", "acceptor", "acyclic_neg", "acceptor_neg", "cyclic_oeps")
SEEDS = 24


@functools.lru_cache(maxsize=None)
def small(family, seed, sort="ilabel", min_fanout=1):
    """one small input: 2..8 states (acyclic: 2..7), labels 1..2, epsilons on both sides except in the acceptors
    (cyclic_oeps: on the output side only, what the string kernel of the fused batch takes), weights on the quarter grid;
    seed 0 of every family accepts nothing (no final state), seed 1 has a final start state"""
    rng = np.random.default_rng(1000 * (1 + FAMILIES.index(family)) + seed)
    acyclic = not family.startswith("cyclic")
    n = int(rng.integers(2, 8 if acyclic else 9))
    if family.startswith("acceptor"):
        f = random_fst_flat(rng, n, 4, 2, p_final=0.6, sort=sort, weight_grid=GRID, max_w=12, acyclic=True,
                            min_fanout=min_fanout)
        f["arcs"]["olabel"] = f["arcs"]["ilabel"]
    else:
        p_eps_i = 0.0 if family == "cyclic_oeps" else float(rng.choice([0.2, 0.3]))
        f = random_fst_flat(rng, n, 3, 2, p_eps_i=p_eps_i, p_eps_o=float(rng.choice([0.2, 0.3])), p_final=0.5,
                            sort=sort, weight_grid=GRID, max_w=12, acyclic=acyclic, min_fanout=min_fanout)
    if acyclic:
        f["finals"][n - 1] = float(rng.integers(0, 12)) / GRID  # the last state, where every full walk ends
    if family.endswith("_neg"):
        f = negate_some(rng, f)
    if seed == 0:
        f["finals"][:] = np.inf
    if seed == 1:
        f["finals"][0] = 0.5  # a final start state: (eps, eps) is in the relation
    return assert_exact(with_word(f, acyclic))


def family(name, sort="ilabel", min_fanout=1):
    return [small(name, seed, sort, min_fanout) for seed in range(SEEDS)]


@functools.lru_cache(maxsize=None)
def small_relation(family, seed, sort="ilabel", min_fanout=1):
    return relation(small(family, seed, sort, min_fanout))


def compose_pair(family, seed):
    """(a, b) of one family: a's arcs sorted by olabel, b's by ilabel, at least two arcs per state (acyclic: where there is
    a later state)"""
    return small(family, seed, "olabel", 2), small(family, 100 + seed, "ilabel", 2)


def string_acceptor(labels):
    """the linear acceptor of a string, weight 0"""
    L = len(labels)
    rows = [[(int(a), int(a), 0.0, i + 1)] for i, a in enumerate(labels)] + [[]]
    return with_word(make(L + 1, 0, rows, [np.inf] * L + [0.0]), True)


def vacuity(relations):
    """(share of cases with at least 3 pairs, cases with an empty relation, cases with (eps, eps))"""
    rs = list(relations)
    return (sum(len(r) >= 3 for r in rs) / len(rs), sum(not r for r in rs), sum((EPS, EPS) in r for r in rs))


def assert_not_vacuous(relations, what, share=0.6, need_empty=True):
    big, empty, epseps = vacuity(relations)
    assert big >= share, f"{what}: only {big:.0%} of the inputs have 3 pairs or more"
    assert empty >= 1 or not need_empty, f"{what}: no input with an empty relation"
    assert epseps >= 1, f"{what}: no input with (eps, eps)"
    return big, empty, epseps


# ---------------------------------------------------------------- the mid-size family
LATTICE_WIDTHS = (1, 17, 280, 300, 40, 8, 1)  # 647 states in layers; two layers wider than 256
LATTICE_SIGMA = 8


@functools.lru_cache(maxsize=None)
def lattice(seed=0, acceptor=True):
    """An acyclic lattice in layers: the start state has 300 arcs into the 17 states of the next layer (duplicate
    (ilabel, olabel, nextstate) keys by the pigeonhole: above the rank limit 256 of tr_sum and tr_sort), state 1 has
    exactly 17 arcs, every other state 1..4 and what it takes to give every state an arc from the layer before it; about
    10 % of the arcs are 0:0; an arc goes to the next layer (a 0:0 arc
    sometimes one further); quarter-grid weights; the last layer is final, and a few states before it."""
    rng = np.random.default_rng(7700 + seed)
    base = np.concatenate([[0], np.cumsum(LATTICE_WIDTHS)])
    n = int(base[-1])
    rows = []
    for layer, width in enumerate(LATTICE_WIDTHS):
        for k in range(width):
            s = int(base[layer]) + k
            if layer + 1 == len(LATTICE_WIDTHS):
                rows.append([])
                continue
            deg = 300 if s == 0 else (17 if s == 1 else int(rng.integers(1, 5)))
            row = []
            for _ in range(deg):
                eps = rng.random() < 0.1
                lab = 0 if eps else int(rng.integers(1, LATTICE_SIGMA + 1))
                to = layer + 1 + (1 if eps and layer + 2 < len(LATTICE_WIDTHS) and rng.random() < 0.3 else 0)
                first = s == 0 and len(row) < LATTICE_WIDTHS[1]  # (the start state's first arcs: one into every state)
                t = int(base[to]) + (len(row) if first else int(rng.integers(0, LATTICE_WIDTHS[to])))
                ol = lab if acceptor or eps else int(rng.integers(1, LATTICE_SIGMA + 1))
                row.append((lab, ol, float(rng.integers(0, 12)) / GRID, t))
            rows.append(row)
    # every state has an arc from the layer before it, so the layers are the levels of a topological peeling too
    fed = {(a[3]) for layer in range(len(LATTICE_WIDTHS) - 1) for s in range(int(base[layer]), int(base[layer + 1]))
           for a in rows[s] if a[3] < base[layer + 2]}
    for layer in range(2, len(LATTICE_WIDTHS)):
        for t in range(int(base[layer]), int(base[layer + 1])):
            if t not in fed:
                s = int(rng.integers(max(int(base[layer - 1]), 2), int(base[layer])))
                lab = int(rng.integers(1, LATTICE_SIGMA + 1))
                ol = lab if acceptor else int(rng.integers(1, LATTICE_SIGMA + 1))
                rows[s].append((lab, ol, float(rng.integers(0, 12)) / GRID, t))
    finals = np.full(n, np.inf, np.float32)
    finals[n - 1] = 0.25
    for s in rng.integers(int(base[3]), n - 1, 12):
        finals[int(s)] = float(rng.integers(0, 12)) / GRID
    f = make(n, 0, rows, finals)
    assert max(LATTICE_WIDTHS) > 256 and len(rows[0]) == 300 and len(rows[1]) == 17
    assert len({(a[0], a[1], a[3]) for a in rows[0]}) < 300
    return assert_exact(with_word(f, True))


@functools.lru_cache(maxsize=None)
def mid_transducer(seed=0):
    """a cyclic transducer of 200 states over the lattice's labels, epsilons on both sides, arcs sorted by ilabel"""
    rng = np.random.default_rng(7800 + seed)
    f = random_fst_flat(rng, 200, 6, LATTICE_SIGMA, p_eps_i=0.1, p_eps_o=0.2, p_final=0.5, sort="ilabel", weight_grid=GRID,
                        max_w=12, min_fanout=3)
    return assert_exact(with_word(f, False))


def successful_walk(rng, m, max_steps=64):
    """the label strings (x, y) of a random walk from the start state that ends in a final state, preferring to stop there;
    None when the walk dies"""
    m = as_machine(m)
    s, x, y = m.start, [], []
    if s is None:
        return None
    for _ in range(max_steps):
        row = m.arcs(s)
        if m.final(s) != INF and (not row or rng.random() < 0.5):
            return tuple(x), tuple(y)
        if not row:
            return None
        il, ol, _, s = row[int(rng.integers(0, len(row)))]
        x += [il] if il else []
        y += [ol] if ol else []
    return None


def sample_pairs(rng, machines, n_walks=48, n_random=16, sigma=LATTICE_SIGMA):
    """n_walks string pairs read off successful random walks (in turn over `machines`), finite by construction, and
    n_random uniform random pairs of the same lengths, mostly rejected"""
    walks, tries = [], 0
    while len(walks) < n_walks:
        p = successful_walk(rng, machines[tries % len(machines)])
        tries += 1
        assert tries < 100 * n_walks, "the walks find no successful path"
        if p is not None:
            walks.append(p)
    rand = []
    for k in range(n_random):
        x, y = walks[k % len(walks)]
        rx = tuple(int(v) for v in rng.integers(1, sigma + 1, len(x)))
        rand.append((rx, rx if x == y else tuple(int(v) for v in rng.integers(1, sigma + 1, len(y)))))
    return walks + rand


# ================================================================ operations: inputs, specification, postconditions
COMPOSE_FILTERS = ("AUTOFILTER", "TRIVIALFILTER", "SEQUENCEFILTER", "ALTSEQUENCEFILTER", "MATCHFILTER")
# (NULLFILTER refuses the matcher's implicit epsilon loops, null_compose_filter.rs:122-129: an epsilon of one side never
# moves alone, which is not composition by definition; it is tried on the acceptors, which have no epsilons.
# NOMATCHFILTER refuses epsilon:epsilon matches and is left out.)
_ANY = ("cyclic", "acyclic", "acyclic_neg")
_DAG = ("acyclic", "acceptor", "acyclic_neg", "acceptor_neg")
_POS = ("cyclic", "acyclic")
_ACC = ("acceptor", "acceptor_neg")
OPS = {  # operation -> the families it is tried on (each call only on inputs it supports)
    "rm_epsilon": _ANY, "tr_sum": _ANY, "tr_unique": _ANY, "connect": _ANY, "state_sort": _ANY, "tr_sort_i": _ANY,
    "tr_sort_o": _ANY,
    "reverse": _ANY, "invert": _ANY, "project_i": _ANY, "project_o": _ANY,
    "optimize": _DAG, "top_sort": _DAG, "determinize": _ACC, "minimize": _ACC,
    "reweight_i": _ANY, "reweight_f": _ANY, "push_i": _POS, "push_f": _POS, "push_i_total": _POS, "push_f_total": _POS,
    "union": _ANY, "concat": _ANY, "union_list": _ANY, "concat_list": _ANY, "closure_plus": _POS, "closure_star": _POS,
    "lookahead": _ANY,
}
OPS.update({"compose_" + f: _ANY for f in COMPOSE_FILTERS})
OPS["compose_NULLFILTER"] = _ACC
SAME = {"rm_epsilon", "tr_sum", "tr_unique", "optimize", "connect", "top_sort", "state_sort", "tr_sort_i", "tr_sort_o",
        "determinize", "minimize", "reweight_i", "reweight_f", "push_i", "push_f"}
CASES = [(op, fam) for op, fams in OPS.items() for fam in fams]


def inputs_of(op, fam, seed):
    """(the operand FSTs, the extra argument or None) of one case"""
    rng = np.random.default_rng(50_000 + seed)
    if op.startswith("compose_") or op == "lookahead":
        return list(compose_pair(fam, seed)), None
    if op in ("union", "concat"):
        return [small(fam, seed), small(fam, 100 + seed)], None
    if op in ("union_list", "concat_list"):
        return [small(fam, seed), small(fam, 100 + seed), small(fam, 200 + seed)], None
    f = small(fam, seed, "none") if op.startswith("tr_sort") else small(fam, seed)
    if op == "minimize":
        from oracle.model import determinize_ref
        return [determinize_ref(f)], None
    if op == "state_sort":
        return [f], rng.permutation(f["n_states"]).astype(np.uint32)
    if op.startswith("reweight"):
        return [f], (rng.integers(0, 12, f["n_states"]) / GRID).astype(np.float32)
    return [f], None


def expected(op, ins):
    """the relation over S x S the result of `op` on `ins` must have (section 2 of the issue, one line each)"""
    R = relation(ins[0])
    if op in SAME:
        return R
    if op in ("push_i_total", "push_f_total"):
        # push.rs:120-142 as oracle/model/push.py restates it: ToInitial divides the start state's arcs and final weight by
        # the reverse distance of the start state, ToFinal every final weight by the sum over states of distance * final
        # weight; either is the weight of the best successful path, and every successful path loses it once
        total = best_total(ins[0])
        return R if total in (0.0, INF) else shifted(R, total)
    if op == "reverse":
        return reversed_rel(R)
    if op == "invert":
        return inverted_rel(R)
    if op in ("project_i", "project_o"):
        return projection_spec(ins[0], op == "project_o")
    if op in ("union", "union_list"):
        return union_rel(*[relation(f) for f in ins])
    if op in ("concat", "concat_list"):
        return functools.reduce(concat_rel, [relation(f) for f in ins])
    if op in ("closure_plus", "closure_star"):
        return closure_rel(R, op == "closure_star")
    if op.startswith("compose_") or op == "lookahead":
        return relation(naive_product(*ins))
    raise KeyError(op)


def postconditions(op, ins, out):
    """properties of the result alone"""
    if op == "rm_epsilon":
        assert no_eps_eps_arc(out), "rm_epsilon left a 0:0 arc"
    if op == "determinize":
        eps_in = bool(np.any(ins[0]["arcs"]["ilabel"] == 0))
        assert input_deterministic(out, eps_in), "determinize: two arcs of one state share a label"
    if op == "minimize":
        assert out["n_states"] <= ins[0]["n_states"], "minimize added states"
    if op == "top_sort":
        assert top_sorted(out), "top_sort: an arc does not go forward"
    if op == "connect":
        assert connected(out), "connect left a state that is not accessible and coaccessible"
    if op in ("push_i", "push_i_total"):
        # the start state keeps the total weight (reweight.rs:105-146) unless remove_total_weight takes it off again
        total = best_total(ins[0])
        assert pushed_to_initial(out, total if op == "push_i" and total != INF else 0.0), \
            "push to_initial: a state whose least out-weight is not 0.0"


def supported(op, ins):
    """optimize hands a transducer that rm_epsilon and tr_sum leave input-deterministic to minimize, which this project
    refuses for transducers (wfst.h): such inputs are outside what the call supports"""
    if op != "optimize" or ins[0]["props"] & ACCEPTOR:
        return True
    from oracle import oracle_py
    from oracle.model.optimize import branch_of
    return branch_of(ins[0], oracle_py) != "min"


@functools.lru_cache(maxsize=None)
def seeds_for(op, fam, count=SEEDS):
    """the first `count` seeds whose inputs the operation supports"""
    out, seed = [], 0
    while len(out) < count:
        if supported(op, inputs_of(op, fam, seed)[0]):
            out.append(seed)
        seed += 1
        assert seed < 100, "the family has too few supported inputs"
    return tuple(out)


def check_case(op, fam, seed, apply):
    """one case: apply(op, ins, extra) -> the result's flat form; its relation must equal the specification exactly"""
    ins, extra = inputs_of(op, fam, seed)
    out = apply(op, ins, extra)
    want, got = expected(op, ins), relation(out)
    assert got == want, f"{op} on {fam} seed {seed}: " + diff(got, want)
    postconditions(op, ins, out)
    return want


def diff(got, want):
    keys = sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))
    shown = "; ".join(f"{k}: result {got.get(k)}, specification {want.get(k)}" for k in keys[:6])
    return shown + f" ({len(keys)} pairs differ)"


def check_string_path(result, x, t, what=""):
    """one item of compose_shortest_path_batch(accs, t): the path reads x, its weight is best_total of the product of x's
    acceptor with t by definition, and its output string y has that weight with x in t"""
    total = best_total(naive_product(string_acceptor(x), t))
    p = path_of(result)
    if total == INF:
        assert p is None, f"{what}: a path where t does not accept the string"
        return False
    assert p is not None, f"{what}: no path, the product's best is {total}"
    w, px, py = p
    assert px == tuple(x), f"{what}: the path reads {px}"
    assert w == total, f"{what}: path weight {w}, best total {total}"
    assert weight_of(t, px, py) == w, f"{what}: t gives {px} / {py} weight {weight_of(t, px, py)}, the path says {w}"
    return True
