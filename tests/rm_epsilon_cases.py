"""rm_epsilon: the retry ladder of the kernels restated once, the model that predicts a call's needs and counters,
and the input families that more than one test module uses."""
import numpy as np

from rustfst_amd._lib import TR_DTYPE

from oracle.model import F32, INF
from helpers import P, random_fst_flat

# The retry ladder of rm_epsilon_fst, restated once (rustfst_amd/csrc/rm_epsilon.hip, the attempt loop of rm_epsilon_fst:
# `RmCaps caps{16, 32, 32}`, `RmBigCaps big{1024, 1024, 1024}`, `const bool wave = caps.C > 64`, every size times 4 per
# retry).  A state finishes in the first rung whose (C, K, A) hold its closure, its largest stack occupancy and its arcs.
THREAD_RUNGS = ((16, 32, 32), (64, 128, 128))
WAVE_FIRST = (1024, 1024, 1024)
GROWTH = 4
STAT_KEYS = ("batches", "thread_launches", "wave_launches", "states_thread", "states_wave", "max_closure_cap")


def rungs():
    for caps in THREAD_RUNGS:
        yield "thread", caps
    caps = WAVE_FIRST
    while True:
        yield "wave", caps
        caps = tuple(c * GROWTH for c in caps)


def _eps(t):
    return t[0] == 0 and t[1] == 0


def _rewrite(cur, finals, s):
    """RmEpsilonState::expand of state s over the arc lists as they are now: (arcs, final weight, (C, K, A))"""
    # the closure in reverse post-order of the epsilon arcs (acyclic: a topological order), then one relaxation pass:
    # f32 addition is monotone, so this is the exact minimum over the paths of the left-folded f32 sums
    post, seen, stack = [], {s}, [(s, 0)]
    while stack:
        q, a = stack.pop()
        trs = cur[q]
        while a < len(trs) and not (_eps(trs[a]) and trs[a][3] not in seen):
            a += 1
        if a < len(trs):
            stack.append((q, a + 1))
            seen.add(trs[a][3])
            stack.append((trs[a][3], 0))
        else:
            post.append(q)
    d = {q: INF for q in post}
    d[s] = F32(0.0)
    for q in reversed(post):
        for il, ol, w, ns in cur[q]:
            if il == 0 and ol == 0:
                cand = F32(d[q] + w)
                if cand < d[ns]:
                    d[ns] = cand
    # the explicit-stack depth-first walk: pop, mark, push the unvisited epsilon targets in arc order
    walk, visited, out, index, k_max, fw = [s], set(), [], {}, 1, INF
    while walk:
        q = walk.pop()
        if q in visited:
            continue
        visited.add(q)
        for il, ol, w, ns in cur[q]:
            w = F32(d[q] + w)
            if il == 0 and ol == 0:
                if ns not in visited:
                    walk.append(ns)
                    k_max = max(k_max, len(walk))
            elif (il, ol, ns) in index:  # combined by min at the first occurrence
                j = index[(il, ol, ns)]
                if w < out[j][2]:
                    out[j] = (il, ol, w, ns)
            else:
                index[(il, ol, ns)] = len(out)
                out.append((il, ol, w, ns))
        fq = F32(d[q] + finals[q])
        fw = fq if fq < fw else fw
    out.reverse()
    return out, fw, (len(d), k_max, len(out))


def expected_stats(batches):
    """the counters of wfst_ctx_get_rm_epsilon_stats from the needs of every batch's states"""
    st = dict.fromkeys(STAT_KEYS, 0)
    st["batches"] = len(batches)
    for todo in batches:
        for kind, caps in rungs():
            if not todo:
                break
            st[kind + "_launches"] += 1
            st["max_closure_cap"] = max(st["max_closure_cap"], caps[0])
            rest = [need for need in todo if any(x > c for x, c in zip(need, caps))]
            st["states_" + kind] += len(todo) - len(rest)
            todo = rest
    return st


def rm_epsilon_model(flat):
    """rm_epsilon before its connect, for an input whose epsilon graph is acyclic:
    (flat FST, {rewritten state: (C, K, A)}, expected counters)"""
    n, start = flat["n_states"], flat["start"]
    if start is None or start < 0:
        return flat, {}, dict.fromkeys(STAT_KEYS, 0)
    off, arcs = flat["offsets"], flat["arcs"]
    cur = [[(int(a["ilabel"]), int(a["olabel"]), F32(a["weight"]), int(a["nextstate"])) for a in arcs[off[s]:off[s + 1]]]
           for s in range(n)]
    finals = [F32(x) for x in flat["finals"]]
    noneps_in = [False] * n
    noneps_in[start] = True
    for trs in cur:
        for t in trs:
            if not _eps(t):
                noneps_in[t[3]] = True
    # epsilon depth: the longest epsilon path to a state without epsilon arcs
    targets = [[t[3] for t in trs if _eps(t)] for trs in cur]
    depth, colour = [0] * n, [0] * n
    for root in range(n):
        if colour[root]:
            continue
        colour[root] = 1
        stack = [(root, iter(targets[root]))]
        while stack:
            s, it = stack[-1]
            for t in it:
                if colour[t] == 1:
                    raise ValueError("the epsilon graph has a cycle")
                if colour[t] == 0:
                    colour[t] = 1
                    stack.append((t, iter(targets[t])))
                    break
            else:
                stack.pop()
                colour[s] = 2
                depth[s] = max((depth[t] + 1 for t in targets[s]), default=0)
    needs, batches = {}, []
    for d in sorted(set(depth)):
        batch = [s for s in range(n) if noneps_in[s] and depth[s] == d]
        if not batch:
            continue
        done = [(s,) + _rewrite(cur, finals, s) for s in batch]  # (states of one depth do not read each other)
        for s, trs, fw, need in done:
            cur[s], finals[s], needs[s] = trs, fw, need
        batches.append([needs[s] for s in batch])
    for s in range(n):
        if not noneps_in[s]:
            cur[s] = []
    rows = [t for trs in cur for t in trs]
    out = dict(n_states=n, start=start, offsets=np.cumsum([0] + [len(trs) for trs in cur]).astype(np.uint32),
               arcs=np.array(rows, dtype=TR_DTYPE) if rows else np.zeros(0, TR_DTYPE),
               finals=np.array(finals, np.float32), props=0)
    return out, needs, expected_stats(batches)


class Builder:
    """states and arcs in creation order; weights in units of 1/512"""

    def __init__(self):
        self.trs, self.finals = [], []

    def state(self, final=None):
        self.trs.append([])
        self.finals.append(np.inf if final is None else final / 512.0)
        return len(self.trs) - 1

    def arc(self, s, il, ol, w, ns):
        self.trs[s].append((il, ol, w / 512.0, ns))

    def eps(self, s, w, ns):
        self.arc(s, 0, 0, w, ns)

    def flat(self, start=0, props=0, perm=None):
        trs, finals = self.trs, self.finals
        if perm is not None:  # state s becomes perm[s]
            inv = np.argsort(perm)
            trs = [[(il, ol, w, int(perm[ns])) for il, ol, w, ns in self.trs[inv[s]]] for s in range(len(trs))]
            finals = [self.finals[inv[s]] for s in range(len(trs))]
            start = int(perm[start])
        rows = [t for row in trs for t in row]
        return dict(n_states=len(trs), start=start, offsets=np.cumsum([0] + [len(r) for r in trs]).astype(np.uint32),
                    arcs=np.array(rows, dtype=TR_DTYPE) if rows else np.zeros(0, TR_DTYPE),
                    finals=np.array(finals, np.float32), props=props)


# Families: the start state 0 is rewritten over a sub-graph that ends in one final sink; each isolates one capacity.
def fan(m):
    """m epsilon arcs to m states with one labelled arc each: (m + 1, m, m)"""
    b = Builder()
    root = b.state()
    mids = [b.state() for _ in range(m)]
    sink = b.state(final=256)
    for i, q in enumerate(mids):
        b.eps(root, (i * 7) % 50, q)
        b.arc(q, i + 1, i + 1, (i * 13) % 97, sink)
    return b.flat()


def chain(length):
    """an epsilon chain of `length` arcs, then one labelled arc: (length + 1, 1, 1)"""
    b = Builder()
    states = [b.state() for _ in range(length + 1)]
    sink = b.state(final=256)
    for i in range(length):
        b.eps(states[i], 1 + i % 3, states[i + 1])
    b.arc(states[-1], 4, 5, 77, sink)
    return b.flat()


def par(p):
    """p parallel epsilon arcs with different weights to ONE state: (2, p, 1)"""
    b = Builder()
    root, q, sink = b.state(), b.state(), b.state(final=256)
    for i in range(p):
        b.eps(root, 5 + (i * 11) % p, q)  # (the smallest weight is not the first arc)
    b.arc(q, 4, 5, 77, sink)
    return b.flat()


def wide(a):
    """one epsilon arc to a state with `a` distinct labelled arcs: (2, 1, a)"""
    b = Builder()
    root, q, sink = b.state(), b.state(), b.state(final=256)
    b.eps(root, 9, q)
    for i in range(a):
        b.arc(q, i + 1, i + 1, (i * 13) % 97, sink)
    return b.flat()


def value_cases():
    """name -> (flat, epsilon graph acyclic)"""
    out = {}
    b = Builder()  # an epsilon arc of weight +inf beside a finite one
    root, u, v, sink = b.state(), b.state(), b.state(), b.state(final=256)
    b.arc(root, 0, 0, np.inf, u)
    b.eps(root, 512, v)
    b.eps(v, 3, u)  # (and u again over a finite path behind a second infinite arc)
    b.arc(root, 0, 0, np.inf, v)
    b.arc(u, 1, 1, 5, sink)
    b.arc(v, 2, 2, 6, sink)
    out["inf_epsilon"] = (b.flat(), True)
    b = Builder()  # only the infinite arc reaches u: the oracle keeps u's arc with weight +inf
    root, u, sink = b.state(), b.state(final=3), b.state(final=256)
    b.arc(root, 0, 0, np.inf, u)
    b.arc(u, 1, 1, 5, sink)
    b.arc(root, 2, 2, 5, sink)
    out["inf_epsilon_only"] = (b.flat(), True)
    b = Builder()  # negative epsilon weights, the longer path cheaper
    root, m1, m2, t, sink = b.state(), b.state(), b.state(), b.state(), b.state(final=256)
    b.eps(root, 100, t)
    b.eps(root, 50, m1)
    b.eps(m1, -300, m2)
    b.eps(m2, 40, t)
    b.eps(m1, 10, t)
    b.arc(t, 1, 1, 5, sink)
    b.arc(m2, 2, 2, -20, sink)
    out["negative_epsilon"] = (b.flat(), True)
    b = Builder()  # final states inside the closure and at the root
    root, u, v, sink = b.state(final=900), b.state(final=30), b.state(final=2), b.state(final=256)
    b.eps(root, 100, u)
    b.eps(u, 50, v)
    b.arc(v, 1, 1, 5, sink)
    out["final_in_closure"] = (b.flat(), True)
    b = Builder()
    root, u, sink = b.state(final=10), b.state(final=30), b.state(final=256)
    b.eps(root, 100, u)
    b.arc(u, 1, 1, 5, sink)
    out["final_at_root"] = (b.flat(), True)
    b = Builder()  # arcs with only one label 0 are not epsilon and stay
    root, u, v, sink = b.state(), b.state(), b.state(), b.state(final=256)
    b.arc(root, 0, 5, 1, u)
    b.arc(root, 5, 0, 2, v)
    b.eps(root, 3, u)
    b.arc(u, 0, 6, 4, sink)
    b.arc(v, 6, 0, 5, sink)
    b.eps(v, 1, u)
    out["half_epsilon"] = (b.flat(), True)
    b = Builder()  # a start state without arcs
    b.state()
    b.state(final=1)
    out["start_without_arcs"] = (b.flat(), True)
    b = Builder()
    b.state(final=5)
    out["single_state"] = (b.flat(), True)
    b = Builder()  # a zero-weight two-cycle with an epsilon self-loop
    hub, a, c, sink = b.state(), b.state(), b.state(final=9), b.state(final=256)
    b.arc(hub, 1, 1, 1, a)
    b.arc(hub, 2, 2, 2, c)
    b.eps(a, 0, a)
    b.eps(a, 0, c)
    b.eps(c, 0, a)
    b.arc(a, 3, 3, 7, sink)
    b.arc(c, 4, 4, 8, sink)
    out["zero_two_cycle"] = (b.flat(), False)
    b = Builder()  # a positive-weight epsilon self-loop alone
    hub, a, sink = b.state(), b.state(), b.state(final=256)
    b.arc(hub, 1, 1, 1, a)
    b.eps(a, 512, a)
    b.arc(a, 3, 3, 7, sink)
    out["self_loop"] = (b.flat(), False)
    return out


ACYCLIC_WORD = P.ACYCLIC | P.INITIAL_ACYCLIC


def props_random_inputs():
    """thirty seeded epsilon-acyclic inputs, half of them acceptors, each with three truthful words (acyclic = True
    numbers the states in topological order)"""
    rng = np.random.default_rng(20260)
    out = []
    for k in range(30):
        f = random_fst_flat(rng, int(rng.integers(3, 25)), 3, 3, p_eps_i=0.5, p_eps_o=0.5, p_final=0.3, acyclic=True)
        if not np.isfinite(f["finals"]).any():
            f["finals"][-1] = 1.0
        acceptor = k % 2 == 0
        if acceptor:
            f["arcs"]["olabel"] = f["arcs"]["ilabel"]
        base = ACYCLIC_WORD | (P.ACCEPTOR if acceptor else 0)
        for word in (0, base, base | P.TOP_SORTED):
            out.append(("random %d word %#x" % (k, word), dict(f, props=word)))
    return out


def props_hand_made():
    """cases in which exactly one fact about the added arcs decides the word.  The word is the caller's claim, which the
    reference trusts as the library does; the first two claims are contradicted by one arc on purpose, because no
    truthful ACCEPTOR or TOP_SORTED input can gain an arc that breaks them."""
    out = []
    for olabel in (2, 1):  # the only added arc has ilabel != olabel (and its twin, where ACCEPTOR survives)
        b = Builder()
        root, u, sink = b.state(), b.state(), b.state(final=256)
        b.eps(root, 3, u)
        b.arc(u, 1, olabel, 5, sink)
        out.append(("acceptor claim, added arc 1:%d" % olabel, b.flat(props=ACYCLIC_WORD | P.ACCEPTOR | P.TOP_SORTED)))
    for back in (True, False):  # the only added arc goes to a state <= its source (and its twin, where TOP_SORTED survives)
        b = Builder()
        s, u, sink = b.state(), b.state(final=5), b.state(final=256)
        b.eps(s, 3, u)
        b.arc(u, 1, 1, 5, s if back else sink)
        out.append(("top-sorted claim, added arc %s" % ("backwards" if back else "forwards"),
                    b.flat(props=ACYCLIC_WORD | P.ACCEPTOR | P.TOP_SORTED)))
    for gains in (False, True):  # no state gains an arc: ACYCLIC survives without TOP_SORTED (and its twin, where it goes)
        b = Builder()
        root, u = b.state(), b.state(final=5)
        b.eps(root, 3, u)
        if gains:
            sink = b.state(final=256)
            b.arc(u, 1, 1, 5, sink)
        out.append(("acyclic claim, %s" % ("an arc added" if gains else "nothing added"), b.flat(props=ACYCLIC_WORD)))
    return out
