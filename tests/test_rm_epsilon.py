"""wfst_rm_epsilon at every scratch limit, kernel hand-over and cycle order.

Without a GPU: the C-ABI and Python surface of wfst_ctx_get_rm_epsilon_stats, a plain Python restatement of the reference's
rewrite for inputs whose epsilon graph is acyclic (checked against the oracle), and the needs (closure states, stack
entries, arcs) of every input family below, so that a family that stops hitting its edge fails here.

On the device: every case bit-exact against the oracle, property word included, and for epsilon-acyclic cases the counters
of the call (which kernel ran, how often, how many states finished where) against what the restatement predicts from the
needs and the retry ladder.  Result parity alone cannot see a capacity comparison that is off by one: only the number of
retries changes.  Weights are on the 1/512 grid, where the exact minimum the kernels compute is the reference's distance."""
import ctypes as C
import functools
import inspect

import numpy as np
import pytest

from rustfst_amd._lib import TR_DTYPE
from rustfst_amd import synth as P

from oracle.model import F32, INF
import helpers
from helpers import assert_flat_identical, random_fst_flat, to_device, to_oracle


# The retry ladder of rm_epsilon_fst, restated once (rustfst_amd/csrc/rm_epsilon.hip, the attempt loop of rm_epsilon_fst:
# `RmCaps caps{16, 32, 32}`, `RmBigCaps big{1024, 1024, 1024}`, `const bool wave = caps.C > 64`, every size times 4 per
# retry).  A state finishes in the first rung whose (C, K, A) hold its closure, its largest stack occupancy and its arcs.
THREAD_RUNGS = ((16, 32, 32), (64, 128, 128))
WAVE_FIRST = (1024, 1024, 1024)
GROWTH = 4
WAVE_COMPONENT = 64  # members of an epsilon component larger than this go straight to the wave kernel (`closure_hint > 64`)
STAT_KEYS = ("batches", "thread_launches", "wave_launches", "states_thread", "states_wave", "max_closure_cap")


def rungs():
    for caps in THREAD_RUNGS:
        yield "thread", caps
    caps = WAVE_FIRST
    while True:
        yield "wave", caps
        caps = tuple(c * GROWTH for c in caps)


# ---------------------------------------------------------------- restatement (rm_epsilon_static.rs:50-163)
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


# ---------------------------------------------------------------- inputs
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


def ladder(length):
    """a chain 1 -> 2 -> ... -> length of cheap epsilon arcs, every chain state with one labelled arc, and one expensive
    epsilon arc from the root to every chain state but the first, which it reaches by a cheap one: (length + 1, length,
    length).  The root's arcs list the chain backwards, so the closure is discovered farthest state first and every
    distance improves one hop per label-correcting round whichever way a round sweeps the closure."""
    b = Builder()
    root = b.state()
    states = [b.state() for _ in range(length)]
    sink = b.state(final=256)
    for i in range(length - 1, 0, -1):
        b.eps(root, 2048, states[i])
    b.eps(root, 1, states[0])
    for i, q in enumerate(states):
        if i + 1 < length:
            b.eps(q, 1, states[i + 1])
        b.arc(q, i + 1, i + 1, (i * 13) % 97, sink)
    return b.flat()


FAMILIES = {"fan": fan, "chain": chain, "par": par, "wide": wide, "ladder": ladder}
FAMILY_CASES = ([("chain", c - 1, (c, 1, 1)) for c in (16, 17, 64, 65, 1024, 1025)]
                + [("par", p, (2, p, 1)) for p in (32, 33, 128, 129, 1024, 1025)]
                + [("wide", a, (2, 1, a)) for a in (32, 33, 128, 129, 1024, 1025)]
                + [("fan", m, (m + 1, m, m)) for m in (15, 16, 63, 64, 1023, 1024)]
                + [("ladder", n, (n + 1, n, n)) for n in (14, 60, 200, 1100)])
FAMILY_IDS = ["%s-%d" % (name, size) for name, size, _ in FAMILY_CASES]


@functools.lru_cache(maxsize=None)
def family(name, size):
    flat = FAMILIES[name](size)
    return flat, rm_epsilon_model(flat)


DUP_POSITIONS = (3, 67, 129)
CHUNK_CASES = [(a, m, a == 130) for a in (130, 192, 193) for m in DUP_POSITIONS]  # (130 - 3 arcs fit the thread kernel)


def chunk_case(a, min_at, force_wave):
    """wide(a) whose arcs 3, 67 and 129 share one (ilabel, olabel, nextstate), the smallest weight at `min_at`; arcs 10
    and 20 share a second key inside one chunk of 64; a second closure state, walked first, holds the keys of arcs 5
    (cheaper there) and 100 (cheaper here).  force_wave: 129 parallel epsilon arcs send the rewrite to the wave kernel."""
    b = Builder()
    root, w, v, sink = b.state(), b.state(), b.state(), b.state(final=256)
    for i in range(129 if force_wave else 1):
        b.eps(root, 5 + i, w)
    b.eps(root, 3, v)  # (pushed last: popped and walked first)
    for i in range(a):
        if i in DUP_POSITIONS:
            b.arc(w, 7777, 7777, 10 if i == min_at else 50 + i, sink)
        elif i in (10, 20):
            b.arc(w, 8888, 8889, 60 - i, sink)
        else:
            b.arc(w, i + 1, i + 1, 100 + (i * 37) % 64, sink)
    b.arc(v, 6, 6, 20, sink)
    b.arc(v, 101, 101, 900, sink)
    return b.flat()


def push_case():
    """under the root one state with 100 arcs, 70 of them epsilon arcs to distinct unvisited targets (the 64th arc lies
    between them); some targets also reach the next one, which is then walked before its own stack entry comes up"""
    b = Builder()
    root, x = b.state(), b.state()
    b.eps(root, 2, x)
    targets = [b.state(final=(40 + j if j % 9 == 0 else None)) for j in range(70)]
    sink = b.state(final=256)
    j = 0
    for i in range(100):
        if i % 10 < 7:
            b.eps(x, (i * 5) % 31, targets[j])
            j += 1
        else:
            b.arc(x, 500 + i, 500 + i, i, sink)
    for j, t in enumerate(targets):
        b.arc(t, 200 + j % 60, 200 + j % 60, (j * 13) % 97, sink)  # (the last ten repeat keys of the first ten)
        if j % 5 == 0 and j + 1 < len(targets):
            b.eps(t, 1, targets[j + 1])
    return b.flat()


def arena_case():
    """states that read rewritten successors out of the arenas of earlier attempts:
    q  (depth 0) 210 arcs, 200 distinct: finishes in the wave kernel
    r  (depth 1) an epsilon arc to q: 201 arcs, the wave kernel reads q from its arena; r1 beside it has a closure of two
       and finishes in the first thread launch of the same batch
    q2 (depth 1) 129 parallel epsilon arcs to a state with 20 arcs: the wave kernel, 20 arcs
    r2 (depth 2) an epsilon arc to q2: the thread kernel reads q2 from the arena of a wave attempt
    r3 (depth 2) epsilon arcs to r and q2: the wave kernel reads both, and q2's keys are twenty of those r took from q"""
    b = Builder()
    hub, q, r, r1, z, q2, z2, r2, r3 = (b.state() for _ in range(9))
    sink = b.state(final=256)
    for i, s in enumerate((q, r, r1, q2, r2, r3)):
        b.arc(hub, 900 + i, 900 + i, 3 * i, s)
    for i in range(210):
        k = i - 200 if i >= 200 else i  # the last ten repeat the first ten keys
        b.arc(q, k + 1, k + 1, (i * 29) % 113, sink)
    b.eps(r, 4, q)
    b.arc(r, 300, 300, 1, sink)
    b.eps(r1, 6, z)
    for i in range(3):
        b.arc(z, 10 + i, 20 + i, i, sink)
    for i in range(129):
        b.eps(q2, 1 + (i * 7) % 129, z2)
    for i in range(20):
        b.arc(z2, 40 + i, 40 + i, (i * 5) % 17, sink)
    b.eps(r2, 8, q2)
    b.arc(r2, 301, 301, 2, sink)
    b.eps(r3, 2, r)
    b.eps(r3, 1, q2)
    return b.flat()


MIXED_ARCS = (5, 100, 500, 1025, 0)  # first / second thread size, first / second wave size, no arcs


def mixed_case():
    """one depth-0 batch of fifteen states in interleaved id order, three each of MIXED_ARCS (plus the hub and the sink),
    and above every one a depth-1 state that reads it"""
    b = Builder()
    hub = b.state()
    sink = b.state(final=256)
    for i in range(15):
        n_arcs = MIXED_ARCS[i % 5]
        item = b.state(final=None if n_arcs else 7 + i)
        upper = b.state()
        b.arc(hub, 2000 + i, 2000 + i, i, item)
        b.arc(hub, 3000 + i, 3000 + i, i, upper)
        for k in range(n_arcs):
            b.arc(item, k + 1, k + 1, (k * 13 + i) % 97, sink)
        b.eps(upper, 1 + i, item)
        b.arc(upper, 4000, 4000, 3, sink)
    return b.flat()


def ring(k, seed=None, hub_every=1, two=False):
    """a ring of k epsilon arcs, a labelled arc out of every member to the sink, a start hub with labelled arcs into every
    hub_every-th member (through one more hub per 100 members, so that no hub outgrows the thread kernel).  seed: ids
    permuted.  two: a second ring one epsilon depth up, joined by an epsilon arc.
    Returns (flat, number of rewritten ring members, number of rewritten states outside the rings)."""
    b = Builder()
    hub = b.state()
    rings = [[b.state() for _ in range(k)] for _ in range(2 if two else 1)]
    rewritten, hubs = 0, []
    for ri, members in enumerate(rings):
        for i, s in enumerate(members):
            b.eps(s, 1 + (i * 3 + ri) % 5, members[(i + 1) % k])
            if i % hub_every == 0:
                if rewritten % 100 == 0:
                    hubs.append(b.state())
                    b.arc(hub, 5000 + len(hubs), 5000 + len(hubs), len(hubs), hubs[-1])
                b.arc(hubs[-1], 1000 * (ri + 1) + i, 7, i % 11, s)
                rewritten += 1
    sink = b.state(final=256)
    for ri, members in enumerate(rings):
        for i, s in enumerate(members):
            b.arc(s, 1 + i, 1 + i + ri, (i * 13) % 97, sink)
    if two:
        b.eps(rings[1][0], 2, rings[0][3 % k])
    perm = None
    if seed is not None:
        perm = np.arange(len(b.trs))
        ids = perm[1:-1].copy()
        np.random.default_rng(seed).shuffle(ids)
        perm[1:-1] = ids
    return b.flat(perm=perm), rewritten, len(hubs) + 2


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


# ================================================================ no GPU
def test_stats_symbol_declared_exported_and_bound(wfst_lib):
    import rustfst_amd
    helpers.check_counter_getter(wfst_lib, "wfst_ctx_get_rm_epsilon_stats", STAT_KEYS, rustfst_amd.rm_epsilon_stats)


def test_stats_null_context_is_ko(wfst_lib):
    assert "null" in helpers.ko_message(wfst_lib.wfst_ctx_get_rm_epsilon_stats(None, None, None, None, None, None, None))
    vals = [C.c_uint64(7) for _ in STAT_KEYS]
    assert "null" in helpers.ko_message(wfst_lib.wfst_ctx_get_rm_epsilon_stats(None, *[C.byref(v) for v in vals]))
    assert [v.value for v in vals] == [7] * len(STAT_KEYS)


def test_python_surface():
    import rustfst_amd
    assert "rm_epsilon_stats" in rustfst_amd.__all__ and hasattr(rustfst_amd, "rm_epsilon_stats")
    p = inspect.signature(rustfst_amd.rm_epsilon_stats).parameters
    assert list(p) == ["ctx"] and p["ctx"].default is None


def assert_model_is_oracle(oracle, flat, what):
    model, needs, stats = rm_epsilon_model(flat)
    got = to_oracle(oracle, model)
    got.connect()
    ref = to_oracle(oracle, flat)
    ref.rm_epsilon()
    assert_flat_identical(got.to_flat(), ref.to_flat(), what, check_props=False)
    return needs, stats


def test_model_against_oracle(oracle):
    rng = np.random.default_rng(1234)
    with_arcs = 0
    for k in range(200):
        f = random_fst_flat(rng, int(rng.integers(1, 40)), 3, 3, p_eps_i=0.5, p_eps_o=0.5, p_final=0.3, acyclic=True,
                            sort=("none", "ilabel")[k % 2])
        if not np.isfinite(f["finals"]).any():
            f["finals"][-1] = 1.0
        needs, _ = assert_model_is_oracle(oracle, f, "random %d" % k)
        with_arcs += any(c > 1 for c, _, _ in needs.values())
    assert with_arcs > 100  # (the inputs do have closures to walk)


@pytest.mark.parametrize("name,size,need", FAMILY_CASES, ids=FAMILY_IDS)
def test_family_needs(oracle, name, size, need):
    """the start state of every family needs exactly what the family is there for, and the model is the oracle on it"""
    flat, (_, needs, stats) = family(name, size)
    assert needs[0] == need
    assert {s: v for s, v in needs.items() if s} == {flat["n_states"] - 1: (1, 1, 0)}  # (only the sink beside it)
    assert stats["batches"] == 2
    assert_model_is_oracle(oracle, flat, "%s(%d)" % (name, size))


def test_expected_stats_of_the_ladder():
    """the prediction itself at the rungs: fits at a capacity, retries one above it"""
    def one(need):
        return expected_stats([[need]])
    assert one((16, 32, 32)) == dict(batches=1, thread_launches=1, wave_launches=0, states_thread=1, states_wave=0,
                                     max_closure_cap=16)
    for need in ((17, 1, 1), (2, 33, 1), (2, 1, 33), (64, 128, 128)):
        assert one(need) == dict(batches=1, thread_launches=2, wave_launches=0, states_thread=1, states_wave=0,
                                 max_closure_cap=64), need
    for need in ((65, 1, 1), (2, 129, 1), (2, 1, 129), (1024, 1024, 1024)):
        assert one(need) == dict(batches=1, thread_launches=2, wave_launches=1, states_thread=0, states_wave=1,
                                 max_closure_cap=1024), need
    for need in ((1025, 1, 1), (2, 1025, 1), (2, 1, 1025)):
        assert one(need) == dict(batches=1, thread_launches=2, wave_launches=2, states_thread=0, states_wave=1,
                                 max_closure_cap=4096), need
    assert expected_stats([[(1, 1, 0), (2, 1, 1025)], [(17, 1, 1)]]) == dict(
        batches=2, thread_launches=4, wave_launches=2, states_thread=2, states_wave=1, max_closure_cap=4096)


def test_hand_made_inputs_are_what_they_claim(oracle):
    """the model is the oracle on every epsilon-acyclic hand-made input, and the inputs reach the kernels they are for"""
    for a, min_at, force in CHUNK_CASES:
        needs, stats = assert_model_is_oracle(oracle, chunk_case(a, min_at, force), "chunk")
        assert needs[0] == (3, 130 if force else 2, a - 3) and stats["states_wave"] == 1
    needs, stats = assert_model_is_oracle(oracle, push_case(), "push")
    assert needs[0][0] == 72 and stats["states_wave"] == 1
    needs, stats = assert_model_is_oracle(oracle, arena_case(), "arena")
    assert [needs[s] for s in (1, 2, 3, 5, 7, 8)] == [(1, 1, 200), (2, 1, 201), (2, 1, 3), (2, 129, 20), (2, 1, 21),
                                                      (3, 2, 201)]  # (q2's twenty keys are twenty of q's)
    assert stats["batches"] == 3 and stats["states_wave"] == 4
    needs, stats = assert_model_is_oracle(oracle, mixed_case(), "mixed")
    assert stats == dict(batches=2, thread_launches=4, wave_launches=4, states_thread=2 + 9 + 9, states_wave=6 + 6,
                         max_closure_cap=4096)
    for name, (flat, acyclic) in value_cases().items():
        if acyclic:
            assert_model_is_oracle(oracle, flat, name)
    for name, flat in props_random_inputs()[::3] + props_hand_made():
        assert_model_is_oracle(oracle, flat, name)


def test_property_inputs_give_distinct_words(oracle):
    words = set()
    for name, flat in props_random_inputs() + props_hand_made():
        words.add(to_oracle(oracle, flat).rm_epsilon().properties)
    assert len(words) >= 3, [hex(w) for w in words]
    # every hand-made pair differs in exactly the bit it is made for
    hand = [to_oracle(oracle, flat).rm_epsilon().properties for _, flat in props_hand_made()]
    assert not hand[0] & P.ACCEPTOR and hand[1] & P.ACCEPTOR
    assert not hand[2] & P.TOP_SORTED and hand[3] & P.TOP_SORTED
    assert hand[4] & P.ACYCLIC and not hand[4] & P.TOP_SORTED and not hand[5] & P.ACYCLIC


# ================================================================ device
def run(gpu_ctx, oracle, flat, what, model=True, expected=None):
    """rm_epsilon on the device against the oracle, bit for bit; the counters against the model.  Returns the counters."""
    import rustfst_amd
    ref = to_oracle(oracle, flat)
    ref.rm_epsilon()
    got = to_device(flat, gpu_ctx).rm_epsilon().to_flat()
    stats = rustfst_amd.rm_epsilon_stats(gpu_ctx)
    if model and expected is None:
        expected = rm_epsilon_model(flat)[2]
    print("%s: counters %s, model %s" % (what, stats, expected))
    assert_flat_identical(got, ref.to_flat(), what)
    if model:
        assert stats == expected, what
    return stats


@pytest.mark.gpu
@pytest.mark.parametrize("name,size,need", FAMILY_CASES, ids=FAMILY_IDS)
def test_family_on_device(gpu_ctx, oracle, name, size, need):
    flat, (_, _, expected) = family(name, size)
    run(gpu_ctx, oracle, flat, "%s(%d)" % (name, size), expected=expected)


@pytest.mark.gpu
@pytest.mark.parametrize("a,min_at,force_wave", CHUNK_CASES)
def test_wave_chunks_combine_duplicates(gpu_ctx, oracle, a, min_at, force_wave):
    stats = run(gpu_ctx, oracle, chunk_case(a, min_at, force_wave), "chunk(%d, min at %d)" % (a, min_at))
    assert stats["states_wave"] == 1
    if a == 130:  # the same arcs through the thread kernel
        stats = run(gpu_ctx, oracle, chunk_case(a, min_at, False), "chunk(%d, min at %d), thread" % (a, min_at))
        assert stats["states_wave"] == 0


@pytest.mark.gpu
def test_wave_push_order_across_a_chunk(gpu_ctx, oracle):
    assert run(gpu_ctx, oracle, push_case(), "push")["states_wave"] == 1


@pytest.mark.gpu
def test_rewritten_successors_are_read_from_the_arenas(gpu_ctx, oracle):
    stats = run(gpu_ctx, oracle, arena_case(), "arena")
    assert stats["states_wave"] == 4 and stats["batches"] == 3


@pytest.mark.gpu
def test_one_mixed_batch(gpu_ctx, oracle):
    stats = run(gpu_ctx, oracle, mixed_case(), "mixed")
    assert stats["thread_launches"] == 4 and stats["wave_launches"] == 4


@pytest.mark.gpu
@pytest.mark.parametrize("k", (2, 16, 64, 65, 300))
def test_epsilon_ring(gpu_ctx, oracle, k):
    flat, members, others = ring(k)
    stats = run(gpu_ctx, oracle, flat, "ring(%d)" % k, model=False)
    assert members == k and stats["batches"] == k + 1  # hubs and sink together, then one batch per member
    assert stats["states_wave"] == (0 if k <= WAVE_COMPONENT else members)
    assert stats["states_thread"] + stats["states_wave"] == members + others


@pytest.mark.gpu
@pytest.mark.parametrize("k", (64, 65))
@pytest.mark.parametrize("variant", ("permuted", "every_third", "two_rings"))
def test_epsilon_ring_variants(gpu_ctx, oracle, k, variant):
    flat, members, others = ring(k, seed=77 + k if variant == "permuted" else None, hub_every=3 if variant == "every_third" else 1,
                         two=variant == "two_rings")
    stats = run(gpu_ctx, oracle, flat, "ring(%d) %s" % (k, variant), model=False)
    assert stats["batches"] == members + 1
    if variant != "two_rings":
        assert stats["states_wave"] == (0 if k <= WAVE_COMPONENT else members)
    else:  # the upper ring's closures run into the lower ring: 65 states and more, whatever the component's size
        assert stats["states_wave"] >= 1
    assert stats["states_thread"] + stats["states_wave"] == members + others


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(value_cases()))
def test_values(gpu_ctx, oracle, name):
    flat, acyclic = value_cases()[name]
    run(gpu_ctx, oracle, flat, name, model=acyclic)


@pytest.mark.gpu
def test_no_start_leaves_the_counters_zero(gpu_ctx, oracle):
    flat = fan(15)
    assert run(gpu_ctx, oracle, flat, "fan(15)")["batches"] == 2  # (counters that the next call has to clear)
    stats = run(gpu_ctx, oracle, dict(flat, start=-1), "no start", model=False)
    assert stats == dict.fromkeys(STAT_KEYS, 0)


@pytest.mark.gpu
def test_property_word(gpu_ctx, oracle):
    words = set()
    for name, flat in props_random_inputs() + props_hand_made():
        run(gpu_ctx, oracle, flat, name)
        words.add(to_oracle(oracle, flat).rm_epsilon().properties)
    assert len(words) >= 3
