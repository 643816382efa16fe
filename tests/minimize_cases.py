"""Input families and the invariant check of minimize that more than one test module, or a tool, uses."""
import json
import os

import numpy as np

from rustfst_amd._lib import TR_DTYPE

from oracle import model
from oracle.model import (ACCEPTOR, ACCESSIBLE, ACYCLIC, COACCESSIBLE, F32, INF, INITIAL_ACYCLIC, I_DETERMINISTIC,
                          KSHORTESTDELTA, O_DETERMINISTIC, UNWEIGHTED, WEIGHTED, make_flat, minimize_ref)
from helpers import ROOT, assert_flat_identical, to_device

GOLDEN = os.path.join(ROOT, "tests", "golden", "k16_minimize.json")


def trie_flat(rng, n_words, sigma, max_len, weighted=True, props=ACCEPTOR):
    """a trie of random words over `sigma` labels; arcs in insertion order (not label order).  Weights depend on the
    label alone (plus a rare odd one), so that many suffixes carry equal pushed weights and merge."""
    rows, finals = [[]], [INF]
    for _ in range(n_words):
        s = 0
        for _ in range(int(rng.integers(1, max_len + 1))):
            lab = int(rng.integers(1, sigma + 1))
            nxt = next((a[3] for a in rows[s] if a[0] == lab), None)
            if nxt is None:
                nxt = len(rows)
                rows.append([])
                finals.append(INF)
                w = float(lab % 3) if weighted else 0.0
                if weighted and rng.random() < 0.05:
                    w += float(rng.integers(1, 4))
                rows[s].append((lab, lab, w, nxt))
            s = nxt
        finals[s] = float(rng.integers(0, 2)) if weighted else 0.0
    return make_flat(len(rows), 0, rows, finals, props)


def random_dag(rng, n, sigma, weighted=True, props=ACCEPTOR, real=False):
    """a random deterministic acyclic acceptor (distinct labels per state, arcs forward), untrimmed"""
    rows, finals = [], []
    for s in range(n):
        labs = rng.permutation(np.arange(1, sigma + 1))[:int(rng.integers(0, sigma + 1))]
        row = []
        for lab in labs:
            if s + 1 >= n:
                break
            t = int(rng.integers(s + 1, min(n, s + 6)))
            w = (float(F32(rng.random() * 4)) if real else float(rng.integers(0, 3))) if weighted else 0.0
            row.append((int(lab), int(lab), w, t))
        rows.append(row)
        f = (float(F32(rng.random())) if real else float(rng.integers(0, 2))) if weighted else 0.0
        finals.append(f if rng.random() < 0.3 or s == n - 1 else INF)
    return make_flat(n, 0, rows, finals, props)


def random_cases(seed, count):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        kind = i % 4
        if kind == 0:
            out.append(("trie-w", trie_flat(rng, int(rng.integers(5, 60)), int(rng.integers(3, 6)), 6, True)))
        elif kind == 1:
            out.append(("trie-u", trie_flat(rng, int(rng.integers(5, 60)), int(rng.integers(3, 6)), 6, False)))
        elif kind == 2:
            out.append(("dag-w", random_dag(rng, int(rng.integers(2, 60)), 3, True)))
        else:
            out.append(("dag-u", random_dag(rng, int(rng.integers(2, 60)), 3, False, props=0)))
    return out


def golden_cases():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def cfg_of(c):
    return c.get("delta", KSHORTESTDELTA), bool(c.get("allow_nondet", False))


def accepts(flat, labels):
    """weight of the string in a deterministic acceptor, or None"""
    if flat["start"] is None:
        return None
    s, w = flat["start"], F32(0.0)
    off, arcs = flat["offsets"], flat["arcs"]
    for lab in labels:
        seg = arcs[off[s]:off[s + 1]]
        hit = np.nonzero(seg["ilabel"] == lab)[0]
        if not hit.size:
            return None
        w = F32(w + seg["weight"][hit[0]])
        s = int(seg["nextstate"][hit[0]])
    return None if not np.isfinite(flat["finals"][s]) else float(F32(w + flat["finals"][s]))


def label_sorted(flat):
    """the same FST with every state's arcs in label order"""
    arcs = flat["arcs"].copy()
    off = flat["offsets"]
    for s in range(flat["n_states"]):
        seg = arcs[off[s]:off[s + 1]]
        arcs[off[s]:off[s + 1]] = seg[np.argsort(seg["ilabel"], kind="stable")]
    return dict(flat, arcs=arcs)


def assert_idempotent(again, got, what):
    """minimize(minimize(x)) against minimize(x).  Exactly equal for the unweighted branch.  In the weighted branch the
    reference orders a state's arcs by the first occurrence of their (label, weight) tuples over the UNTRIMMED input of that
    call; the second call no longer sees the states the first one removed, so that order may differ (the restatement shows
    it, test_generator_shrinks_and_restatement_is_idempotent): there the two are equal once every state's arcs are put
    in label order — same states, same numbering, same weights.
    The property word is left out: the result of the weighted branch may have no weight left (then the second call takes
    the unweighted branch, whose word differs), and an empty result keeps what its input's content gave it; the word of
    the second call is checked against the restatement instead."""
    if got["n_states"] == 0:
        assert again["n_states"] == 0 and again["start"] is None, what
    elif np.array_equal(again["arcs"]["ilabel"], got["arcs"]["ilabel"]):
        assert_flat_identical(again, got, what, check_props=False)
    else:
        assert_flat_identical(label_sorted(again), label_sorted(got), what, check_props=False)


def weight_bound(length, wmax, delta):
    return (length + 1) * (delta / 2 + 8 * 2.0 ** -24 * max(1.0, 2 * wmax))


def no_start_cases():
    """weighted inputs without a start state: (flat, None) where pushing leaves no weight (the reference returns the empty
    FST), (flat, message) where a pushed weight stays (its acceptor_minimize bails)"""
    gone = make_flat(2, None, [[(1, 1, 1.0, 1)], []], [INF, 0.0], 0)  # d = [1, 0]: the arc becomes (1 + 0) - 1 = 0
    gone_known = dict(gone, props=ACCEPTOR | I_DETERMINISTIC | O_DETERMINISTIC | WEIGHTED | ACYCLIC | INITIAL_ACYCLIC)
    stays = make_flat(2, None, [[(1, 1, 1.0, 1), (2, 2, 3.0, 1)], []], [INF, 0.0], ACCEPTOR)  # d = [1, 0]: arcs 0 and 2
    return [(gone, None), (gone_known, None), (stays, "FST is not an unweighted acceptor")]


def far_apart_cases():
    """the unweighted branch compares no arc weight: states 1 and 2 merge although their arcs weigh -0.0009 / +0.0009
    (each within KDELTA of one, 0.0018 apart), or 0 / 0.5 under a stored UNWEIGHTED word"""
    rows = [[(1, 1, 0.0, 1), (2, 2, 0.0, 2)], [(3, 3, -0.0009, 3)], [(3, 3, 0.0009, 3)], []]
    a = make_flat(4, 0, rows, [INF, INF, INF, 0.0], 0)
    rows = [[(1, 1, 0.0, 1), (2, 2, 0.0, 2)], [(3, 3, 0.0, 3)], [(3, 3, 0.5, 3)], []]
    b = make_flat(4, 0, rows, [INF, INF, INF, 0.0], ACCEPTOR | I_DETERMINISTIC | UNWEIGHTED | ACYCLIC | INITIAL_ACYCLIC)
    return [a, b]


def finite_max(*arrays):
    m = 0.0
    for a in arrays:
        a = np.abs(np.asarray(a, dtype=np.float64))
        a = a[np.isfinite(a)]
        if a.size:
            m = max(m, float(a.max()))
    return m


def check_invariants(src_flat, got_dev, delta, ctx, rng, what, idempotent=True):
    """On a device result `got_dev` of minimizing `src_flat`: deterministic, acyclic, connected; the start's shortest
    distance and sampled strings keep their weight within the bound; minimizing again equals the restatement of that
    second call and (idempotent) changes nothing but, in the weighted branch, the arc order (assert_idempotent).
    The bound: weight_bound(L, W, delta) of the module docstring in the weighted branch, with W taken from the reverse
    distances, arc and final weights of the source and of the result.  The unweighted branch neither pushes nor quantizes:
    a merged state takes its survivor's arc weights, which tr_unique found within KDELTA of its own, and final weights are
    compared exactly, so a string with L arcs moves by at most L * KDELTA."""
    got = got_dev.to_flat()
    n = got["n_states"]
    if n == 0 or src_flat["start"] is None:
        return
    off, arcs = got["offsets"], got["arcs"]
    for s in range(min(n, 2000)):
        labs = arcs["ilabel"][off[s]:off[s + 1]]
        assert len(set(labs.tolist())) == len(labs), f"{what}: state {s} is not deterministic"
    acc, co, cyc, _ = model.graph_facts(got)
    assert acc and co and not cyc, what
    d_in = to_device(src_flat, ctx).shortest_distance(reverse=True)
    d_out = got_dev.shortest_distance(reverse=True)
    wmax = finite_max(d_in, d_out, src_flat["arcs"]["weight"], src_flat["finals"], got["arcs"]["weight"], got["finals"])
    unweighted = bool(got["props"] & UNWEIGHTED)

    def bound(length):
        return length * float(model.KDELTA) if unweighted else weight_bound(length, wmax, delta)
    # the longest string of the result: its height (longest path from the start), by peeling in topological order
    height = np.zeros(n, dtype=np.int64)
    indeg = np.bincount(arcs["nextstate"], minlength=n)
    fr = np.nonzero(indeg == 0)[0]
    src_of = np.repeat(np.arange(n), np.diff(off.astype(np.int64)))
    while fr.size:
        sel = np.isin(src_of, fr)
        t = arcs["nextstate"][sel].astype(np.int64)
        np.maximum.at(height, t, height[src_of[sel]] + 1)
        np.subtract.at(indeg, t, 1)
        t = np.unique(t)
        fr = t[indeg[t] == 0]
    longest = int(height.max())
    assert abs(float(d_in[src_flat["start"]]) - float(d_out[got["start"]])) <= bound(longest), what
    for _ in range(50):  # random walks in the result: the same string in the source
        s, labels = got["start"], []
        while True:
            deg = int(off[s + 1] - off[s])
            if deg == 0 or (np.isfinite(got["finals"][s]) and rng.random() < 0.3):
                break
            a = arcs[int(off[s]) + int(rng.integers(0, deg))]
            labels.append(int(a["ilabel"]))
            s = int(a["nextstate"])
        w_out, w_in = accepts(got, labels), accepts(src_flat, labels)
        assert (w_out is None) == (w_in is None), (what, labels)
        if w_out is not None:
            assert abs(w_out - w_in) <= bound(len(labels)), (what, labels, w_out, w_in)
    again = got_dev.minimize(None if delta == KSHORTESTDELTA else _cfg(delta)).to_flat()
    assert_flat_identical(again, minimize_ref(got, delta), f"{what} second call")
    if idempotent:
        assert_idempotent(again, got, f"{what} idempotent")


def _cfg(delta):
    import rustfst_amd
    return rustfst_amd.MinimizeConfig(delta)


def blow_up(rng, m, k):
    """k copies of every state of the minimal pushed DAG m (state-major: copy c of s is s * k + c), every arc to a random
    copy of its target, integer potentials V added (w + V(t) - V(s), finals f - V(s)); V = 0 on copy 0 of the start"""
    n = m["n_states"]
    V = rng.integers(-3, 4, size=n * k).astype(np.float32)
    V[m["start"] * k] = 0.0
    deg = np.diff(m["offsets"].astype(np.int64))
    src = np.repeat(np.arange(n), deg)
    big_src = (np.repeat(src, k).reshape(-1, k) * k + np.arange(k)).reshape(-1)  # arcs of copy c of s: grouped per state
    # state-major CSR: for state s, copy c: the arcs of s in order
    order = np.argsort(big_src, kind="stable")
    arc_of = np.repeat(np.arange(len(src)), k)[order]
    big_src = big_src[order]
    tgt = m["arcs"]["nextstate"][arc_of].astype(np.int64) * k + rng.integers(0, k, size=len(arc_of))
    arcs = np.zeros(len(arc_of), dtype=TR_DTYPE)
    arcs["ilabel"] = m["arcs"]["ilabel"][arc_of]
    arcs["olabel"] = m["arcs"]["olabel"][arc_of]
    arcs["weight"] = m["arcs"]["weight"][arc_of] + V[tgt] - V[big_src]
    arcs["nextstate"] = tgt
    off = np.zeros(n * k + 1, dtype=np.uint32)
    off[1:] = np.cumsum(np.repeat(deg, k))
    finals = np.repeat(m["finals"], k) - V
    return dict(n_states=n * k, start=int(m["start"]) * k, offsets=off, arcs=arcs, finals=finals.astype(np.float32),
                props=ACCEPTOR | ACYCLIC | INITIAL_ACYCLIC)


def closed_form_base(rng):
    """a minimal weighted DAG with integer weights that minimize_ref maps to itself, arc order included (the arc order of
    a result follows the untrimmed input of that call, so the restatement is applied until nothing moves)"""
    for _ in range(50):
        m = minimize_ref(random_dag(rng, 60, 3, True))
        if m["n_states"] < 20 or m["props"] != ACCESSIBLE | COACCESSIBLE:
            continue
        for _ in range(10):
            m["props"] = ACCEPTOR
            again = minimize_ref(m)
            if again["props"] != ACCESSIBLE | COACCESSIBLE:
                break
            same = np.array_equal(again["arcs"], m["arcs"]) and again["n_states"] == m["n_states"]
            m = again
            if same:
                m["props"] = ACCEPTOR
                return m
    raise AssertionError("no base graph found")
