"""minimize / minimize_with_config of input-deterministic acyclic acceptors (wfst_minimize): the C-ABI surface without a
GPU, a literal sequential Python restatement of rustfst's minimize_with_config (AcyclicMinimizer branch; written out
below) checked against the hand-derived K16 known answers, the survivor rule checked against it, and on the device
parity with the restatement in every regime, closed-form answers at scale, invariants and error handling.

Bound on weights (used by the invariants): push_weights(ToInitial) replaces w by (w + d[t]) - d[s]; along a path these
telescope, so in exact arithmetic the weight of every string is unchanged.  Each of the two f32 operations rounds by at
most 2^-24 relative to a magnitude of at most 2 W (W = the largest |distance| or |weight| met), QuantizeMapper moves a
value by at most delta / 2 and its own division, floor and product round by at most 3 * 2^-24 relative.  A string with
L arcs and one final weight therefore moves by at most
    weight_bound(L, W, delta) = (L + 1) * (delta / 2 + 8 * 2^-24 * max(1, 2 W))."""
import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest

from rustfst_amd._lib import TR_DTYPE

from oracle import model
from oracle.model import (ACCEPTOR, ACCESSIBLE, ACYCLIC, ADD_SUPER_FINAL, ALL, ARCSORT, ARC_RELEVANT, COACCESSIBLE,
                          CYCLIC, EPSILONS, F32, INF, INITIAL_ACYCLIC, I_DETERMINISTIC, I_EPSILONS, I_LABEL_INVARIANT,
                          I_LABEL_SORTED, KSHORTESTDELTA, NOT_ACCEPTOR, NOT_I_DETERMINISTIC, NOT_I_LABEL_SORTED,
                          NOT_O_LABEL_SORTED, NOT_TOP_SORTED, NO_EPSILONS, NO_I_EPSILONS, NO_O_EPSILONS,
                          O_DETERMINISTIC, O_EPSILONS, O_LABEL_INVARIANT, O_LABEL_SORTED, RM_SUPER_FINAL, TOP_SORTED,
                          UNWEIGHTED, Unsupported, WEIGHTED, WEIGHT_INVARIANT, compute_and_update, connect, flat_to_fst,
                          fst_to_flat, is_cyclic, known, make_flat, p_add_tr, quantize, rm_final_epsilon, tr_map,
                          tr_unique, wkey)
from helpers import ROOT, assert_flat_identical, ko_message, to_device
import test_push_weights as pw

GOLDEN = os.path.join(ROOT, "tests", "golden", "k16_minimize.json")
PATHS = ("narrow", "wide", "auto")
MSG_NONDET = "Refusing to minimize a non-deterministic FST with allow_nondet = false"


# ---------------------------------------------------------------- the restatement
class Partition:  # partition.rs:6-92
    def __init__(self, n):
        self.cls = [None] * n
        self.nxt = [-1] * n
        self.prv = [-1] * n
        self.head = []

    def add_class(self):
        self.head.append(-1)
        return len(self.head) - 1

    def add(self, e, c):
        h = self.head[c]
        if h >= 0:
            self.prv[h] = e
        self.head[c] = e
        self.cls[e] = c
        self.nxt[e] = h
        self.prv[e] = -1

    def move_element(self, e, c):
        p, nx, old = self.prv[e], self.nxt[e], self.cls[e]
        if p >= 0:
            self.nxt[p] = nx
        else:
            self.head[old] = nx
        if nx >= 0:
            self.prv[nx] = p
        self.add(e, c)

    def members(self, c):
        e = self.head[c]
        while e >= 0:
            yield e
            e = self.nxt[e]


def fst_depth(fst):  # minimize.rs:269-304 (an explicit stack in place of the recursion; same post-order)
    rows = fst["rows"]
    heights = []
    visited = set()
    stack = [(fst["start"], 0)]
    visited.add(fst["start"])
    while stack:
        s, i = stack[-1]
        while len(heights) <= s:
            heights.append(-1)
        if i < len(rows[s]):
            stack[-1] = (s, i + 1)
            t = rows[s][i][3]
            if t not in visited:
                visited.add(t)
                stack.append((t, 0))
        else:
            stack.pop()
            heights[s] = max([0] + [1 + heights[tr[3]] for tr in rows[s]])
    return heights


def acyclic_partition(fst):
    """AcyclicMinimizer::new (minimize.rs:306-387): classes by height, refined height by height; two states compare Equal
    when StateComparator finds neither below the other (:389-456): final weight (exact), arc count, positionally
    (ilabel, class of nextstate)."""
    heights = fst_depth(fst)
    part = Partition(len(heights))
    for _ in range(max(heights) + 1):
        part.add_class()
    for s, h in enumerate(heights):
        part.add(s, h)
    n_height = len(part.head)
    for h in range(n_height):
        def key(s):
            f = fst["finals"][s]
            return (float(INF if f is None else f), len(fst["rows"][s]), tuple((tr[0], part.cls[tr[3]]) for tr in fst["rows"][s]))
        members = list(part.members(h))
        equiv = {key(members[0]): h}
        for e in members[1:]:
            k = key(e)
            if k not in equiv:
                equiv[k] = part.add_class()
        target = {s: equiv[key(s)] for s in members}  # (the keys read the partition before any move of this height)
        for s in members:
            if part.cls[s] != target[s]:
                part.move_element(s, target[s])
    return part


def merge_states(part, fst):  # minimize.rs:213-266
    rows = fst["rows"]
    state_map = [next(part.members(c)) for c in range(len(part.head))]
    p = fst["props"]
    for c in range(len(part.head)):
        for s in part.members(c):
            if s == state_map[c]:
                for tr in rows[s]:
                    p &= ARC_RELEVANT  # set_nextstate_unchecked (trs_iter_mut.rs:222-225, 293-305)
                    tr[3] = state_map[part.cls[tr[3]]]
            else:
                for tr in [list(t) for t in rows[s]]:
                    tr[3] = state_map[part.cls[tr[3]]]
                    dst = rows[state_map[c]]
                    dst.append(tr)
                    p = p_add_tr(p, state_map[c], tr, dst[-2] if len(dst) > 1 else None)
    fst["start"] = state_map[part.cls[fst["start"]]]
    fst["props"] = model.p_set_start(p)
    connect(fst)


def acceptor_minimize(fst, seen=None):  # minimize.rs:181-211
    """seen (a dict): receives T, a copy of the connected, label-sorted machine the partition is computed on (what
    minimize.hip's run_core refines), and part, its Partition"""
    props = compute_and_update(fst, ACCEPTOR | UNWEIGHTED | ACYCLIC)
    if props & (ACCEPTOR | UNWEIGHTED) != ACCEPTOR | UNWEIGHTED:
        raise Unsupported("FST is not an unweighted acceptor")
    if not props & ACYCLIC:
        raise Unsupported("cyclic inputs are not supported")  # (this project: a cycle anywhere, before connect)
    connect(fst)
    if not fst["rows"]:
        return
    for row in fst["rows"]:  # tr_sort(ILabelCompare): stable
        row.sort(key=lambda t: t[0])
    p = (fst["props"] & ARCSORT) | I_LABEL_SORTED
    if fst["props"] & ACCEPTOR:
        p |= O_LABEL_SORTED
    fst["props"] = p
    part = acyclic_partition(fst)
    if seen is not None:
        seen["T"] = dict(rows=[[list(tr) for tr in row] for row in fst["rows"]], finals=list(fst["finals"]),
                         start=fst["start"], props=fst["props"])
        seen["part"] = part
    merge_states(part, fst)
    tr_unique(fst)


def rdist_dag(flat):
    """reverse shortest distances of an acyclic FST in f32: d[s] = min(final[s], min over arcs (w + d[next])), the value the
    relaxation converges to (f32 addition is monotone); +inf for a state that reaches no final state"""
    n = flat["n_states"]
    off, arcs, fin = flat["offsets"], flat["arcs"], flat["finals"]
    d = [None] * n
    for root in range(n):
        if d[root] is not None:
            continue
        stack = [(root, 0)]
        while stack:
            s, i = stack[-1]
            b, e = int(off[s]), int(off[s + 1])
            if b + i < e:
                stack[-1] = (s, i + 1)
                t = int(arcs["nextstate"][b + i])
                if d[t] is None and all(t != q for q, _ in stack):
                    stack.append((t, 0))
            else:
                stack.pop()
                best = F32(fin[s])
                for a in arcs[b:e]:
                    v = model.times(F32(a["weight"]), d[int(a["nextstate"])])
                    best = v if v < best else best
                d[s] = best
    return d


def minimize_ref(flat, delta=KSHORTESTDELTA, allow_nondet=False, partition_out=None):
    """minimize_with_config (minimize.rs:92-176), statement by statement, for the branch this project supports; raises
    Unsupported with the KO message otherwise.  Returns flat arrays.  partition_out (a dict): see acceptor_minimize (in the
    weighted branch T is the encoded machine with its superfinal state)."""
    fst = flat_to_fst(flat)
    props = compute_and_update(fst, ACCEPTOR | I_DETERMINISTIC | WEIGHTED | UNWEIGHTED)
    if not props & I_DETERMINISTIC and not allow_nondet:
        raise Unsupported(MSG_NONDET)
    if not props & ACCEPTOR:
        raise Unsupported("transducers are not supported")
    if not props & I_DETERMINISTIC:
        raise Unsupported("non-deterministic inputs are not supported")
    if not known(fst["props"]) & ACYCLIC:
        if is_cyclic(flat):
            raise Unsupported("cyclic inputs are not supported")
    elif fst["props"] & CYCLIC:
        raise Unsupported("cyclic inputs are not supported")
    if props & WEIGHTED:
        # (without a start state push still reweights, every tr_map below returns at once, and acceptor_minimize decides
        # from the pushed content: the empty FST, or "FST is not an unweighted acceptor")
        # push_weights_with_config(ToInitial, default.with_delta(delta)) (push.rs:89-118)
        cur = fst_to_flat(fst)
        dist = rdist_dag(cur)[:pw.reverse_len_rule(cur)]
        fst = pw.push_ref(cur, dist, False, False)
        fst["props"] &= ALL
        # tr_map(QuantizeMapper(delta)) (quantize_mapper.rs)
        def q_arc(tr):
            tr[2] = quantize(tr[2], delta)

        def q_fin(ftr):
            ftr[2] = quantize(ftr[2], delta)
        tr_map(fst, q_arc, q_fin, False, lambda p: p & WEIGHT_INVARIANT)
        # encode(EncodeWeightsAndLabels) (encode_static.rs): one table for arc and final tuples, in scan order
        table, tuples = {}, []

        def enc(il, ol, w):
            k = (il, ol, wkey(w))
            if k not in table:
                table[k] = len(tuples) + 1
                tuples.append((il, ol, F32(w)))
            return table[k]

        def e_arc(tr):
            lab = enc(tr[0], tr[1], tr[2])
            tr[0], tr[1], tr[2] = lab, lab, F32(0.0)

        def e_fin(ftr):
            lab = enc(ftr[0], ftr[1], ftr[2])
            ftr[0], ftr[1], ftr[2] = lab, lab, F32(0.0)
        enc_mask = I_LABEL_INVARIANT & O_LABEL_INVARIANT & WEIGHT_INVARIANT & ADD_SUPER_FINAL
        tr_map(fst, e_arc, e_fin, True, lambda p: p & enc_mask)
        acceptor_minimize(fst, partition_out)
        # decode (decode_static.rs): labels and weights back, then rm_final_epsilon
        def d_arc(tr):
            il, ol, w = tuples[tr[0] - 1]
            tr[0], tr[1], tr[2] = il, ol, w
        dec_mask = I_LABEL_INVARIANT & O_LABEL_INVARIANT & WEIGHT_INVARIANT & RM_SUPER_FINAL
        tr_map(fst, d_arc, lambda ftr: None, False, lambda p: p & dec_mask)
        rm_final_epsilon(fst)
    else:
        acceptor_minimize(fst, partition_out)
    return fst_to_flat(fst)


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


def golden_flat(c, key="input"):
    g = c[key]
    n = g["n_states"]
    rows = [[] for _ in range(n)]
    for s, il, ol, w, ns in g["arcs"]:
        rows[s].append((il, ol, w, ns))
    finals = [INF] * n
    for s, w in g["finals"]:
        finals[s] = w
    return make_flat(n, g["start"], rows, finals, int(g["props"], 16))


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


# ================================================================ CPU
def test_symbol_declared_and_bound(wfst_lib):
    from rustfst_amd import _lib
    with open(os.path.join(ROOT, "include", "wfst.h")) as f:
        header = f.read()
    assert re.search(r"\bwfst_status\s+wfst_minimize\s*\(", header)
    assert "wfst_minimize" in {name for name, _, _ in _lib.SYMBOLS}
    assert hasattr(wfst_lib, "wfst_minimize")
    assert re.search(r"#define\s+WFST_ABI_VERSION\s+7\b", header)
    assert C.sizeof(_lib.MinimizeConfig) == 8
    assert _lib.MinimizeConfig.delta.offset == 0 and _lib.MinimizeConfig.allow_nondet.offset == 4


def test_argument_validation_without_gpu(wfst_lib):
    from rustfst_amd import _lib
    out = C.c_void_p(1)
    for d in (0.0, -1e-3, float("nan"), float("inf")):
        cfg = _lib.MinimizeConfig(d, 0)
        assert "delta" in ko_message(wfst_lib.wfst_minimize(None, None, C.byref(cfg), C.byref(out)))
        assert out.value is None
    assert "null" in ko_message(wfst_lib.wfst_minimize(None, None, None, C.byref(out)))
    good = _lib.MinimizeConfig(1e-6, 1)
    assert "null" in ko_message(wfst_lib.wfst_minimize(None, None, C.byref(good), None))


def test_python_surface():
    import rustfst_amd
    cfg = rustfst_amd.MinimizeConfig()
    assert cfg.delta == 1e-6 and cfg.allow_nondet is False
    cfg = rustfst_amd.MinimizeConfig(delta=0.5, allow_nondet=True)
    assert cfg.delta == 0.5 and cfg.allow_nondet is True
    assert rustfst_amd.KSHORTESTDELTA == 1e-6
    for name in ("minimize", "minimize_with_config", "MinimizeConfig"):
        assert name in rustfst_amd.__all__ and callable(getattr(rustfst_amd, name))
    assert inspect.signature(rustfst_amd.DeviceFst.minimize).parameters["config"].default is None
    assert inspect.signature(rustfst_amd.VectorFst.minimize).parameters["config"].default is None


def test_k16_restatement_reproduces_the_derivations():
    """the hand derivations of K16_DERIVATION.md, replayed by this file's restatement (checks the restatement itself)"""
    cases = golden_cases()
    assert len(cases) >= 8
    for c in cases:
        delta, nondet = cfg_of(c)
        got = minimize_ref(golden_flat(c), delta, nondet)
        assert_flat_identical(got, golden_flat(c, "expected"), c["name"])
        for labels, weight in c.get("accepts", []):
            for f in (golden_flat(c), got):
                w = accepts(f, labels)
                assert (w is None) == (weight is None), (c["name"], labels)
                if w is not None:
                    assert abs(w - weight) <= 1e-5, (c["name"], labels, w)


def survivors_by_rule(fst):
    """the closed rule: at every height the class holding the height's highest state id keeps its highest id, every other
    class its lowest — on the connected, label-sorted FST acyclic_partition sees; returns {state: survivor}"""
    heights = fst_depth(fst)
    cls = [None] * len(heights)
    for h in range(max(heights) + 1):
        members = [s for s in range(len(heights)) if heights[s] == h]
        groups = {}
        for s in members:
            f = fst["finals"][s]
            k = (float(INF if f is None else f), len(fst["rows"][s]), tuple((tr[0], cls[tr[3]]) for tr in fst["rows"][s]))
            groups.setdefault(k, []).append(s)
        top = max(members)
        for g in groups.values():
            keep = max(g) if top in g else min(g)
            for s in g:
                cls[s] = keep
    return cls


def test_survivor_rule_against_the_partition_lists():
    rng = np.random.default_rng(16)
    several = 0
    for i in range(300):
        flat = trie_flat(rng, int(rng.integers(5, 50)), 3, 5, False) if i % 2 else random_dag(rng, int(rng.integers(2, 50)), 3, False)
        fst = flat_to_fst(flat)
        connect(fst)
        if not fst["rows"]:
            continue
        for row in fst["rows"]:
            row.sort(key=lambda t: t[0])
        part = acyclic_partition(fst)
        rule = survivors_by_rule(fst)
        for c in range(len(part.head)):
            mem = list(part.members(c))
            several += len(mem) > 1
            for s in mem:
                assert rule[s] == mem[0], (i, c, mem, rule[s])
    assert several > 300


def test_generator_shrinks_and_restatement_is_idempotent():
    cases = random_cases(7, 80)
    shrunk = reordered = 0
    for name, flat in cases:
        got = minimize_ref(flat)
        trimmed = flat_to_fst(flat)
        connect(trimmed)
        shrunk += got["n_states"] < len(trimmed["rows"])
        again = minimize_ref(got)
        assert_idempotent(again, got, name + " idempotent")
        reordered += not np.array_equal(again["arcs"]["ilabel"], got["arcs"]["ilabel"])
    assert 2 * shrunk >= len(cases), shrunk
    assert reordered > 0  # (the case assert_idempotent describes does occur)


def test_restatement_errors():
    nd = make_flat(2, 0, [[(1, 1, 0.0, 1), (1, 1, 0.0, 1)], []], [INF, 0.0])
    with pytest.raises(Unsupported, match="Refusing"):
        minimize_ref(nd)
    with pytest.raises(Unsupported, match="non-deterministic inputs"):
        minimize_ref(nd, allow_nondet=True)
    with pytest.raises(Unsupported, match="transducers"):
        minimize_ref(make_flat(2, 0, [[(1, 2, 0.0, 1)], []], [INF, 0.0]))
    with pytest.raises(Unsupported, match="cyclic"):
        minimize_ref(make_flat(2, 0, [[(1, 1, 0.0, 1)], [(1, 1, 0.0, 0)]], [INF, 0.0]))


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


def test_restatement_without_a_start_state():
    for flat, message in no_start_cases():
        if message is None:
            got = minimize_ref(flat)
            assert got["n_states"] == 0 and got["start"] is None and len(got["arcs"]) == 0
            assert got["props"] & (ACCESSIBLE | COACCESSIBLE | ACCEPTOR | UNWEIGHTED) == ACCESSIBLE | COACCESSIBLE | ACCEPTOR | UNWEIGHTED
        else:
            with pytest.raises(Unsupported, match=message):
                minimize_ref(flat)
    # the stored determinism bits: set_weight_unchecked on the one reweighted arc drops them, the recomputation does not
    # ask for them again
    assert not minimize_ref(no_start_cases()[1][0])["props"] & (I_DETERMINISTIC | O_DETERMINISTIC)


def test_restatement_keeps_both_arcs_when_merged_weights_are_far_apart():
    """what the reference does where the device answers KO: merge_states appends the member's arc, tr_unique's approximate
    == does not drop it, and the survivor ends with two arcs of one label"""
    for flat in far_apart_cases():
        got = minimize_ref(flat)
        assert got["n_states"] == 3
        seg = got["arcs"][got["offsets"][1]:got["offsets"][2]]
        assert seg["ilabel"].tolist() == [3, 3] and seg["nextstate"].tolist() == [2, 2]
        assert sorted(seg["weight"].tolist()) == sorted(F32(flat["arcs"]["weight"][2:4]).tolist())


# ================================================================ GPU
def dev_minimize(flat, ctx, delta=None, allow_nondet=False):
    import rustfst_amd
    cfg = None if delta is None and not allow_nondet else rustfst_amd.MinimizeConfig(delta, allow_nondet)
    return to_device(flat, ctx).minimize(cfg)


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


@pytest.mark.gpu
def test_k16_on_the_device(gpu_ctx, monkeypatch):
    for path in PATHS:
        monkeypatch.setenv("WFST_MINIMIZE_PATH", path)
        for c in golden_cases():
            delta, nondet = cfg_of(c)
            got_dev = dev_minimize(golden_flat(c), gpu_ctx, delta, nondet)
            assert_flat_identical(got_dev.to_flat(), golden_flat(c, "expected"), f"{c['name']} [{path}]")
            check_invariants(golden_flat(c), got_dev, delta, gpu_ctx, np.random.default_rng(1), c["name"])


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
def test_random_acceptors_match_the_restatement(gpu_ctx, monkeypatch, path):
    monkeypatch.setenv("WFST_MINIMIZE_PATH", path)
    rng = np.random.default_rng(3)
    cases = random_cases(11, 60)
    shrunk = 0
    for name, flat in cases:
        dev = to_device(flat, gpu_ctx)
        before = dev.to_flat()
        got_dev = dev.minimize()
        got = got_dev.to_flat()
        exp = minimize_ref(flat)
        assert_flat_identical(got, exp, f"{name} [{path}]")
        assert_flat_identical(dev.to_flat(), before, "source handle")
        trimmed = flat_to_fst(flat)
        connect(trimmed)
        shrunk += got["n_states"] < len(trimmed["rows"])
        check_invariants(flat, got_dev, KSHORTESTDELTA, gpu_ctx, rng, name)
    assert 2 * shrunk >= len(cases), shrunk


@pytest.mark.gpu
def test_determinized_lattices(gpu_ctx):
    """determinize -> minimize -> compose on handles, no download in between; the minimized lattice equals the restatement"""
    from helpers import random_fst_flat
    import rustfst_amd
    rng = np.random.default_rng(21)
    shrunk = 0
    for i in range(12):
        lat = random_fst_flat(rng, int(rng.integers(8, 40)), 3, 3, acyclic=True, weight_grid=1, max_w=3)
        lat["arcs"]["olabel"] = lat["arcs"]["ilabel"]
        lat["props"] = ACCEPTOR | ACYCLIC | INITIAL_ACYCLIC
        lat["finals"][-1] = 0.0
        det = to_device(lat, gpu_ctx).determinize()
        mini = det.minimize()
        det_flat, got = det.to_flat(), mini.to_flat()
        assert_flat_identical(got, minimize_ref(det_flat), f"lattice {i}")
        shrunk += got["n_states"] < det_flat["n_states"]
        check_invariants(det_flat, mini, KSHORTESTDELTA, gpu_ctx, rng, f"lattice {i}")
        if got["n_states"]:
            # (the weighted result's arcs are in first-occurrence order and its word says nothing about label order:
            # compose wants sorted labels, as in the reference; tr_sort works on the handle)
            comp = mini.tr_sort().compose(mini)
            assert comp.to_flat()["n_states"] >= got["n_states"]
    assert shrunk >= 3


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
def test_fan_out_above_64(gpu_ctx, monkeypatch, path):
    """two hub states with 200 arcs each that merge (a wave per state), next to one that differs in a single target"""
    monkeypatch.setenv("WFST_MINIMIZE_PATH", path)
    rng = np.random.default_rng(5)
    labs = rng.permutation(np.arange(1, 201))
    # states: 0 start -> 1, 2, 3 (hubs) -> 4..9 (leaves: 4, 5 final 0; 6, 7 final 1; 8, 9 one arc to 4 / 5)
    rows = [[(1, 1, 0.0, 1), (2, 2, 0.0, 2), (3, 3, 0.0, 3)], [], [], [], [], [], [], [], [(7, 7, 1.0, 4)], [(7, 7, 1.0, 5)]]
    for k, lab in enumerate(labs):
        t = (4, 6, 8)[k % 3]
        rows[1].append((int(lab), int(lab), float(k % 2), t))
        rows[2].append((int(lab), int(lab), float(k % 2), t + 1))
        rows[3].append((int(lab), int(lab), float(k % 2), t + 1 if k != 150 else 4 + (k + 1) % 3 * 2))
    finals = [INF, INF, INF, INF, 0.0, 0.0, 1.0, 1.0, INF, INF]
    for props in (ACCEPTOR, 0):
        flat = make_flat(10, 0, rows, finals, props)
        got_dev = dev_minimize(flat, gpu_ctx)
        got = got_dev.to_flat()
        assert_flat_identical(got, minimize_ref(flat), f"fan-out [{path}]")
        check_invariants(flat, got_dev, KSHORTESTDELTA, gpu_ctx, rng, f"fan-out [{path}]")
        nxt = got["arcs"]["nextstate"][:3]  # the start's three arcs: hubs 1 and 2 are one state, hub 3 another
        assert nxt[0] == nxt[1] != nxt[2] and got["n_states"] < 10
    unweighted = make_flat(10, 0, [[(a[0], a[1], 0.0, a[3]) for a in r] for r in rows], [INF] * 4 + [0.0] * 4 + [INF] * 2)
    got_dev = dev_minimize(unweighted, gpu_ctx)
    assert_flat_identical(got_dev.to_flat(), minimize_ref(unweighted), f"fan-out unweighted [{path}]")
    check_invariants(unweighted, got_dev, KSHORTESTDELTA, gpu_ctx, rng, f"fan-out unweighted [{path}]")


@pytest.mark.gpu
@pytest.mark.parametrize("delta", [1e-6, 1.0 / 1024.0])
def test_real_valued_weights(gpu_ctx, delta):
    rng = np.random.default_rng(9)
    for i in range(10):
        flat = random_dag(rng, int(rng.integers(5, 80)), 4, True, real=True)
        got_dev = dev_minimize(flat, gpu_ctx, delta)
        assert_flat_identical(got_dev.to_flat(), minimize_ref(flat, delta), f"real {i} delta {delta}")
        # (idempotent=False: the second push computes (w - d) + d at the start state, which need not round back to w on
        # real-valued weights; the second call is still compared bit for bit with the restatement of that call)
        check_invariants(flat, got_dev, delta, gpu_ctx, rng, f"real {i}", idempotent=False)


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


def test_closed_form_on_the_restatement():
    """the closed form of the scale test, checked on the CPU at k = 3 and k = 7 with the restatement itself"""
    rng = np.random.default_rng(33)
    m = closed_form_base(rng)
    exp = minimize_ref(m)
    assert exp["n_states"] == m["n_states"] and np.array_equal(exp["arcs"], m["arcs"])
    for k in (3, 7):
        assert_flat_identical(minimize_ref(blow_up(rng, m, k)), exp, f"k = {k}")


@pytest.mark.gpu
def test_scale_closed_form(gpu_ctx):
    rng = np.random.default_rng(33)
    m = closed_form_base(rng)
    for k in (3, (1 << 20) // m["n_states"] + 1):
        big = blow_up(rng, m, int(k))
        got_dev = dev_minimize(big, gpu_ctx)
        assert_flat_identical(got_dev.to_flat(), minimize_ref(m), f"k = {k}, {big['n_states']} states")
        check_invariants(big, got_dev, KSHORTESTDELTA, gpu_ctx, rng, f"k = {k}")
    assert big["n_states"] >= 1_000_000


@pytest.mark.gpu
def test_word_list(gpu_ctx):
    """200 k random words = random prefix + one of 300 suffixes: the suffixes are shared after minimization"""
    rng = np.random.default_rng(44)
    suffixes = [tuple(rng.integers(1, 6, size=int(rng.integers(3, 9))).tolist()) for _ in range(300)]
    words = set()
    while len(words) < 200_000:
        pre = rng.integers(1, 6, size=(20_000, 9))
        ln = rng.integers(6, 10, size=20_000)
        sx = rng.integers(0, 300, size=20_000)
        for p, l, x in zip(pre, ln, sx):
            words.add(tuple(p[:l].tolist()) + suffixes[x])
    words = sorted(words)
    # trie by sorted insertion (vectorised enough: a dict per depth)
    nxt, rows_src, rows_lab, rows_dst, final = {}, [], [], [], set()
    n = 1
    for w in words:
        s = 0
        for lab in w:
            key = (s, lab)
            t = nxt.get(key)
            if t is None:
                t = n
                n += 1
                nxt[key] = t
                rows_src.append(s)
                rows_lab.append(lab)
                rows_dst.append(t)
            s = t
        final.add(s)
    src = np.array(rows_src)
    order = np.argsort(src, kind="stable")
    arcs = np.zeros(len(src), dtype=TR_DTYPE)
    arcs["ilabel"] = arcs["olabel"] = np.array(rows_lab)[order]
    arcs["nextstate"] = np.array(rows_dst)[order]
    off = np.zeros(n + 1, dtype=np.uint32)
    off[1:] = np.cumsum(np.bincount(src, minlength=n))
    finals = np.full(n, np.inf, dtype=np.float32)
    finals[list(final)] = 0.0
    flat = dict(n_states=n, start=0, offsets=off, arcs=arcs, finals=finals, props=ACCEPTOR)
    mini = dev_minimize(flat, gpu_ctx)
    got = mini.to_flat()
    assert got["n_states"] < n // 2
    acc, co, cyc, _ = model.graph_facts(got)
    assert acc and co and not cyc
    for w in [words[i] for i in rng.integers(0, len(words), size=300)]:
        assert accepts(got, w) == 0.0
    for _ in range(300):
        w = tuple(rng.integers(1, 6, size=int(rng.integers(1, 18))).tolist())
        assert (accepts(got, w) is None) == (accepts(flat, w) is None)
    check_invariants(flat, mini, KSHORTESTDELTA, gpu_ctx, rng, "word list")
    # the number of states of the minimal automaton is unique: the sequential restatement agrees on it
    if n <= 3_000_000:
        assert minimize_ref(flat)["n_states"] == got["n_states"]


@pytest.mark.gpu
def test_errors(gpu_ctx):
    import rustfst_amd
    from rustfst_amd import _lib

    def ko(flat, match, **kw):
        with pytest.raises(rustfst_amd.WfstError, match=match):
            dev_minimize(flat, gpu_ctx, **kw)
        # (WfstError carries wfst_last_error's text: _lib.check reads it, which also clears it)
        out = C.c_void_p()
        cfg = _lib.MinimizeConfig(kw.get("delta") or 1e-6, 1 if kw.get("allow_nondet") else 0)
        src = to_device(flat, gpu_ctx)
        assert _lib.lib().wfst_minimize(gpu_ctx._h, src._h, C.byref(cfg), C.byref(out)) == 1 and out.value is None
        assert re.search(match, ko_message(1))

    nd = make_flat(3, 0, [[(1, 1, 0.0, 1), (1, 1, 1.0, 2)], [], []], [INF, 0.0, 0.0])
    for props in (0, ACCEPTOR | NOT_I_DETERMINISTIC | WEIGHTED):
        nd["props"] = props
        ko(nd, MSG_NONDET)
        ko(nd, "non-deterministic inputs are not supported", allow_nondet=True)
    tr = make_flat(2, 0, [[(1, 2, 0.0, 1)], []], [INF, 0.0])
    for props in (0, NOT_ACCEPTOR | I_DETERMINISTIC | UNWEIGHTED):
        tr["props"] = props
        ko(tr, "transducers are not supported")
    cyc = make_flat(3, 0, [[(1, 1, 1.0, 1)], [(1, 1, 0.0, 2), (2, 2, 0.0, 0)], []], [INF, INF, 0.0])
    for props in (0, ACCEPTOR | I_DETERMINISTIC | WEIGHTED | CYCLIC, ACCEPTOR):
        cyc["props"] = props
        ko(cyc, "cyclic inputs are not supported")
    cyc["arcs"]["weight"] = 0.0
    cyc["props"] = 0
    ko(cyc, "cyclic inputs are not supported")
    # merged states whose arc weights tr_unique would not unite: the reference keeps both arcs, the device says so
    for flat in far_apart_cases():
        ko(flat, "arc weights further than 1/1024 apart")
    # a weighted input without a start state: the empty FST when pushing leaves no weight, else the reference's error
    for flat, message in no_start_cases():
        if message is None:
            got = dev_minimize(flat, gpu_ctx).to_flat()
            assert_flat_identical(got, minimize_ref(flat), "no start state")
            assert got["n_states"] == 0 and got["start"] is None
        else:
            ko(flat, message)
    # the context still works, and empty results are the empty FST
    dead = make_flat(3, 0, [[(1, 1, 1.0, 1)], [(1, 1, 2.0, 2)], []], [INF, INF, INF], ACCEPTOR)
    for f in (dead, make_flat(2, None, [[(1, 1, 0.0, 1)], []], [INF, 0.0], ACCEPTOR), make_flat(0, None, [], [], 0)):
        got = dev_minimize(f, gpu_ctx).to_flat()
        assert_flat_identical(got, minimize_ref(f), "empty")
        assert got["n_states"] == 0 and got["start"] is None


# ---------------------------------------------------------------- the facts of an arc, one at a time
# (fact bit, its pair in the property word when the fact is present / absent): fst_props.h FACT_* and add_trs_by_facts
FACT_PAIRS = ((1, NOT_ACCEPTOR, ACCEPTOR), (2, I_EPSILONS, NO_I_EPSILONS), (4, EPSILONS, NO_EPSILONS), (8, O_EPSILONS, NO_O_EPSILONS),
              (16, NOT_I_LABEL_SORTED, I_LABEL_SORTED), (32, NOT_O_LABEL_SORTED, O_LABEL_SORTED), (64, WEIGHTED, UNWEIGHTED),
              (128, NOT_TOP_SORTED, TOP_SORTED))
_KD_UP = float(np.nextafter(model.KDELTA, F32(1.0)))


def _fact_fst(rows, finals=(INF, INF, INF), start=2):
    return make_flat(3, start, rows, list(finals))


# name -> (the FST, the facts reverse() finds).  Three states, start 2, arcs running down (2 -> 1 -> 0) and no final state
# unless the fact needs one: reverse() then adds no super-initial arcs and turns every arc s -> t into (t + 1) -> (s + 1), which
# runs upwards, so the reversed FST's arcs carry exactly the facts listed (a fact that implies another, as eps:eps does,
# brings it along).  minimize() sees the same arcs from their own side, running downwards (always "nextstate <= state").
FACT_CASES = {
    "none": (_fact_fst([[], [(4, 4, 0.0, 0)], [(3, 3, 0.0, 1)]]), 0),
    "1_not_acceptor": (_fact_fst([[], [(4, 4, 0.0, 0)], [(3, 4, 0.0, 1)]]), 1),
    "2_ilabel_epsilon": (_fact_fst([[], [(4, 4, 0.0, 0)], [(0, 4, 0.0, 1)]]), 1 | 2),
    "4_epsilon": (_fact_fst([[], [(4, 4, 0.0, 0)], [(0, 0, 0.0, 1)]]), 2 | 4 | 8),
    "8_olabel_epsilon": (_fact_fst([[], [(4, 4, 0.0, 0)], [(3, 0, 0.0, 1)]]), 1 | 8),
    # two arcs of one state into one state: the pair is consecutive for minimize() and, reversed, for reverse()
    # (state 0's in-arcs, in reverse()'s order: the one from state 1, then these two)
    "16_ilabel_order": (_fact_fst([[], [(1, 1, 0.0, 0)], [(5, 3, 0.0, 0), (3, 4, 0.0, 0)]]), 1 | 16),
    "32_olabel_order": (_fact_fst([[], [(1, 1, 0.0, 0)], [(3, 5, 0.0, 0), (4, 3, 0.0, 0)]]), 1 | 32),
    # is_one is the approximate ==: a weight of exactly KDELTA is still one, the next f32 is a weight
    "64_weight_kdelta": (_fact_fst([[], [(4, 4, 0.0, 0)], [(3, 3, float(model.KDELTA), 1)]]), 0),
    "64_weight_above_kdelta": (_fact_fst([[], [(4, 4, 0.0, 0)], [(3, 3, _KD_UP, 1)]]), 64),
    "64_weighted": (_fact_fst([[], [(4, 4, 0.75, 0)], [(3, 3, 0.0, 1)]]), 64),
    # one arc running up, 0 -> 1: reversed it runs down
    "128_not_top_sorted": (_fact_fst([[(3, 3, 0.0, 1)], [], [(4, 4, 0.0, 1)]]), 128),
    # ... and all of them running up from start 0: minimize() finds no fact at all, reverse() finds both arcs running down
    "128_top_sorted_for_minimize": (_fact_fst([[(3, 3, 0.0, 1)], [(4, 4, 0.0, 2)], []], start=0), 128),
    # a final weight that is not one (minimize.hip's FACT_FINAL_WEIGHTED): reverse() turns it into the weight of the
    # super-initial state's eps:eps arc
    "256_final_weight": (_fact_fst([[], [(4, 4, 0.0, 0)], [(3, 3, 0.0, 1)]], finals=(F32(0.75), INF, INF)), 2 | 4 | 8 | 64),
    "256_final_weight_kdelta": (_fact_fst([[], [(4, 4, 0.0, 0)], [(3, 3, 0.0, 1)]], finals=(model.KDELTA, INF, INF)), 2 | 4 | 8),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FACT_CASES))
def test_each_arc_fact_reaches_the_property_word(gpu_ctx, oracle, name):
    """One tiny FST per fact of fst_props.h's arc_facts (and FACT_FINAL_WEIGHTED), uploaded with an EMPTY property word, so
    that reverse() (rev_facts_kernel and the host loop over the super-initial arcs) and minimize() (facts_kernel) have to
    find the fact in the content.  reverse(): FST and word are the oracle's, and the word holds, pair by pair, the negative
    bit of every listed fact and the positive bit of every other one.  minimize(): FST and word are the restatement's, or
    both refuse the input in the same words (a transducer)."""
    from helpers import to_oracle
    import rustfst_amd
    flat, rev_facts = FACT_CASES[name]
    assert flat["props"] == 0
    got = to_device(flat, gpu_ctx).reverse().to_flat()
    assert_flat_identical(got, to_oracle(oracle, flat).reverse().to_flat(), f"reverse {name}")
    for bit, present, absent in FACT_PAIRS:
        assert got["props"] & (present | absent) == (present if rev_facts & bit else absent), f"reverse {name}: fact {bit}"
    try:
        want = minimize_ref(flat)
    except Unsupported as e:
        with pytest.raises(rustfst_amd.WfstError, match=re.escape(e.args[0])):
            dev_minimize(flat, gpu_ctx)
    else:
        assert_flat_identical(dev_minimize(flat, gpu_ctx).to_flat(), want, f"minimize {name}")
