"""Inputs of the sigma-matcher tests (tests/test_compose_sigma.py on the CPU, tests/test_compose_sigma_gpu.py on the device):
the K21 known answers, seeded random pairs and the hand-built machines at the limits of compose_sigma.hip.  Everything is
in the rows form of oracle.model; configs are sigma_ref's (sigma_label, rewrite_mode, allowed)."""
import json
import os

import numpy as np

from oracle.model import (ACCEPTOR, I_LABEL_SORTED, O_LABEL_SORTED, content_word_of_flat, flat_to_fst, fst_to_flat,
                          rows_flat)
from oracle.model.props import NOT_I_LABEL_SORTED, NOT_O_LABEL_SORTED

from helpers import random_fst_flat

import sigma_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
INF = np.inf
SORT_BITS = I_LABEL_SORTED | NOT_I_LABEL_SORTED | O_LABEL_SORTED | NOT_O_LABEL_SORTED
FILTERS = (R.NULL, R.TRIVIAL, R.SEQUENCE, R.ALT_SEQUENCE, R.MATCH, R.NO_MATCH)


def k21():
    with open(os.path.join(HERE, "golden", "k21_sigma_matcher.json")) as f:
        return json.load(f)


def from_spec(spec, sort_bits=I_LABEL_SORTED | O_LABEL_SORTED):
    """a golden FST spec under the word of its content plus `sort_bits` (every K21 machine is sorted on both tapes)"""
    rows = [[] for _ in range(spec["n_states"])]
    for s, il, ol, w, ns in spec["arcs"]:
        rows[s].append((il, ol, w, ns))
    finals = [INF] * spec["n_states"]
    for s, w in spec["finals"]:
        finals[s] = w
    return with_content_word(flat_to_fst(rows_flat(rows, finals, start=spec["start"])), sort_bits)


def to_spec(fst):
    return dict(n_states=len(fst["rows"]), start=fst["start"],
                arcs=[[s, int(t[0]), int(t[1]), float(t[2]), int(t[3])] for s, r in enumerate(fst["rows"]) for t in r],
                finals=[[s, float(w)] for s, w in enumerate(fst["finals"]) if w is not None])


def sortedness(fst):
    """the four label-order bits, truthfully"""
    il = all(r[k][0] <= r[k + 1][0] for r in fst["rows"] for k in range(len(r) - 1))
    ol = all(r[k][1] <= r[k + 1][1] for r in fst["rows"] for k in range(len(r) - 1))
    return (I_LABEL_SORTED if il else NOT_I_LABEL_SORTED) | (O_LABEL_SORTED if ol else NOT_O_LABEL_SORTED)


def with_content_word(fst, sort_bits=None):
    """the word compute_fst_properties finds in the content, with the label-order bits replaced by `sort_bits` (default:
    the truth)"""
    word = int(content_word_of_flat(fst_to_flat(fst))) & ~SORT_BITS
    return dict(fst, props=word | (sortedness(fst) if sort_bits is None else sort_bits))


def with_sort_word(fst, acceptor=False):
    """the word of the seeded random machines: the label-order bits, truthfully, and ACCEPTOR where the maker copied a tape
    (cyclic and weighted: oracle.model does not restate the SCC test the full word would need)"""
    return dict(fst, props=sortedness(fst) | (ACCEPTOR if acceptor else 0))


def machine(rows, finals, start=0, sort_bits=None):
    return with_content_word(flat_to_fst(rows_flat(rows, finals, start=start)), sort_bits)


def golden_pair(oracle):
    """sigma-matcher-2 left / right, sorted as the reference's test sorts them (sigma_matcher.rs:564-565)"""
    out = []
    for name, by_olabel in (("left", True), ("right", False)):
        with open(os.path.join(HERE, "golden", "sigma_matcher_2_%s.fst" % name), "rb") as f:
            o = oracle.OracleFst.load(f.read())
        o.tr_sort(by_olabel=by_olabel)
        out.append(flat_to_fst(o.to_flat()))
    return out


def count_paths(fst):
    """complete paths of an acyclic FST"""
    memo = {}

    def rec(s):
        if s not in memo:
            memo[s] = (fst["finals"][s] is not None) + sum(rec(t[3]) for t in fst["rows"][s])
        return memo[s]
    return rec(fst["start"]) if fst["start"] is not None else 0


# ---------------------------------------------------------------- random pairs
SIGMA1, SIGMA2 = 3, 4  # inside the alphabet 1..5


def _sorted_rows(fst, key):
    return dict(fst, rows=[sorted(r, key=lambda t: t[key]) for r in fst["rows"]])  # (stable)


def _relabel(fst, tape, frm, to, rng, keep):
    """label `frm` on `tape` becomes `to`, except with probability `keep`"""
    for r in fst["rows"]:
        for t in r:
            if t[tape] == frm and rng.random() >= keep:
                t[tape] = to
    return fst


def random_pair(seed, side, acceptor, plain_unsorted):
    """(fst1, fst2, m1, m2) without rewrite mode (the caller fills it in): 6-30 states over labels 1..5, epsilons on both
    tapes.  side: 1, 2 or 3 (both).  The sigma operand(s) sorted on the matched tape; the other operand sorted too (BOTH mode)
    or, with `plain_unsorted`, left in random order under NOT_*_LABEL_SORTED.  `acceptor`: the sigma operand(s) copy the
    matched tape onto the other one and say ACCEPTOR.  The other side's arcs labelled with the searched sigma are mostly
    relabelled: each that stays can end the call in "bad label"."""
    rng = np.random.default_rng(seed)
    n1, n2 = int(rng.integers(6, 31)), int(rng.integers(6, 31))
    f1 = flat_to_fst(random_fst_flat(rng, n1, 3, 5, p_eps_i=0.1, p_eps_o=0.15, p_final=0.3, sort="none", min_fanout=1))
    f2 = flat_to_fst(random_fst_flat(rng, n2, 3, 5, p_eps_i=0.2, p_eps_o=0.1, p_final=0.3, sort="none", min_fanout=1))
    sg1, sg2 = side in (1, 3), side in (2, 3)
    if acceptor:
        if sg1:
            f1["rows"] = [[[t[1], t[1], t[2], t[3]] for t in r] for r in f1["rows"]]
        if sg2:
            f2["rows"] = [[[t[0], t[0], t[2], t[3]] for t in r] for r in f2["rows"]]
    if sg2:  # fst1's output labels are looked up in matcher2 wherever fst1 is iterated
        _relabel(f1, 1, SIGMA2, 5, rng, keep=0.02)
    if sg1:
        _relabel(f2, 0, SIGMA1, 5, rng, keep=0.02)
    if sg1 and sg2:  # a pair of states that both carry a sigma arc ends the call: thin the sigma arcs out
        _relabel(f1, 1, SIGMA1, 1, rng, keep=0.25)
        _relabel(f2, 0, SIGMA2, 2, rng, keep=0.25)
    if sg1 or not plain_unsorted:
        f1 = _sorted_rows(f1, 1)
    if sg2 or not plain_unsorted:
        f2 = _sorted_rows(f2, 0)
    f1, f2 = with_sort_word(f1, acceptor and sg1), with_sort_word(f2, acceptor and sg2)
    if plain_unsorted:  # the plain side must SAY it is unsorted, whatever its random order happens to be
        if not sg1:
            f1["props"] = (f1["props"] & ~(O_LABEL_SORTED | NOT_O_LABEL_SORTED)) | NOT_O_LABEL_SORTED
        if not sg2:
            f2["props"] = (f2["props"] & ~(I_LABEL_SORTED | NOT_I_LABEL_SORTED)) | NOT_I_LABEL_SORTED
    return f1, f2, (SIGMA1 if sg1 else None), (SIGMA2 if sg2 else None)


def has_sigma_state_with_ieps(fst, sigma):
    return any(any(t[0] == sigma for t in r) and any(t[0] == 0 for t in r) for r in fst["rows"])


def grid(side, plain_unsorted):
    """the cases of one (side, mode): filter x rewrite mode x acceptor / transducer, each on a pair of its own"""
    k = 0
    for flt in FILTERS:
        for rw in (0, 1, 2):
            for acc in (False, True):
                seed = 1000 * side + 500 * int(plain_unsorted) + k
                k += 1
                f1, f2, s1, s2 = random_pair(seed, side, acc, plain_unsorted)
                yield dict(name="side%d-%s-f%d-rw%d-%s-seed%d" % (side, "one" if plain_unsorted else "both", flt, rw,
                                                                  "acc" if acc else "tr", seed),
                           f1=f1, f2=f2, filter=flt, m1=None if s1 is None else (s1, rw, None),
                           m2=None if s2 is None else (s2, rw, None))


GRIDS = [(1, False), (1, True), (2, False), (2, True), (3, False)]


def run_ref(case, connect=False):
    """(result, info) or (SigmaError message, None)"""
    info = {}
    try:
        return R.compose_sigma(case["f1"], case["f2"], case["filter"], connect, case["m1"], case["m2"], info), info
    except R.SigmaError as e:
        return e.args[0], None


# ---------------------------------------------------------------- the limits of the kernel
def chain_query(labels, sort_bits=I_LABEL_SORTED | O_LABEL_SORTED):
    """utils::acceptor: a string acceptor"""
    n = len(labels)
    return machine([[(l, l, 0.0, i + 1)] for i, l in enumerate(labels)] + [[]], [INF] * n + [0.0], sort_bits=sort_bits)


def fan_query(labels, weight=0.25):
    """one state with an arc per label into a final state: len(labels) + 1 items at the start state"""
    return machine([[(l, l, weight * (k % 5), 1) for k, l in enumerate(sorted(labels))], []], [INF, 0.5])


def sigma_state(explicit, sigma_arcs, n_next=2):
    """fst2: a start state with `explicit` input labels (x:x+100 each) and `sigma_arcs` [(il, ol)] in label order, all into
    state 1, which is final"""
    row = [(x, x + 100, 0.5, 1) for x in explicit] + [(il, ol, 1.0 + 0.25 * k, 1) for k, (il, ol) in enumerate(sigma_arcs)]
    row.sort(key=lambda t: t[0])
    return machine([row, []], [INF, 0.0])
