"""Input families and kernel-route restatements that more than one test module, or a tool, uses."""
import json
import os

import numpy as np

from rustfst_amd import synth
from rustfst_amd._lib import TR_DTYPE

from oracle.model.props import ACCEPTOR, determinize_props
from helpers import ROOT, make_fst


# ================================================================ determinize
def twin_copy(n, seed=3):
    """D = make_transducer(n) with the first arc per (state, ilabel), olabel = ilabel; N on 2n states (every arc four
    times, the copy +0.5), finals f(q) on both copies.  Returns (N, expected det(N)): D in FIFO first-touch order from
    {(0, 0)}, the other states {(r, 0), (r + n, 0.5)}, D's weights and finals."""
    t = synth.make_transducer(n, seed=seed)
    off, arcs = t["offsets"].astype(np.int64), t["arcs"]
    src = np.repeat(np.arange(n), np.diff(off))
    keep = np.ones(len(arcs), bool)
    keep[1:] = (src[1:] != src[:-1]) | (arcs["ilabel"][1:] != arcs["ilabel"][:-1])
    src, da = src[keep], arcs[keep].copy()
    da["olabel"] = da["ilabel"]
    doff = np.zeros(n + 1, np.int64)
    np.add.at(doff, src + 1, 1)
    doff = np.cumsum(doff)
    deg = np.diff(doff)
    fin = t["finals"].astype(np.float32)
    # N: state q (q < n) and q + n both carry, per kept arc (a, w, r): (a, w, r), (a, w + 0.5, r + n)
    nd = 2 * deg
    noff = np.concatenate([[0], np.cumsum(np.concatenate([nd, nd]))]).astype(np.uint32)
    one = np.empty(2 * len(da), TR_DTYPE)
    one["ilabel"] = np.repeat(da["ilabel"], 2)
    one["olabel"] = one["ilabel"]
    one["weight"] = np.repeat(da["weight"], 2)
    one["weight"][1::2] = da["weight"] + np.float32(0.5)
    one["nextstate"] = np.repeat(da["nextstate"], 2)
    one["nextstate"][1::2] = da["nextstate"] + n
    N = dict(n_states=2 * n, start=0, offsets=noff, arcs=np.concatenate([one, one]),
             finals=np.concatenate([fin, fin]), props=ACCEPTOR)
    # expected: BFS over D; id 0 = the start subset, D state r -> its own id the first time an arc reaches it
    ids = np.full(n, -1, np.int64)
    order = [0]  # D state of every result state (the start first)
    frontier = np.array([0])
    out_rows = []
    next_id = 1
    while len(frontier):
        seg = [np.arange(doff[q], doff[q + 1]) for q in frontier]
        idx = np.concatenate(seg) if seg else np.zeros(0, np.int64)
        tgt = da["nextstate"][idx].astype(np.int64)
        new = tgt[ids[tgt] < 0]
        _, first = np.unique(new, return_index=True)
        fresh = new[np.sort(first)]
        ids[fresh] = next_id + np.arange(len(fresh))
        next_id += len(fresh)
        order += list(fresh)
        out_rows.append((idx, ids[tgt]))
        frontier = fresh
    idx = np.concatenate([r[0] for r in out_rows])
    dst = np.concatenate([r[1] for r in out_rows])
    exp_arcs = np.empty(len(idx), TR_DTYPE)
    exp_arcs["ilabel"] = da["ilabel"][idx]
    exp_arcs["olabel"] = da["ilabel"][idx]
    exp_arcs["weight"] = da["weight"][idx]
    exp_arcs["nextstate"] = dst
    order = np.array(order)
    exp = dict(n_states=len(order), start=0,
               offsets=np.concatenate([[0], np.cumsum(deg[order])]).astype(np.uint32), arcs=exp_arcs,
               finals=fin[order], props=determinize_props(ACCEPTOR, True))
    return N, exp


def diamond_chain(levels, seed=11):
    """start 0 -> {1, 2}; states 2k-1, 2k each with arcs (label 1) into 2k+1 and 2k+2; the last two states final"""
    rng = np.random.default_rng(seed)
    n = 2 * levels + 1
    rows = [[(1, 1, 0.0, 1), (1, 1, 1.0, 2)]]
    for s in range(1, n):
        if s < n - 2:
            base = 2 * ((s + 1) // 2) + 1
            rows.append([(1, 1, float(rng.integers(0, 4)), base), (1, 1, float(rng.integers(0, 4)), base + 1)])
        else:
            rows.append([])
    arcs = np.array([x for r in rows for x in r], dtype=TR_DTYPE)
    offsets = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint32)
    fin = np.full(n, np.inf, np.float32)
    fin[n - 2:] = [0.0, 2.0]
    return dict(n_states=n, start=0, offsets=offsets, arcs=arcs, finals=fin, props=ACCEPTOR)


# ================================================================ top_sort, the rational operations
TOP_SORT_GOLDEN = os.path.join(ROOT, "tests", "golden", "k19_top_sort.json")


def top_sort_golden():
    with open(TOP_SORT_GOLDEN) as f:
        return json.load(f)


def random_shuffled_dag(rng, n, max_arcs_per_state=3, start=None):
    """n states in a hidden topological order; arcs (multi-arcs too) from earlier to later places, rows shuffled; some states
    the start cannot reach; the start anywhere"""
    place = rng.permutation(n)  # place[k] = the state at topological place k
    rows = [[] for _ in range(n)]
    if n > 1:
        for _ in range(int(rng.integers(0, max_arcs_per_state * n + 1))):
            a, b = sorted(int(x) for x in rng.choice(n, 2, replace=False))
            il = int(rng.integers(0, 4))
            rows[place[a]].append([il, il if rng.random() < 0.5 else int(rng.integers(0, 4)), float(rng.integers(0, 9)) / 4, int(place[b])])
        if rng.random() < 0.5:  # a doubled arc
            src = [s for s in range(n) if rows[s]]
            if src:
                s = src[int(rng.integers(0, len(src)))]
                rows[s].append(list(rows[s][0]))
    for r in rows:
        rng.shuffle(r)
    finals = [float(rng.integers(0, 8)) / 4 if rng.random() < 0.4 else None for _ in range(n)]
    return make_fst(rows, finals, int(rng.integers(0, n)) if start is None else start)


def chain(n, rng, finals_from=None, fan=1, start=0):
    """n states; state s has `fan` arcs into later states (none from the last); finals at states >= finals_from"""
    rows = [[[int(rng.integers(1, 9)), int(rng.integers(1, 9)), float(rng.integers(0, 16)) / 8,
              int(rng.integers(s + 1, n))] for _ in range(fan)] if s + 1 < n else [] for s in range(n)]
    ff = n - 1 if finals_from is None else finals_from
    return make_fst(rows, [float(rng.integers(0, 8)) / 4 if s >= ff else None for s in range(n)], start)
