"""Inputs of the isomorphic / invert tests (tests/test_isomorphic*.py, tests/test_invert_gpu.py), each defined once: the K22
golden file, the seeded parity families with their mutations, and the FSTs at the limits of isomorphic.hip.  FSTs are in the
rows form of oracle.model (dict(rows, finals, start, props)); holds no test."""
import json
import os
import struct

import numpy as np

from oracle.model import F32, flat_to_fst

import helpers
import inputs
from rustfst_amd import synth

K22 = os.path.join(helpers.ROOT, "tests", "golden", "k22_isomorphic.json")
# the narrow limits as the tests expect them (tests/test_isomorphic.py compares them with the three places that state them)
NARROW_PAIRS, NARROW_EVENTS, WAVE_ARCS, RANK_MAX = 256, 2048, 64, 256
PATHS = ("auto", "narrow", "wide")


def _weight(w):
    if isinstance(w, str):
        if w.startswith("0x"):
            return F32(struct.unpack("<f", struct.pack("<I", int(w, 16)))[0])
        return F32(float(w))
    return F32(w)


def from_spec(spec):
    return dict(rows=[[[il, ol, _weight(w), ns] for il, ol, w, ns in row] for row in spec["rows"]],
                finals=[None if w is None else _weight(w) for w in spec["finals"]], start=spec["start"], props=0)


def k22():
    with open(K22) as f:
        return json.load(f)


def k22_cases():
    """(name, fst1, fst2, delta or None, expected)"""
    return [(c["name"], from_spec(c["fst1"]), from_spec(c["fst2"]), c["delta"], c["expected"]) for c in k22()["cases"]]


# ---------------------------------------------------------------- parity families
def permuted(fst, rng):
    """the states renumbered by a random permutation, the arcs of every state shuffled"""
    n = len(fst["rows"])
    perm = [int(x) for x in rng.permutation(n)]  # old -> new
    rows, finals = [None] * n, [None] * n
    for s in range(n):
        row = [[il, ol, w, perm[ns]] for il, ol, w, ns in fst["rows"][s]]
        rng.shuffle(row)
        rows[perm[s]], finals[perm[s]] = row, fst["finals"][s]
    return dict(rows=rows, finals=finals, start=None if fst["start"] is None else perm[fst["start"]], props=0)


def _copy(fst):
    return dict(rows=[[list(a) for a in row] for row in fst["rows"]], finals=list(fst["finals"]), start=fst["start"], props=0)


def reached(fst):
    """the states the start reaches, in breadth-first order"""
    if fst["start"] is None:
        return []
    seen, order = {fst["start"]}, [fst["start"]]
    for s in order:
        for a in fst["rows"][s]:
            if a[3] not in seen:
                seen.add(a[3])
                order.append(a[3])
    return order


MUTATIONS = ("label", "weight_within_delta", "weight_beyond_delta", "final", "destination", "added_arc", "duplicated_arcs")


def mutated(fst, kind, rng):
    """a copy of fst with one mutation of `kind` at a state the start reaches (None: fst has no arc to mutate)"""
    out = _copy(fst)
    states = reached(out)
    with_arcs = [s for s in states if out["rows"][s]]
    if not with_arcs:
        return None
    s = with_arcs[int(rng.integers(0, len(with_arcs)))]
    row = out["rows"][s]
    k = int(rng.integers(0, len(row)))
    if kind == "label":
        row[k][int(rng.integers(0, 2))] += 1000
    elif kind == "weight_within_delta":
        row[k][2] = F32(F32(row[k][2]) + F32(1.0 / 4096.0))
    elif kind == "weight_beyond_delta":
        row[k][2] = F32(F32(row[k][2]) + F32(1.0 / 256.0))
    elif kind == "final":
        t = states[int(rng.integers(0, len(states)))]
        out["finals"][t] = F32(0.25) if out["finals"][t] is None else None
    elif kind == "destination":
        row[k][3] = int((row[k][3] + 1 + rng.integers(0, max(1, len(out["rows"]) - 1))) % len(out["rows"]))
    elif kind == "added_arc":
        row.append([int(rng.integers(1, 9)), int(rng.integers(1, 9)), F32(0.5), states[int(rng.integers(0, len(states)))]])
    elif kind == "duplicated_arcs":
        row.append([row[k][0], row[k][1], row[k][2], states[int(rng.integers(0, len(states)))]])
    return out


def with_twin_arcs(fst, rng, count):
    """`count` arcs doubled (same labels and weight) towards another state: non-determinism as an unweighted automaton"""
    out = _copy(fst)
    states = reached(out)
    with_arcs = [s for s in states if out["rows"][s]]
    for _ in range(count if with_arcs else 0):
        s = with_arcs[int(rng.integers(0, min(len(with_arcs), 4)))]  # near the start: marked early in the search
        a = out["rows"][s][int(rng.integers(0, len(out["rows"][s])))]
        out["rows"][s].append([a[0], a[1], a[2], states[int(rng.integers(0, len(states)))]])
    return out


def _dag(seed):
    rng = np.random.default_rng(22000 + seed)
    n = int(rng.integers(5, 401))
    fst = inputs.random_shuffled_dag(rng, n, max_arcs_per_state=2, start=0)
    fst["start"] = max(range(n), key=lambda s: len(reached(dict(fst, start=s))))  # lattice-like: the start sees most of it
    return fst, rng


def _cyclic(seed):
    rng = np.random.default_rng(22500 + seed)
    n = int(rng.integers(5, 401))
    flat = synth.make_transducer(n, int(rng.integers(1, 5)), 6, 0.1, seed=700 + seed, p_final=0.3)
    return flat_to_fst(flat), rng


FAMILIES = {"dag": (_dag, 8), "cyclic": (_cyclic, 8)}


def family(name):
    """(case name, fst1, fst2) of the family: per seed the base (every other seed with twin arcs) against its permuted copy
    and against the permuted copy of each mutation"""
    make, seeds = FAMILIES[name]
    out = []
    for seed in range(seeds):
        base, rng = make(seed)
        if seed % 2:
            base = with_twin_arcs(base, rng, 1 + seed % 3)
        out.append(("%s-%d-permuted" % (name, seed), base, permuted(base, rng)))
        for kind in MUTATIONS:
            m = mutated(base, kind, rng)
            if m is not None:
                out.append(("%s-%d-%s" % (name, seed, kind), base, permuted(m, rng)))
    return out


# ---------------------------------------------------------------- the limits of isomorphic.hip
def hub(deg, rng, negative=False, n_targets=None):
    """state 0 with `deg` arcs over a few labels (many equal label pairs, weights on a coarse grid: the sort has to look at
    every part of the key) into n_targets final states"""
    t = n_targets or min(deg, 7)
    rows = [[[int(rng.integers(1, 4)), int(rng.integers(1, 4)), F32((rng.integers(0, 64) - (32 if negative else 0)) / 8.0),
              1 + int(rng.integers(0, t))] for _ in range(deg)]] + [[] for _ in range(t)]
    return dict(rows=rows, finals=[None] + [F32(s) for s in range(t)], start=0, props=0)


def fan(width, arcs_per_state=0):
    """level 2 of exactly `width` pairs: the start has one arc (label k + 1) to each of them; each has `arcs_per_state` arcs
    (labels 1 ..) to one final sink"""
    sink = width + 1
    rows = [[[k + 1, k + 1, F32(0.0), k + 1] for k in range(width)]]
    rows += [[[j + 1, j + 1, F32(k % 5), sink] for j in range(arcs_per_state)] for k in range(width)]
    rows.append([])
    return dict(rows=rows, finals=[None] * (width + 1) + [F32(0.0)], start=0, props=0)


def diamond(width, tail=3):
    """1 -> 2 -> `width` -> 2 -> 1 -> .. : narrow levels, one wide level, narrow levels again"""
    rows, finals = [], []

    def state(row, final=None):
        rows.append(row)
        finals.append(final)
        return len(rows) - 1
    n_mid = width
    # ids: 0 start, 1..2 level 2, 3..3+width-1 level 3, then two joins, then a tail chain
    first_mid, join0 = 3, 3 + n_mid
    state([[1, 1, F32(0.0), 1], [2, 2, F32(0.0), 2]])
    half = n_mid // 2
    state([[k + 1, k + 1, F32(0.5), first_mid + k] for k in range(half)])
    state([[k + 1, k + 1, F32(0.5), first_mid + k] for k in range(half, n_mid)])
    for k in range(n_mid):
        state([[7, 7, F32(k % 3), join0 + (k % 2)]])
    state([[1, 1, F32(0.0), join0 + 2]])
    state([[2, 2, F32(0.0), join0 + 2]])
    for k in range(tail):
        state([[3, 3, F32(1.0), join0 + 3 + k]])
    state([], F32(0.0))
    return dict(rows=rows, finals=finals, start=0, props=0)


def chain(n):
    rows = [[[1 + s % 5, 1 + s % 3, F32((s % 7) / 4.0), s + 1]] for s in range(n - 1)] + [[]]
    return dict(rows=rows, finals=[None] * (n - 1) + [F32(0.0)], start=0, props=0)
