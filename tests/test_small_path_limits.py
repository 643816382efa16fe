"""The two one-wavefront-per-FST kernels of nbest_batch.hip at every limit.  An item that does not fit a kernel goes through
a slower path that returns the same FST, so a wrong limit, a guard that fires early or a branch that never runs changes no
result: only the counters of wfst_ctx_get_small_path_stats show which path answered.  Without a GPU: the symbol, the
generators' exact sizes, a Python restatement of the routing rules and of the n-best search's tree growth, and the counters
both predict for every input list used below.  On the device: every result against the oracle AND against the general path
on the same handles, bit for bit including the property word, and the counters against the prediction.

Weights are on the 1/4 grid (many ties) or the 1/512 grid (few): sums of them are exact in f32 and in Python floats alike,
which is what lets the restatement compute distances and search keys with Python floats."""
import functools

import numpy as np
import pytest

from rustfst_amd._lib import TR_DTYPE
from rustfst_amd import synth

import helpers
from helpers import (NOT_O_LABEL_SORTED, _flat, assert_flat_identical, check_nbest_against_brute_force, empty_flat,
                     enumerate_paths, to_device, to_oracle)
from small_path_cases import (forward_distances, has_negative, has_start, n_arcs, nbest_offered, nbest_tree_entries,
                              predict_nbest, ring_with_chords, tree_capacity)

INF = float("inf")
# ---- the limits of nbest_batch.hip, restated (include/wfst.h states them in numbers)
SP1_MAX_STATES, SP1_MAX_ARCS, SP1_LONE_ARCS = 4096, 16384, 2048
SP1_STAGE_STATES, SP1_STAGE_ARCS = 2048, 4096
COUNTERS = ("n1_in_kernel", "n1_staged", "n1_handed_back", "nbest_in_kernel", "nbest_tree_full", "nbest_out_full",
            "nbest_tree_capacity")


# ================================================================ generators
def reversed_chain(n):
    """start state n - 1, arcs s -> s - 1, state 0 final: numbered against its direction, so a round of relaxation in
    state order moves the frontier by one state — n - 1 improving rounds and a quiet one; the only path visits all n states"""
    rows = [[]] + [[(1 + s % 5, 1 + s % 3, (1 + s % 7) / 4.0, s - 1)] for s in range(1, n)]
    finals = np.full(n, np.inf, dtype=np.float32)
    finals[0] = 0.5
    return _flat(n, n - 1, rows, finals)


def complete(n, seed):
    """every ordered pair of distinct states has an arc, integer weights 0..7; the last state is final"""
    rng = np.random.default_rng(seed)
    rows = [[(t + 1, t + 1, float(rng.integers(0, 8)), t) for t in range(n) if t != s] for s in range(n)]
    finals = np.full(n, np.inf, dtype=np.float32)
    finals[n - 1] = 0.0
    return _flat(n, 0, rows, finals)


def parallel_chain(n, labels, extra=0):
    """`labels` parallel arcs s -> s + 1 with distinct labels (an acceptor whose reversed form is deterministic); the first
    `extra` states carry one more, with its own label"""
    rows = [[(l, l, ((l * 3 + s) % 8) / 4.0, s + 1) for l in range(1, labels + 1 + (1 if s < extra else 0))] for s in range(n - 1)] + [[]]
    finals = np.full(n, np.inf, dtype=np.float32)
    finals[n - 1] = 0.25
    return _flat(n, 0, rows, finals, props=synth.ACCEPTOR | synth.I_LABEL_SORTED | synth.O_LABEL_SORTED)


def sparse_lone(n, e):
    """n states of which only the first e + 1 are connected (a chain); the others are isolated"""
    rows = [[(1 + s % 4, 1 + s % 4, (s % 5) / 4.0, s + 1)] if s < e else [] for s in range(n)]
    finals = np.full(n, np.inf, dtype=np.float32)
    finals[e] = 1.0
    return _flat(n, 0, rows, finals)


def one_state(final=0.75):
    return _flat(1, 0, [[]], [final])


def three_paths():
    """acyclic, exactly three complete paths: 0 -> 1 -> 3, 0 -> 2 -> 3, 0 -> 3"""
    rows = [[(1, 1, 1.0, 1), (2, 2, 0.5, 2), (3, 3, 4.0, 3)], [(4, 4, 1.0, 3)], [(5, 5, 1.25, 3)], []]
    return _flat(4, 0, rows, [np.inf, np.inf, np.inf, 0.0])


def inf_third_path():
    """three_paths with +inf on the direct arc: the third of three paths runs through it"""
    f = three_paths()
    f["arcs"]["weight"][2] = np.inf
    return f


def all_final(rng, n=300):
    """every state final: as many super-initial arcs in the reversed search as states"""
    f = ring_with_chords(rng, n, 2 * n, 4)
    f["finals"] = (rng.integers(0, 12, n) / 4).astype(np.float32)
    return f


def start_final_self_loop(rng):
    """the start state is itself final and has a self loop"""
    f = ring_with_chords(rng, 40, 90, 4)
    rows = _rows(f)
    rows[0].append((7, 7, 0.25, 0))
    f2 = _flat(40, 0, rows, f["finals"])
    f2["finals"][0] = 0.5
    return f2


def _rows(flat):
    off = flat["offsets"]
    return [[(int(a["ilabel"]), int(a["olabel"]), float(a["weight"]), int(a["nextstate"])) for a in flat["arcs"][off[s]:off[s + 1]]]
            for s in range(flat["n_states"])]


def with_edge_weights(flat, seed):
    """the same states and arcs with: -0.0 on some arcs (every zero weight and a few more); +inf on a few arcs off the
    routes and on EVERY arc into one final state (the only routes to it); negative final weights, the farthest final state
    given the one that makes it the best; a final weight on the start state.  No arc weight is < 0 (-0.0 < 0 is false), so
    both kernels take the item."""
    rng = np.random.default_rng(seed)
    f = dict(flat, arcs=flat["arcs"].copy(), finals=flat["finals"].copy())
    a, n = f["arcs"], f["n_states"]
    fin = [int(s) for s in np.flatnonzero(np.isfinite(f["finals"])) if s != f["start"]]
    cut = fin[0]
    a["weight"][a["nextstate"] == cut] = np.inf  # on the only routes to a final state
    off_route = rng.choice(len(a), max(2, len(a) // 40), replace=False)
    a["weight"][off_route[a["nextstate"][off_route] != (f["start"] + 1) % n]] = np.inf
    zero = np.flatnonzero(a["weight"] == 0)
    a["weight"][zero] = -0.0
    more = rng.choice(np.flatnonzero(np.isfinite(a["weight"])), 5, replace=False)
    a["weight"][more] = -0.0
    d = forward_distances(f)
    reach = [s for s in fin if d[s] < INF]
    assert len(reach) >= 3, "edge weights: too few final states left"
    far = max(reach, key=lambda s: d[s])
    for s in fin:
        f["finals"][s] = -0.25 * (1 + s % 3)
    f["finals"][far] = -d[far] - 4.0  # d + rho = -4 at the farthest final state, >= -0.75 at every other
    f["finals"][f["start"]] = 1.0
    return f


# ================================================================ the routing rules, restated
def sp1_staged(n, arcs):
    return n <= SP1_STAGE_STATES and arcs <= SP1_STAGE_ARCS


def _n1(items):
    """the counters of one launch of the n = 1 kernel over `items` (none is handed back: without negative arc weights the
    relaxation settles within n rounds, and the guard sits at n + 1)"""
    return dict(n1_in_kernel=len(items), n1_handed_back=0,
                n1_staged=sum(1 for f in items if f["n_states"] and has_start(f) and sp1_staged(f["n_states"], n_arcs(f))))


ZERO_N1 = dict(n1_in_kernel=0, n1_staged=0, n1_handed_back=0)


def predict_n1_lone(f):
    """a lone shortest_path: at most 4096 states and 2048 arcs, no negative arc weight"""
    return _n1([f]) if f["n_states"] <= SP1_MAX_STATES and n_arcs(f) <= SP1_LONE_ARCS and not has_negative(f) else dict(ZERO_N1)


def predict_n1_batch(flats):
    """shortest_path_batch(nshortest = 1): a list of at least two offers every item of at most 4096 states and 16384 arcs
    without negative arc weights (an empty or start-less item too: the kernel answers it at once); a list of one is a lone
    call"""
    if len(flats) < 2:
        return predict_n1_lone(flats[0]) if flats else dict(ZERO_N1)
    return _n1([f for f in flats if f["n_states"] <= SP1_MAX_STATES and n_arcs(f) <= SP1_MAX_ARCS and not has_negative(f)])


def predict_export(flats):
    """shortest_path_batch(nshortest > 1, unique): the kernel exports the distances of every item with a start state, at most
    4096 states and 16384 arcs and no negative arc weight, when the list has at least two"""
    if len(flats) < 2:
        return dict(ZERO_N1)
    return _n1([f for f in flats if has_start(f) and 0 < f["n_states"] <= SP1_MAX_STATES and n_arcs(f) <= SP1_MAX_ARCS
                and not has_negative(f)])


# ================================================================ the input lists (built once)
SIZE_CASES = {"2048x4096": (2048, 4096), "2049x4096": (2049, 4096), "2048x4097": (2048, 4097), "4096x16384": (4096, 16384),
              "4097x8192": (4097, 8192), "4096x16385": (4096, 16385)}
# (in the kernel, staged) of the size item in a batch of two
SIZE_EXPECT = {"2048x4096": (1, 1), "2049x4096": (1, 0), "2048x4097": (1, 0), "4096x16384": (1, 0), "4097x8192": (0, 0),
               "4096x16385": (0, 0)}


@functools.lru_cache(maxsize=None)
def size_item(case, grid):
    n, e = SIZE_CASES[case]
    return ring_with_chords(np.random.default_rng(1000 + n + e + grid), n, e, grid)


@functools.lru_cache(maxsize=None)
def small_item(seed=7, n=24, e=60, grid=4):
    return ring_with_chords(np.random.default_rng(seed), n, e, grid)


@functools.lru_cache(maxsize=None)
def chain_item(n):
    return reversed_chain(n)


@functools.lru_cache(maxsize=None)
def mixed_batch():
    startless = dict(small_item(11), start=None)
    return [one_state(), empty_flat(), small_item(8), size_item("4096x16384", 512), startless, one_state(np.inf),
            size_item("2048x4096", 4), small_item(9, 60, 150, 512), one_state(2.0)]


@functools.lru_cache(maxsize=None)
def edge_items():
    """(60 states, the smallest unstaged size) with every edge weight"""
    return [with_edge_weights(ring_with_chords(np.random.default_rng(61), 60, 170, 4), 1),
            with_edge_weights(size_item("2049x4096", 4), 2)]


@functools.lru_cache(maxsize=None)
def edge_dags():
    """small acyclic items with -0.0 arc weights, negative final weights and a final start state, every weight finite: the
    brute force can enumerate them"""
    from helpers import random_fst_flat
    rng = np.random.default_rng(77)
    out = []
    for k in range(6):
        f = random_fst_flat(rng, int(rng.integers(5, 12)), 3, 4, p_final=0.4, min_fanout=1, acyclic=True, weight_grid=4, max_w=12)
        f["arcs"]["weight"][f["arcs"]["weight"] == 0] = -0.0
        f["arcs"]["weight"][::5] = -0.0
        fin = np.isfinite(f["finals"])
        f["finals"][fin] = -f["finals"][fin] - np.float32(0.25)
        f["finals"][0] = 1.0
        f["finals"][-1] = -2.5
        out.append(f)
    return out


@functools.lru_cache(maxsize=None)
def edge_nbest_list():
    return edge_items() + edge_dags() + [inf_third_path()]


@functools.lru_cache(maxsize=None)
def nbest_limit_lists():
    """name -> (list, nshortest values)"""
    fit = ring_with_chords(np.random.default_rng(4096), 4096, 8192, 512)
    return {"4096x8192": ([fit, small_item()], (2, 10, 64)),
            "4097x8192": ([ring_with_chords(np.random.default_rng(4097), 4097, 8192, 512), small_item()], (2,)),
            "4096x8193": ([ring_with_chords(np.random.default_rng(8193), 4096, 8193, 512), small_item()], (2,)),
            "65 paths": ([small_item(), small_item(8), three_paths()], (65,))}


@functools.lru_cache(maxsize=None)
def capacity_lists():
    """(list, nshortest, the T the formula gives)"""
    return [([small_item(), small_item(8)], 2, 2048),
            ([ring_with_chords(np.random.default_rng(100), 100, 240, 512), small_item()], 20, 4320),
            ([chain_item(4096), small_item()], 64, 16384)]


@functools.lru_cache(maxsize=None)
def overflow_list():
    """complete(20) between fitting items: T follows the largest item, 24 states"""
    return [small_item(), complete(20, 1), three_paths(), complete(20, 2), small_item(8)]


@functools.lru_cache(maxsize=None)
def dense_fit_list():
    """complete(12) in a batch of its own kind: T = 2 * 64 * (12 + 8) = 2560"""
    return [complete(12, 2), three_paths()]


@functools.lru_cache(maxsize=None)
def guard_list():
    return [chain_item(4096), three_paths()]


@functools.lru_cache(maxsize=None)
def finals_list():
    rng = np.random.default_rng(300)
    return [all_final(rng), start_final_self_loop(rng), small_item()]


UNIQUE_CASES = {"16384 arcs": (4096, 4, 4), "16385 arcs": (4096, 4, 5), "4097 states": (4097, 3, 0)}


@functools.lru_cache(maxsize=None)
def unique_list(case):
    n, labels, extra = UNIQUE_CASES[case]
    return [parallel_chain(n, labels, extra), parallel_chain(30, 3)]


# ---- the oracle's answers, computed once per (item, question) and left unchanged
_REF = {}


def ref(oracle, flat, n=1, unique=False):
    key = (id(flat), n, unique)
    if key not in _REF:
        o = to_oracle(oracle, flat)
        _REF[key] = (flat, (o.shortest_path_canonical() if n == 1 else o.shortest_path_n(n, unique=unique)).to_flat())
    return _REF[key][1]


def same(got, exp, what):
    assert_flat_identical(got, exp, what, check_props=True)


# ================================================================ no GPU
def test_new_symbol_declared_exported_and_bound(wfst_lib):
    import rustfst_amd
    name = "wfst_ctx_get_small_path_stats"
    assert len(COUNTERS) == 7
    header = helpers.check_counter_getter(wfst_lib, name, COUNTERS, rustfst_amd.Context.small_path_stats)
    text = header[header.index("which path answered the small shortest-path queries"):header.index("wfst_status " + name)]
    for limit in ("4096 states", "16384 arcs", "2048 arcs", "2048 states", "4096 arcs", "8192 arcs", "nshortest <= 64",
                  "min(16384, max(2048, 2 * nshortest * (max_n + 8)))"):
        assert limit in text, limit


def test_null_ctx_is_ko(wfst_lib):
    helpers.null_ctx_is_ko(wfst_lib, "wfst_ctx_get_small_path_stats", 7)


def test_generators_hit_their_counts():
    rng = np.random.default_rng(3)
    for n, e in list(SIZE_CASES.values()) + [(60, 170), (4096, 8192), (4097, 8192), (4096, 8193)]:
        for grid in (4, 512):
            f = ring_with_chords(rng, n, e, grid)
            assert (f["n_states"], n_arcs(f), int(f["offsets"][-1])) == (n, e, e) and f["start"] == 0
            assert int(np.isfinite(f["finals"]).sum()) == 8
            w = f["arcs"]["weight"].astype(np.float64) * grid
            assert np.array_equal(w, np.round(w)) and w.min() >= 0
            off = f["offsets"]
            assert all(((s + 1) % n) in f["arcs"]["nextstate"][off[s]:off[s + 1]] for s in range(0, n, 97))
            il_sorted = all(np.all(np.diff(f["arcs"]["ilabel"][off[s]:off[s + 1]].astype(np.int64)) >= 0) for s in range(n))
            assert il_sorted and f["props"] & synth.I_LABEL_SORTED
            ol_sorted = all(np.all(np.diff(f["arcs"]["olabel"][off[s]:off[s + 1]].astype(np.int64)) >= 0) for s in range(n))
            assert bool(f["props"] & synth.O_LABEL_SORTED) == ol_sorted and bool(f["props"] & NOT_O_LABEL_SORTED) != ol_sorted
    for n in (2048, 4096):
        f = reversed_chain(n)
        assert (f["n_states"], n_arcs(f), f["start"]) == (n, n - 1, n - 1) and np.isfinite(f["finals"]).sum() == 1
        assert np.array_equal(f["arcs"]["nextstate"], np.arange(n - 1)) and np.isfinite(f["finals"][0])
    for n in (12, 20):
        f = complete(n, 1)
        assert (f["n_states"], n_arcs(f)) == (n, n * (n - 1)) and np.flatnonzero(np.isfinite(f["finals"])).tolist() == [n - 1]
        pairs = {(s, int(t)) for s in range(n) for t in f["arcs"]["nextstate"][f["offsets"][s]:f["offsets"][s + 1]]}
        assert len(pairs) == n * (n - 1) and set(f["arcs"]["weight"].tolist()) <= set(range(8))
    assert (parallel_chain(4096, 4)["n_states"], n_arcs(parallel_chain(4096, 4))) == (4096, 16380)
    for case, (n, labels, extra) in UNIQUE_CASES.items():
        f = unique_list(case)[0]
        assert f["n_states"] == n and n_arcs(f) == (n - 1) * labels + extra and f["props"] & synth.ACCEPTOR
        assert np.array_equal(f["arcs"]["ilabel"], f["arcs"]["olabel"])
        off = f["offsets"]  # the reversed form is deterministic: the arcs INTO a state have distinct labels
        assert all(len(set(f["arcs"]["ilabel"][off[s]:off[s + 1]].tolist())) == off[s + 1] - off[s] for s in range(0, n, 61))
    assert [n_arcs(unique_list(c)[0]) for c in UNIQUE_CASES] == [16384, 16385, 12288]
    f = sparse_lone(4097, 2000)
    assert (f["n_states"], n_arcs(f)) == (4097, 2000)
    assert len(enumerate_paths(three_paths())) == 3


def test_edge_weight_items_carry_every_edge():
    for f, base in zip(edge_items(), (None, size_item("2049x4096", 4))):
        w, fin, start = f["arcs"]["weight"], f["finals"], f["start"]
        assert not has_negative(f) and np.signbit(w).sum() >= 5 and np.isposinf(w).sum() >= 3
        d = forward_distances(f)
        finals = [s for s in range(f["n_states"]) if fin[s] != np.inf]
        cut = [s for s in finals if s != start and d[s] == INF]
        assert cut and all(np.isposinf(w[f["arcs"]["nextstate"] == s]).all() for s in cut)  # +inf ON the only routes
        assert any(d[int(t)] < INF for t in f["arcs"]["nextstate"][np.isposinf(w)] if int(t) not in cut)  # ... and off them
        reach = [s for s in finals if d[s] < INF]
        best = min(reach, key=lambda s: (d[s] + float(fin[s]), s))
        assert best != min(reach, key=lambda s: d[s]) and fin[best] < 0 and np.isfinite(fin[start]) and best != start
        if base is not None:
            assert (f["n_states"], n_arcs(f)) == (2049, 4096) and not sp1_staged(2049, 4096)
    for f in edge_dags():
        assert np.isfinite(f["arcs"]["weight"]).all() and np.signbit(f["arcs"]["weight"]).any() and not has_negative(f)
        assert (f["finals"][np.isfinite(f["finals"])] < 0).any() and np.isfinite(f["finals"][0])


def test_routing_restatement_and_predicted_counters():
    """the rules on both sides of every limit, and the counters they predict for every list of the GPU tests"""
    assert sp1_staged(2048, 4096) and not sp1_staged(2049, 4096) and not sp1_staged(2048, 4097)
    assert [tree_capacity(*a) for a in ((2, 24), (20, 100), (64, 4096), (32, 24), (64, 24), (64, 12), (3, 4096))] == \
        [2048, 4320, 16384, 2048, 4096, 2560, 16384]
    assert has_negative(dict(arcs=np.array([(1, 1, -0.5, 0)], dtype=TR_DTYPE)))
    assert not has_negative(dict(arcs=np.array([(1, 1, -0.0, 0), (1, 1, np.inf, 0)], dtype=TR_DTYPE)))
    for case, (in_kernel, staged) in SIZE_EXPECT.items():
        for grid in (4, 512):
            got = predict_n1_batch([size_item(case, grid), small_item()])
            assert got == dict(n1_in_kernel=1 + in_kernel, n1_staged=1 + staged, n1_handed_back=0), case
    assert predict_n1_batch([chain_item(2048), small_item()]) == dict(n1_in_kernel=2, n1_staged=2, n1_handed_back=0)
    assert predict_n1_batch([chain_item(4096), small_item()]) == dict(n1_in_kernel=2, n1_staged=1, n1_handed_back=0)
    # the mixed batch: all nine offered; the empty and the start-less item are answered before anything is staged, and the
    # 4096-state item is not staged
    assert predict_n1_batch(mixed_batch()) == dict(n1_in_kernel=9, n1_staged=6, n1_handed_back=0)
    assert predict_n1_lone(ring_with_chords(np.random.default_rng(1), 700, 2048, 4))["n1_in_kernel"] == 1
    assert predict_n1_lone(ring_with_chords(np.random.default_rng(1), 700, 2049, 4)) == ZERO_N1
    assert predict_n1_lone(sparse_lone(4097, 2000)) == ZERO_N1 and predict_n1_lone(sparse_lone(4096, 2000))["n1_in_kernel"] == 1
    assert predict_n1_batch([size_item("2048x4096", 4)]) == ZERO_N1  # a list of one is a lone call: 4096 arcs > 2048
    assert predict_n1_batch([small_item()]) == dict(n1_in_kernel=1, n1_staged=1, n1_handed_back=0)
    assert predict_n1_batch(edge_items()) == dict(n1_in_kernel=2, n1_staged=1, n1_handed_back=0)
    neg = dict(small_item(), arcs=small_item()["arcs"].copy())
    neg["arcs"]["weight"][3] = -1.0
    assert predict_n1_batch([neg, small_item()])["n1_in_kernel"] == 1 and nbest_offered([neg, small_item()], 2) == [small_item()]
    want = {"16384 arcs": dict(n1_in_kernel=2, n1_staged=1, n1_handed_back=0), "16385 arcs": dict(n1_in_kernel=1, n1_staged=1, n1_handed_back=0),
            "4097 states": dict(n1_in_kernel=1, n1_staged=1, n1_handed_back=0)}
    for case in UNIQUE_CASES:
        assert predict_export(unique_list(case)) == want[case], case
    assert predict_export([parallel_chain(30, 3)]) == ZERO_N1
    for name, (flats, ns) in nbest_limit_lists().items():
        for n in ns:
            p = predict_nbest(flats, n)
            exp = {"4096x8192": (2, 16384), "4097x8192": (1, 2048), "4096x8193": (1, 2048), "65 paths": (0, 0)}[name]
            assert (p["nbest_in_kernel"], p["nbest_tree_capacity"], p["nbest_tree_full"]) == (exp[0], exp[1], 0), (name, n)
    for flats, n, T in capacity_lists():
        p = predict_nbest(flats, n)
        assert p == dict(nbest_in_kernel=2, nbest_tree_full=0, nbest_out_full=0, nbest_tree_capacity=T)
    assert predict_nbest(guard_list(), 3)["nbest_in_kernel"] == 2 and predict_nbest(guard_list(), 64)["nbest_in_kernel"] == 2
    for n in (2, 10):
        assert predict_nbest(finals_list(), n)["nbest_in_kernel"] == 3
        assert predict_nbest(edge_nbest_list(), n)["nbest_in_kernel"] == len(edge_nbest_list()) == 9


def test_search_restatement_counts_tree_entries():
    """known counts on inputs small enough to trace by hand, and the margins of the overflow / fits inputs"""
    # three_paths, n = 64: the super-initial arc (1), the three arcs into state 3, the arcs into 1 and 2 from 0 (2), and a
    # completed path at each of the three arrivals in state 0: 2 + 1 + 3 + 2 + 3
    assert nbest_tree_entries(three_paths(), 64) == 11
    # a chain has one path: its n - 1 arcs, the super-initial arc and the completed path
    assert nbest_tree_entries(chain_item(2048), 3) == 2 + 2048 + 1
    assert nbest_tree_entries(dict(small_item(), finals=np.full(24, np.inf, np.float32)), 5) == 0
    for seed in (1, 2):
        for n, T in ((32, 2048), (64, 4096)):
            assert tree_capacity(n, 24) == T
            e = nbest_tree_entries(complete(20, seed), n, stop_at=1 << 16)
            print("complete(20, %d) n=%d: %d entries, T=%d" % (seed, n, e, T))
            assert e >= 2 * T
    # (weights 0..7 leave zero-weight cycles, so the count moves a lot with the seed: 1508 entries at seed 2, 3598 at seed 1)
    e = nbest_tree_entries(complete(12, 2), 64)
    print("complete(12, 2) n=64: %d entries, T=%d" % (e, tree_capacity(64, 12)))
    assert e <= 0.8 * tree_capacity(64, 12)
    for n in (32, 64):
        p = predict_nbest(overflow_list(), n)
        assert (p["nbest_in_kernel"], p["nbest_tree_full"], p["nbest_tree_capacity"]) == (3, 2, tree_capacity(n, 24))
    p = predict_nbest(dense_fit_list(), 64)
    assert (p["nbest_in_kernel"], p["nbest_tree_full"], p["nbest_tree_capacity"]) == (2, 0, 2560)


def test_oracle_answers_are_cached_and_quick(oracle):
    """every reference the GPU tests use, computed here once (they share the cache); the unique chain is the one whose
    time was unknown"""
    import time
    t0 = time.perf_counter()
    for case in UNIQUE_CASES:
        for f in unique_list(case):
            ref(oracle, f, 4, unique=True)
    t_unique = time.perf_counter() - t0
    print("oracle: unique n-best of the parallel chains %.2f s" % t_unique)
    a = ref(oracle, chain_item(4096))
    assert a["n_states"] == 4096 and len(a["arcs"]) == 4095 and ref(oracle, chain_item(4096)) is a
    b = ref(oracle, chain_item(4096), 3)
    # one path although three were asked for: ONE arc leaves the start state; the path holds the 4096 states' images, the
    # start state, the completed-path state and the final state
    assert b["start"] == 0 and int(b["offsets"][1]) == 1 and (b["n_states"], len(b["arcs"])) == (4099, 4098)
    assert len(enumerate_paths(ref(oracle, three_paths(), 64))) == 3
    c = ref(oracle, inf_third_path(), 10)  # the oracle returns the path through the +inf arc, as the third of three
    assert int(c["offsets"][1]) == 3 and np.isposinf(c["arcs"]["weight"]).sum() == 1


# ================================================================ GPU
def _counters(ctx, keys):
    st = ctx.small_path_stats()
    assert tuple(st) == COUNTERS
    return {k: st[k] for k in keys}


def run_n1(ctx, oracle, flats, monkeypatch, what, expect=None, canonical=True):
    """one batch through the kernel and one through the general path on the same handles; every result against the oracle
    (where `canonical`) and the two against each other; the counters against the prediction.  Returns the results."""
    import rustfst_amd
    cfg = rustfst_amd.ShortestPathConfig(nshortest=1)
    devs = [to_device(f, ctx) for f in flats]
    monkeypatch.delenv("WFST_SP1_DEVICE", raising=False)
    got = [o.to_flat() for o in rustfst_amd.shortest_path_batch(devs, cfg, ctx)]
    st = _counters(ctx, ZERO_N1)
    print("%s: %s" % (what, st))
    monkeypatch.setenv("WFST_SP1_DEVICE", "0")
    general = [o.to_flat() for o in rustfst_amd.shortest_path_batch(devs, cfg, ctx)]
    assert _counters(ctx, ZERO_N1) == ZERO_N1, "the general path launched the kernel"
    monkeypatch.delenv("WFST_SP1_DEVICE")
    for k, (f, g, h) in enumerate(zip(flats, got, general)):
        same(g, h, "%s item %d vs the general path" % (what, k))
        if canonical:
            same(g, ref(oracle, f), "%s item %d vs the oracle" % (what, k))
    assert st == (predict_n1_batch(flats) if expect is None else expect), what
    return got


def run_nbest(ctx, oracle, flats, n, monkeypatch, what, brute=()):
    import rustfst_amd
    cfg = rustfst_amd.ShortestPathConfig(nshortest=n)
    devs = [to_device(f, ctx) for f in flats]
    monkeypatch.delenv("WFST_NBEST_DEVICE", raising=False)
    monkeypatch.delenv("WFST_NBEST_TREE", raising=False)
    got = [o.to_flat() for o in rustfst_amd.shortest_path_batch(devs, cfg, ctx)]
    keys = COUNTERS[3:]
    st = _counters(ctx, keys)
    print("%s n=%d: %s" % (what, n, st))
    assert int(ctx.stats()["nbest_device_problems"]) == st["nbest_in_kernel"]
    monkeypatch.setenv("WFST_NBEST_DEVICE", "0")
    general = [o.to_flat() for o in rustfst_amd.shortest_path_batch(devs, cfg, ctx)]
    assert _counters(ctx, keys) == dict.fromkeys(keys, 0), "the host search launched the kernel"
    monkeypatch.delenv("WFST_NBEST_DEVICE")
    for k, (f, g, h) in enumerate(zip(flats, got, general)):
        same(g, h, "%s n=%d item %d vs the host search" % (what, n, k))
        same(g, ref(oracle, f, n), "%s n=%d item %d vs the oracle" % (what, n, k))
        if k in brute:
            check_nbest_against_brute_force(g, f, n, "%s n=%d item %d" % (what, n, k))
    assert st == predict_nbest(flats, n), what
    return got, st


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [4, 512])
@pytest.mark.parametrize("case", list(SIZE_CASES))
def test_n1_kernel_at_its_size_limits(gpu_ctx, oracle, monkeypatch, case, grid):
    in_kernel, staged = SIZE_EXPECT[case]
    run_n1(gpu_ctx, oracle, [size_item(case, grid), small_item()], monkeypatch, "%s grid %d" % (case, grid),
           expect=dict(n1_in_kernel=1 + in_kernel, n1_staged=1 + staged, n1_handed_back=0))


@pytest.mark.gpu
@pytest.mark.parametrize("n,staged", [(2048, 2), (4096, 1)])
def test_n1_reversed_chain_converges_within_the_guard(gpu_ctx, oracle, monkeypatch, n, staged):
    """n - 1 improving rounds and a quiet one: a guard two rounds early would hand the item back.  The path takes all n - 1
    arcs, and the payload slice of the item has room for exactly n."""
    got = run_n1(gpu_ctx, oracle, [chain_item(n), small_item()], monkeypatch, "reversed chain %d" % n,
                 expect=dict(n1_in_kernel=2, n1_staged=staged, n1_handed_back=0))
    assert got[0]["n_states"] == n and len(got[0]["arcs"]) == n - 1


@pytest.mark.gpu
def test_n1_mixed_batch_lays_every_item_out_by_its_own_size(gpu_ctx, oracle, monkeypatch):
    """the launch's LDS follows the largest item (4096 states, unstaged); one-state, empty, start-less and staged items
    beside it"""
    got = run_n1(gpu_ctx, oracle, mixed_batch(), monkeypatch, "mixed batch",
                 expect=dict(n1_in_kernel=9, n1_staged=6, n1_handed_back=0))
    assert [g["n_states"] for g in got[:2]] == [1, 0] and got[4]["n_states"] == 0 and got[5]["n_states"] == 0


@pytest.mark.gpu
def test_n1_lone_call_limits(gpu_ctx, oracle, monkeypatch):
    """a lone shortest_path: 2048 arcs go to the kernel, 2049 do not, 4097 states (2000 arcs, most states isolated) do not;
    a batch of one item is a lone call too: 4096 arcs are not offered (n < 2), 60 arcs are taken by the lone route"""
    import rustfst_amd
    rng = np.random.default_rng(2048)
    cases = [(ring_with_chords(rng, 700, 2048, 4), 1), (ring_with_chords(rng, 700, 2049, 4), 0), (sparse_lone(4097, 2000), 0),
             (sparse_lone(4096, 2000), 1)]
    for k, (f, want) in enumerate(cases):
        d = to_device(f, gpu_ctx)
        monkeypatch.delenv("WFST_SP1_DEVICE", raising=False)
        got = d.shortest_path().to_flat()
        st = _counters(gpu_ctx, ZERO_N1)
        assert st == predict_n1_lone(f) and st["n1_in_kernel"] == want, (k, st)
        monkeypatch.setenv("WFST_SP1_DEVICE", "0")
        same(got, d.shortest_path().to_flat(), "lone call %d vs the general path" % k)
        assert _counters(gpu_ctx, ZERO_N1) == ZERO_N1
        monkeypatch.delenv("WFST_SP1_DEVICE")
        same(got, ref(oracle, f), "lone call %d vs the oracle" % k)
    cfg = rustfst_amd.ShortestPathConfig(nshortest=1)
    for f, want in ((size_item("2048x4096", 4), 0), (small_item(), 1)):
        out = rustfst_amd.shortest_path_batch([to_device(f, gpu_ctx)], cfg, gpu_ctx)
        st = _counters(gpu_ctx, ZERO_N1)
        assert st == predict_n1_batch([f]) and st["n1_in_kernel"] == want
        same(out[0].to_flat(), ref(oracle, f), "a batch of one")


@pytest.mark.gpu
def test_n1_edge_weights(gpu_ctx, oracle, monkeypatch):
    """-0.0 and +inf arc weights, negative final weights that make the farthest final state the best, a final start state:
    has_negative reads none of them, so the kernel takes both items (one staged, one not).  The canonical oracle takes
    these inputs: its distances do not depend on the final weights, and it adds them as the kernel does."""
    got = run_n1(gpu_ctx, oracle, edge_items(), monkeypatch, "edge weights",
                 expect=dict(n1_in_kernel=2, n1_staged=1, n1_handed_back=0))
    for f, g in zip(edge_items(), got):
        assert g["n_states"] > 2 and g["finals"][np.isfinite(g["finals"])][0] < 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["4096x8192", "4097x8192", "4096x8193", "65 paths"])
def test_nbest_kernel_at_its_size_limits(gpu_ctx, oracle, monkeypatch, name):
    """4096 states and 8192 arcs are in the kernel at n = 2, 10 and 64 (64: every lane of the connect phase has a path);
    one state or one arc more is not; 65 paths send every item to the host search"""
    flats, ns = nbest_limit_lists()[name]
    for n in ns:
        _, st = run_nbest(gpu_ctx, oracle, flats, n, monkeypatch, name)
        want = {"4096x8192": 2, "4097x8192": 1, "4096x8193": 1, "65 paths": 0}[name]
        assert st["nbest_in_kernel"] == want and st["nbest_tree_full"] == 0


@pytest.mark.gpu
def test_nbest_tree_capacity_follows_the_formula(gpu_ctx, oracle, monkeypatch):
    for flats, n, T in capacity_lists():
        _, st = run_nbest(gpu_ctx, oracle, flats, n, monkeypatch, "capacity %d" % T)
        assert st["nbest_tree_capacity"] == T and st["nbest_in_kernel"] == 2


@pytest.mark.gpu
@pytest.mark.parametrize("n", [32, 64])
def test_nbest_natural_overflow_between_fitting_items(gpu_ctx, oracle, monkeypatch, n):
    """no WFST_NBEST_TREE: complete(20) outgrows the T its own batch gives it and comes back, the fitting items around it
    stay in position with their payloads intact"""
    _, st = run_nbest(gpu_ctx, oracle, overflow_list(), n, monkeypatch, "overflow")
    assert st["nbest_tree_full"] == 2 and st["nbest_in_kernel"] == 3 and st["nbest_tree_capacity"] == tree_capacity(n, 24)


@pytest.mark.gpu
def test_nbest_dense_item_that_fits(gpu_ctx, oracle, monkeypatch):
    _, st = run_nbest(gpu_ctx, oracle, dense_fit_list(), 64, monkeypatch, "complete(12)")
    assert st["nbest_tree_full"] == 0 and st["nbest_in_kernel"] == 2 and st["nbest_tree_capacity"] == 2560


@pytest.mark.gpu
def test_nbest_guard_and_path_count(gpu_ctx, oracle, monkeypatch):
    """reversed_chain(4096) needs 4095 improving rounds and a quiet one and holds ONE path although three are asked for; an
    acyclic item with exactly three paths is asked for 64"""
    got, st = run_nbest(gpu_ctx, oracle, guard_list(), 3, monkeypatch, "guard")
    assert st["nbest_in_kernel"] == 2 and int(got[0]["offsets"][1]) == 1 and (got[0]["n_states"], len(got[0]["arcs"])) == (4099, 4098)
    got, st = run_nbest(gpu_ctx, oracle, guard_list(), 64, monkeypatch, "guard", brute=(1,))
    assert st["nbest_in_kernel"] == 2 and len(enumerate_paths(got[1])) == 3


@pytest.mark.gpu
def test_nbest_finals_and_start(gpu_ctx, oracle, monkeypatch):
    """all 300 states final (300 super-initial arcs); the start state final and with a self loop"""
    for n in (2, 10):
        _, st = run_nbest(gpu_ctx, oracle, finals_list(), n, monkeypatch, "finals")
        assert st["nbest_in_kernel"] == 3


@pytest.mark.gpu
def test_nbest_edge_weights(gpu_ctx, oracle, monkeypatch):
    """the edge weights of the n = 1 test through the n-best kernel; the small acyclic items (every weight finite) also
    against the exhaustive enumeration"""
    flats = edge_nbest_list()
    for n in (2, 10):
        got, st = run_nbest(gpu_ctx, oracle, flats, n, monkeypatch, "edge weights", brute=range(2, len(flats) - 1))
        assert st["nbest_in_kernel"] == len(flats)
    assert int(got[-1]["offsets"][1]) == 3 and np.isposinf(got[-1]["arcs"]["weight"]).sum() == 1


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(UNIQUE_CASES))
def test_unique_batch_export_limits(gpu_ctx, oracle, case):
    """unique = true: the n = 1 kernel exports distances and arrays.  4096 states with exactly 16384 arcs are exported
    (unstaged); 16385 arcs or 4097 states are not.  The inputs' reversed forms are deterministic."""
    import rustfst_amd
    flats = unique_list(case)
    cfg = rustfst_amd.ShortestPathConfig(nshortest=4, unique=True)
    devs = [to_device(f, gpu_ctx) for f in flats]
    outs = rustfst_amd.shortest_path_batch(devs, cfg, gpu_ctx)
    st = _counters(gpu_ctx, ZERO_N1)
    print("unique %s: %s" % (case, st))
    for k, (f, d, o) in enumerate(zip(flats, devs, outs)):
        same(o.to_flat(), ref(oracle, f, 4, unique=True), "unique %s item %d vs the oracle" % (case, k))
        same(o.to_flat(), d.shortest_path(cfg).to_flat(), "unique %s item %d vs the single call" % (case, k))
    assert st == predict_export(flats) and st["n1_in_kernel"] == (2 if case == "16384 arcs" else 1)
