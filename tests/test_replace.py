"""replace (wfst_replace, wfst_ctx_get_replace_stats): the C-ABI surface without a GPU, the literal restatement of
tests/replace_ref.py checked against the hand-traced K20 known answers and against an independent substitution of path sets,
the divergence criterion on the restatement, and on the device bit-exact parity with the restatement: states, arc order,
labels, weights by bit pattern, finals, start state and property word, at every limit of the search's driver and of the
call-stack table."""
import collections
import copy
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from oracle import model
from oracle.model import ALL, I_LABEL_SORTED, O_LABEL_SORTED, fst_to_flat
import helpers
from helpers import ROOT, assert_flat_identical, dev, enumerate_paths, golden_fst, make_fst
from replace_ref import Diverged, ReplaceError, replace_ref

GOLDEN = os.path.join(ROOT, "tests", "golden", "k20_replace.json")
NEW_SYMBOLS = ("wfst_replace", "wfst_ctx_get_replace_stats")
COUNTERS = ("levels", "states", "arcs", "prefixes", "max_depth", "call_arcs", "dropped_calls", "return_arcs", "arena_grows",
            "prefix_reruns", "level_launches")
MSG_CYCLIC = "replace: cyclic dependency between the FSTs: the reference does not terminate on this input"
MSG_ROOT = "ReplaceFstImpl: No FST corresponding to root label {} in the input tuple vector"
KEY0 = 50  # FST i of a random grammar has the label KEY0 + 2 i: the odd labels between are in range and no key


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def probe_dag(n, rng):
    """n states, two arcs from every state but the last into later states, the last state final"""
    rows = [[[int(rng.integers(1, 9)), int(rng.integers(1, 9)), float(rng.integers(0, 16)) / 8, int(rng.integers(s + 1, n))]
             for _ in range(2)] if s + 1 < n else [] for s in range(n)]
    return make_fst(rows, [None] * (n - 1) + [0.25], 0)


def golden_pairs(c, g):
    return [(label, golden_fst(g["machines"][name])) for label, name in c["pairs"]]


# ---------------------------------------------------------------- inputs
def random_grammar(rng, n_fsts, max_states, max_fan, p_call=0.35, p_startless=0.1, min_states=2, max_depth=None):
    """n_fsts acyclic FSTs; FST i calls only FSTs j > i (and, with max_depth, only while i < max_depth: nesting stops
    there), so nothing recurses.  Arcs go to later states, weights are multiples of 1/8; a callee may lack a start state."""
    keys = [KEY0 + 2 * i for i in range(n_fsts)]
    pairs = []
    for i in range(n_fsts):
        n = int(rng.integers(min_states, max_states + 1))
        rows = []
        for s in range(n):
            row = []
            for _ in range(int(rng.integers(1, max_fan + 1)) if s + 1 < n else 0):
                ns = int(rng.integers(s + 1, n))
                w = float(rng.integers(0, 16)) / 8
                may_call = i + 1 < n_fsts and (max_depth is None or i < max_depth)
                if may_call and rng.random() < p_call:
                    row.append([int(rng.integers(0, 10)), keys[int(rng.integers(i + 1, n_fsts))], w, ns])
                else:
                    ol = int(rng.choice([0, 1, 2, 3, KEY0 - 1, KEY0 + 1, KEY0 + 2 * n_fsts]))  # below, between, above the keys
                    row.append([int(rng.integers(0, 10)), ol, w, ns])
            rows.append(row)
        finals = [float(rng.integers(0, 8)) / 8 if s + 1 == n or rng.random() < 0.3 else None for s in range(n)]
        start = None if i > 0 and rng.random() < p_startless else 0
        pairs.append((keys[i], make_fst(rows, finals, start)))
    return pairs


def with_words(pairs, mode):
    """stored words: the full content word, the label-sorted pair of it only, or 0"""
    out = []
    for label, f in pairs:
        w = model.content_word(f) if f["start"] is not None else 0
        f = dict(copy.deepcopy(f), props={"content": w, "sorted_bits": w & (I_LABEL_SORTED | O_LABEL_SORTED), "zero": 0}[mode] & ALL)
        out.append((label, f))
    return out


def word_fst(length, seed):
    """a linear acceptor of `length` arcs, final at its end"""
    rows = [[[1 + (seed + s) % 9, 1 + (seed + s) % 9, ((seed + s) % 8) / 8, s + 1]] for s in range(length)] + [[]]
    return make_fst(rows, [None] * length + [(seed % 4) / 4], 0)


def fan_grammar(n_calls, n_words, lengths):
    """a root whose start state has n_calls call arcs with pairwise different nextstates, cycling through n_words word FSTs"""
    keys = [100 + k for k in range(n_words)]
    root = make_fst([[[1 + s % 7, keys[s % n_words], (s % 8) / 8, 1 + s] for s in range(n_calls)]] + [[] for _ in range(n_calls)],
                       [None] + [0.25] * n_calls, 0)
    return [(99, root)] + [(keys[k], word_fst(lengths[k % len(lengths)], k)) for k in range(n_words)]


def chain_grammar(n_calls, n_words):
    """a root chain of n_calls call arcs, arc s calling word s % n_words, whose length is 1 + (s % n_words) % 4"""
    keys = [100 + k for k in range(n_words)]
    root = make_fst([[[1, keys[s % n_words], (s % 8) / 8, s + 1]] for s in range(n_calls)] + [[]], [None] * n_calls + [0.5], 0)
    return [(99, root)] + [(keys[k], word_fst(1 + k % 4, k)) for k in range(n_words)]


A_SELF = 99  # S -> a S b | epsilon
S_RECURSIVE = make_fst([[[1, 1, 0.0, 1]], [[5, A_SELF, 0.0, 2]], [[2, 2, 0.0, 3]], []], [0.0, None, None, 0.0], 0)
# the same arcs, but the calling state is one the start cannot reach
S_UNREACHABLE = make_fst([[[1, 1, 0.0, 2]], [[5, A_SELF, 0.0, 2]], [[2, 2, 0.0, 3]], []], [0.0, None, None, 0.0], 0)


def mutual(broken):
    """a root calling A, A -> B, B -> A; broken: B has no start state, so the expansion never gets round"""
    r = make_fst([[[1, 100, 0.0, 1]], []], [None, 0.0], 0)
    a = make_fst([[[2, 101, 0.0, 1], [3, 3, 0.0, 1]], []], [None, 0.0], 0)
    b = make_fst([[[4, 100, 0.0, 1], [5, 5, 0.0, 1]], []], [None, 0.0], None if broken else 0)
    return [(99, r), (100, a), (101, b)]


# ---------------------------------------------------------------- the independent check: substitution on path sets
def strip(t):
    return tuple(x for x in t if x != 0)


def substituted_paths(pairs, root, eps):
    """the multiset of (input string, output string, weight) of the grammar, by substituting the callee's path set into
    the caller's, directly on path sets (the last entry with a label is the one that is meant)"""
    index = {label: i for i, (label, _) in enumerate(pairs)}
    memo = {}

    def lang(i):
        if i not in memo:
            f = pairs[i][1]

            def tails(s):
                out = [((), (), f["finals"][s])] if f["finals"][s] is not None else []
                for il, ol, w, ns in f["rows"][s]:
                    if ol != 0 and ol in index:
                        heads = [((() if eps else strip((il,))) + a, b, w + v) for a, b, v in lang(index[ol])]
                    else:
                        heads = [(strip((il,)), strip((ol,)), w)]
                    out += [(a + c, b + d, v + x) for a, b, v in heads for c, d, x in tails(ns)]
                return out
            memo[i] = tails(f["start"]) if f["start"] is not None else []
        return memo[i]
    return collections.Counter((a, b, float(w)) for a, b, w in lang(index[root]))


def result_paths(flat):
    return collections.Counter((strip(il), strip(ol), w) for w, il, ol in enumerate_paths(flat))


# ================================================================ no GPU
def test_symbols_declared_and_bound(wfst_lib):
    from rustfst_amd import _lib
    with open(os.path.join(ROOT, "include", "wfst.h")) as f:
        header = f.read()
    bound = {name for name, _, _ in _lib.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert re.search(r"\bwfst_status\s+" + name + r"\s*\(", header), name
        assert name in bound, name
        assert hasattr(wfst_lib, name), name
    import rustfst_amd
    helpers.check_counter_getter(wfst_lib, "wfst_ctx_get_replace_stats", COUNTERS, rustfst_amd.Context.replace_stats)
    assert re.search(r"typedef\s+struct\s*\{\s*uint32_t\s+label;\s*const\s+wfst_fst\*\s+fst;\s*\}\s*wfst_label_fst_pair;", header)
    m = re.search(r"#define\s+WFST_ABI_VERSION\s+7\b(.*)", header)
    assert m and all(name in m.group(1).split("; 6:")[0] for name in NEW_SYMBOLS) and wfst_lib.wfst_abi_version() == 7


def test_argument_validation_without_gpu(wfst_lib):
    from rustfst_amd import _lib
    pairs = (_lib.LabelFstPair * 1)()
    out = C.c_void_p(1)
    assert "null" in helpers.ko_message(wfst_lib.wfst_replace(None, 1, pairs, 1, 1, C.byref(out)))
    assert out.value is None
    assert "null" in helpers.ko_message(wfst_lib.wfst_replace(None, 1, None, 0, 0, None))
    assert "null" in helpers.ko_message(wfst_lib.wfst_ctx_get_replace_stats(None, *[None] * 11))
    assert C.sizeof(_lib.LabelFstPair) == 16 and _lib.LabelFstPair.fst.offset == 8


def test_python_surface():
    import rustfst_amd
    assert callable(rustfst_amd.replace) and "replace" in rustfst_amd.__all__
    assert callable(rustfst_amd.Context.replace_stats)
    from rustfst_amd import build
    assert "replace.hip" in build.SOURCES
    with open(os.path.join(ROOT, "include", "wfst.hpp")) as f:
        assert re.search(r"inline VectorFst replace\(const std::vector<std::pair<Label, const VectorFst\*>>& fst_list, Label root,", f.read())


def test_k20_restatement_reproduces_the_derivations():
    """the hand traces of K20_DERIVATION.md, replayed by the restatement (checks the restatement itself)"""
    g = golden()
    assert len(g["cases"]) == 21
    for c in g["cases"]:
        if "error" in c:
            with pytest.raises(ReplaceError, match=re.escape(c["error"])):
                replace_ref(golden_pairs(c, g), c["root"], c["epsilon_on_replace"])
            continue
        info = {}
        got = replace_ref(golden_pairs(c, g), c["root"], c["epsilon_on_replace"], step_cap=100, info=info)
        assert_flat_identical(fst_to_flat(got), fst_to_flat(golden_fst(c["expected"])), c["name"], check_props=True)
        assert info["prefixes"] == c["prefixes"], c["name"]
        assert len(c["expected"]["rows"]) <= 12, c["name"]


def test_restatement_errors():
    one = make_fst([[]], [0.0], 0)
    with pytest.raises(ReplaceError, match=re.escape(MSG_ROOT.format(4))):
        replace_ref([(3, one)], 4, True)
    with pytest.raises(ReplaceError, match=re.escape(MSG_ROOT.format(0))):
        replace_ref([], 0, False)


@pytest.mark.parametrize("eps", (True, False))
def test_restatement_accepts_the_substituted_path_set(eps):
    """random small acyclic grammars: the paths of the restated result are the recursive substitution of the callees' path
    sets into the callers', as multisets of (input string, output string, weight); weights are multiples of 1/8, so every sum
    is exact in float32 and in float64 alike"""
    rng = np.random.default_rng(2001 + eps)
    seen_calls = seen_drops = 0
    for i in range(150):
        pairs = random_grammar(rng, int(rng.integers(2, 6)), 6, 2)
        info = {}
        got = replace_ref(pairs, KEY0, eps, step_cap=100_000, info=info)
        assert result_paths(fst_to_flat(got)) == substituted_paths(pairs, KEY0, eps), i
        seen_calls += info["call_arcs"]
        seen_drops += info["dropped_calls"]
    assert seen_calls > 100 and seen_drops > 5


def test_divergence_criterion_on_the_restatement():
    """a grammar whose expansion reaches a recursive call creates a prefix deeper than the list is long and never ends; one
    whose recursive arc is out of reach never does and ends"""
    for pairs in ([(A_SELF, S_RECURSIVE)], mutual(False)):
        info = {}
        with pytest.raises(Diverged):
            replace_ref(pairs, 99, True, step_cap=500, info=info)
        assert info["max_depth"] > len(pairs)
    for pairs in ([(A_SELF, S_UNREACHABLE)], mutual(True)):
        info = {}
        replace_ref(pairs, 99, True, step_cap=500, info=info)
        assert info["max_depth"] <= len(pairs)


def chain_closed_form(n_calls, n_words):
    """chain_grammar(n_calls, n_words) with n_words | n_calls, epsilon_on_replace: (states, arcs, levels, prefixes).

    Word k has L_k = 1 + k % 4 arcs and L_k + 1 states, and every call site gets a copy of its own (its prefix is the one
    frame (root, s + 1), different for every s): prefixes = n_calls.  The root instance has n_calls + 1 states, copy s has
    L_k + 1 with k = s % n_words, and each word is called n_calls / n_words times:
        states = n_calls + 1 + (n_calls / n_words) * sum_k (L_k + 1).
    The root's arcs are its n_calls call arcs; a copy has its L_k arcs and the one return arc of its last state:
        arcs = n_calls + (n_calls / n_words) * sum_k (L_k + 1).
    Every state has exactly one arc except the last root state, so every level of the search holds one state:
        levels = states."""
    per_round = sum(1 + k % 4 + 1 for k in range(n_words))
    states = n_calls + 1 + (n_calls // n_words) * per_round
    return states, n_calls + (n_calls // n_words) * per_round, states, n_calls


def test_chain_closed_form_on_the_restatement():
    info = {}
    got = replace_ref(chain_grammar(2000, 50), 99, True, info=info)
    states, arcs, levels, prefixes = chain_closed_form(2000, 50)
    assert (states, arcs) == (8921, 8920)
    assert (got["n_states"], sum(len(r) for r in got["rows"]), info["levels"], info["prefixes"]) == (states, arcs, levels, prefixes)


# ================================================================ on the device
def dev_pairs(pairs, ctx):
    return [(label, dev(f, ctx)) for label, f in pairs]


def check(pairs, root, eps, ctx, what, handles=None, exact_counters=True):
    """replace on the device == the restatement, bit for bit, and the counters of the call == the restatement's tallies"""
    import rustfst_amd
    info = {}
    exp = replace_ref(pairs, root, eps, info=info)
    got = rustfst_amd.replace(root, handles or dev_pairs(pairs, ctx), eps).to_flat()
    assert_flat_identical(got, fst_to_flat(exp), what, check_props=True)
    st = ctx.replace_stats()
    if exp["start"] is not None:
        assert (st["states"], st["arcs"], st["levels"]) == (exp["n_states"], sum(len(r) for r in exp["rows"]), info["levels"]), what
        assert (st["prefixes"], st["max_depth"]) == (info["prefixes"], info["max_depth"]), what
        arcs_by_kind = (info["call_arcs"], info["dropped_calls"], info["return_arcs"])
        if exact_counters:
            assert (st["call_arcs"], st["dropped_calls"], st["return_arcs"]) == arcs_by_kind, what
    return st, info


@pytest.mark.gpu
@pytest.mark.parametrize("group", (2, 4, 8, 16, 64))
def test_k20_on_the_device(gpu_ctx, monkeypatch, group):
    import rustfst_amd
    monkeypatch.setenv("WFST_WIDE_GROUP", str(group))
    g = golden()
    for c in g["cases"]:
        pairs = golden_pairs(c, g)
        if "error" in c:
            with pytest.raises(rustfst_amd.WfstError, match=re.escape(c["error"])):
                rustfst_amd.replace(c["root"], dev_pairs(pairs, gpu_ctx), c["epsilon_on_replace"])
            continue
        got = rustfst_amd.replace(c["root"], dev_pairs(pairs, gpu_ctx), c["epsilon_on_replace"]).to_flat()
        assert_flat_identical(got, fst_to_flat(golden_fst(c["expected"])), c["name"], check_props=True)
        if c["expected"]["start"] is not None:
            assert gpu_ctx.replace_stats()["prefixes"] == c["prefixes"], c["name"]


@pytest.mark.gpu
@pytest.mark.parametrize("eps", (True, False))
@pytest.mark.parametrize("words", ("content", "sorted_bits", "zero"))
def test_random_grammars_against_the_restatement(gpu_ctx, eps, words):
    rng = np.random.default_rng(2010 + 2 * ("content", "sorted_bits", "zero").index(words) + eps)
    done = 0
    while done < 10:
        pairs = random_grammar(rng, int(rng.integers(3, 7)), 10, 6, p_call=0.3, min_states=3, max_depth=4)
        try:
            n = replace_ref(pairs, KEY0, eps, step_cap=4000)["n_states"]
        except Diverged:
            continue  # (more than a few thousand states: another draw)
        if n < 150:
            continue
        check(with_words(pairs, words), KEY0, eps, gpu_ctx, f"{words} {eps} {done}")
        done += 1


def wide_input():
    return fan_grammar(150, 10, (8, 9, 10, 11, 12))


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", ({"WFST_WIDE_EST_STATES": "64"}, {"WFST_WIDE_EST_STATES": "64", "WFST_WIDE_NO_FORESIGHT": "1"}),
                         ids=("est_states", "est_states_no_foresight"))
def test_arena_grows_mid_search(gpu_ctx, monkeypatch, knobs):
    pairs = wide_input()
    base, info = check(pairs, 99, True, gpu_ctx, "plain")
    assert base["arena_grows"] == 0 and base["prefix_reruns"] == 0 and 1500 < base["states"] < 2500
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    st, _ = check(pairs, 99, True, gpu_ctx, str(knobs), exact_counters=False)
    assert st["arena_grows"] >= 2 and st["prefixes"] == base["prefixes"] == 150
    # (a level emitted again is tallied again: never less than the true figures)
    assert st["call_arcs"] >= info["call_arcs"] and st["return_arcs"] >= info["return_arcs"]


@pytest.mark.gpu
@pytest.mark.parametrize("batch", (1, 8))
def test_levels_per_look(gpu_ctx, monkeypatch, batch):
    monkeypatch.setenv("WFST_WIDE_BATCH", str(batch))
    st, _ = check(wide_input(), 99, False, gpu_ctx, f"batch {batch}")
    assert st["arena_grows"] == 0


@pytest.mark.gpu
def test_prefix_table_reruns(gpu_ctx, monkeypatch):
    pairs = wide_input()
    monkeypatch.setenv("WFST_REPLACE_PREFIX_SLOTS", "16")  # 150 prefixes: 16, 32, .., 256 slots are too few (half full at most)
    st, _ = check(pairs, 99, True, gpu_ctx, "16 slots")
    assert st["prefix_reruns"] == 5 and st["prefixes"] == 150
    monkeypatch.setenv("WFST_REPLACE_PREFIX_SLOTS", "512")
    st, _ = check(pairs, 99, True, gpu_ctx, "512 slots")
    assert st["prefix_reruns"] == 0
    import rustfst_amd
    monkeypatch.setenv("WFST_REPLACE_PREFIX_SLOTS", "48")
    with pytest.raises(rustfst_amd.WfstError, match="WFST_REPLACE_PREFIX_SLOTS"):
        rustfst_amd.replace(99, dev_pairs(pairs, gpu_ctx), True)


@pytest.mark.gpu
@pytest.mark.parametrize("group", (None, 2, 64))
def test_seventy_arcs_of_one_state(gpu_ctx, monkeypatch, group):
    """more items than any group has lanes; 20 calls with pairwise different nextstates (20 prefixes from one state in one
    level) and 20 that share one nextstate and one nonterminal (one prefix, interned by many lanes at once)"""
    if group:
        monkeypatch.setenv("WFST_WIDE_GROUP", str(group))
    distinct = [[1 + j, 100, (j % 8) / 8, 1 + j] for j in range(20)]
    shared = [[30 + j, 100, (j % 8) / 8, 21] for j in range(20)]
    plain = [[60 + j, 1 + j % 9, (j % 8) / 8, 22 + j % 3] for j in range(30)]
    row = [(distinct, shared, plain)[k].pop(0) for k in np.random.default_rng(2020).permutation([0] * 20 + [1] * 20 + [2] * 30)]
    root = make_fst([row] + [[] for _ in range(24)], [None] + [0.5] * 24, 0)
    st, _ = check([(99, root), (100, word_fst(2, 3))], 99, False, gpu_ctx, "70 arcs")
    assert st["prefixes"] == 21 and st["call_arcs"] == 40


@pytest.mark.gpu
@pytest.mark.parametrize("group", (2, 64))
def test_one_frame_from_two_hundred_states(gpu_ctx, monkeypatch, group):
    """200 states of one level of the root instance, each with a call of one nonterminal into one nextstate: one key of the
    prefix table, interned by the lanes of many waves at once"""
    monkeypatch.setenv("WFST_WIDE_GROUP", str(group))
    rows = [[[1 + s % 9, 1 + s % 9, (s % 8) / 8, 1 + s] for s in range(200)]]
    rows += [[[2, 100, (s % 4) / 4, 201]] for s in range(200)] + [[]]
    root = make_fst(rows, [None] * 201 + [0.0], 0)
    st, _ = check([(99, root), (100, word_fst(3, 1))], 99, True, gpu_ctx, "one frame")
    assert st["prefixes"] == 1 and st["call_arcs"] == 200 and st["states"] == 202 + 4


@pytest.mark.gpu
def test_startless_callee_in_the_middle_of_a_level(gpu_ctx):
    rows = [[[1, 1, 0.0, 1 + s] for s in range(60)]]
    rows += [[[3, 100 if s % 3 else 101, 0.125, 61], [4, 4, 0.0, 61]] for s in range(60)] + [[]]
    root = make_fst(rows, [None] * 61 + [0.0], 0)
    startless = make_fst([[[7, 99, 0.0, 0]]], [0.0], None)
    st, info = check([(99, root), (100, word_fst(2, 0)), (101, startless)], 99, True, gpu_ctx, "startless")
    assert st["dropped_calls"] == info["dropped_calls"] == 20


@pytest.mark.gpu
def test_divergence_is_ko_and_the_context_goes_on(gpu_ctx):
    import rustfst_amd
    probe = probe_dag(40, np.random.default_rng(5))
    fresh = dev(probe, gpu_ctx).shortest_path().to_flat()
    for pairs in ([(A_SELF, S_RECURSIVE)], mutual(False)):
        for eps in (True, False):
            with pytest.raises(rustfst_amd.WfstError, match=re.escape(MSG_CYCLIC)):
                rustfst_amd.replace(99, dev_pairs(pairs, gpu_ctx), eps)
            assert_flat_identical(dev(probe, gpu_ctx).shortest_path().to_flat(), fresh, "shortest_path after the KO")
    for pairs in ([(A_SELF, S_UNREACHABLE)], mutual(True)):
        check(pairs, 99, True, gpu_ctx, "the recursion is out of reach")


@pytest.mark.gpu
def test_chain_with_a_closed_form(gpu_ctx):
    """2 000 call arcs in a chain through 50 words: sizes, levels and prefixes by chain_closed_form's derivation"""
    pairs = chain_grammar(2000, 50)
    import rustfst_amd
    got = rustfst_amd.replace(99, dev_pairs(pairs, gpu_ctx), True)
    st = gpu_ctx.replace_stats()
    states, arcs, levels, prefixes = chain_closed_form(2000, 50)
    assert (st["states"], st["arcs"], st["levels"], st["prefixes"], st["max_depth"]) == (states, arcs, levels, prefixes, 1)
    assert (st["call_arcs"], st["return_arcs"], st["dropped_calls"]) == (2000, 2000, 0)
    flat = got.to_flat()
    row0 = flat["arcs"][flat["offsets"][0]:flat["offsets"][1]]
    assert [tuple(a) for a in row0.tolist()] == [(0, 0, 0.0, 1)]
    assert flat["offsets"][states] == flat["offsets"][states - 1] and flat["finals"][states - 1] == 0.5
    assert_flat_identical(flat, fst_to_flat(replace_ref(pairs, 99, True)), "chain", check_props=True)


def acyclic_weighted_grammar(seed):
    rng = np.random.default_rng(seed)
    while True:
        pairs = random_grammar(rng, 4, 5, 2, p_call=0.4, p_startless=0.0, min_states=3)
        exp = replace_ref(pairs, KEY0, True)
        if 20 < len(enumerate_paths(fst_to_flat(exp))) < 5000:
            return pairs, exp


@pytest.mark.gpu
def test_pipeline_rm_epsilon_shortest_path(gpu_ctx):
    import rustfst_amd
    pairs, exp = acyclic_weighted_grammar(2030)
    handles = dev_pairs(with_words(pairs, "content"), gpu_ctx)
    alone = [h.shortest_path().to_flat() for _, h in handles]
    best = rustfst_amd.replace(KEY0, handles, True).rm_epsilon().shortest_path().to_flat()
    weights = [w for w, _, _ in enumerate_paths(best)]
    assert weights == [min(w for w, _, _ in enumerate_paths(fst_to_flat(exp)))]
    for (_, h), before in zip(handles, alone):
        assert_flat_identical(h.shortest_path().to_flat(), before, "an input after replace")


@pytest.mark.gpu
def test_pipeline_top_sort_optimize(gpu_ctx):
    import rustfst_amd
    pairs, exp = acyclic_weighted_grammar(2031)
    got = rustfst_amd.replace(KEY0, dev_pairs(with_words(pairs, "content"), gpu_ctx), True).top_sort().optimize().to_flat()

    def best_per_string(flat):
        out = {}
        for w, il, ol in enumerate_paths(flat):
            out[(strip(il), strip(ol))] = min(w, out.get((strip(il), strip(ol)), np.inf))
        return out
    assert best_per_string(got) == best_per_string(fst_to_flat(exp))


@pytest.mark.gpu
def test_input_handles_are_left_as_they_are(gpu_ctx):
    """in the manner of test_handle_state.py: fill the caches of the inputs, call replace, observe.  The called entry is that
    file's large input, a transducer of 40 000 states and at least 2^18 arcs — the size from which the second shortest_path
    query of a handle builds its transpose and final list, and the relaxations their region plans and the reversed handle.
    After replace with either value of epsilon_on_replace every input has the same word and arrays and gives, bit for bit,
    the answers it gave before; the result, about the size of the large entry, equals the restatement."""
    import rustfst_amd
    from rustfst_amd import synth
    from replace_ref import INPUT, NEITHER, replace_properties
    t = synth.make_transducer(40000, 8, 64, 0.05, seed=77)
    assert t["offsets"][-1] >= 1 << 18 and int(t["arcs"]["olabel"].max()) < 99  # (nothing in it is a call)
    root = make_fst([[[7, 100, 0.25, 1]], [[3, 3, 0.5, 2]], []], [None, None, 0.125], 0)
    big, small = helpers.to_device(t, gpu_ctx), dev(root, gpu_ctx)
    handles = [(99, small), (100, big)]

    def observe(h):  # (O1 and O3 of test_handle_state.py)
        out = [h.shortest_path().to_flat() for _ in range(3)]
        dist, hops = h.shortest_distance(want_hops=True)
        rdist, ln = h.shortest_distance_with_len(reverse=True)
        return out, [dist.copy(), hops.copy(), rdist.copy()], ln, h.to_flat()

    before = [observe(h) for _, h in handles]
    pairs = [(99, root), (100, model.flat_to_fst(t))]
    exp = fst_to_flat(replace_ref(pairs, 99, True))
    assert exp["n_states"] >= 40000
    for eps in (True, False):
        got = rustfst_amd.replace(99, handles, eps).to_flat()
        if not eps:  # the one call arc keeps its ilabel, and the word is the other option's
            exp["arcs"]["ilabel"][0] = 7
            exp["props"] = replace_properties(99, pairs, INPUT, NEITHER, None) & ALL
        assert_flat_identical(got, exp, f"next to a large input, eps {eps}", check_props=True)
        assert gpu_ctx.replace_stats()["prefixes"] == 1
    for (_, h), (paths, dists, ln, flat) in zip(handles, before):
        after_paths, after_dists, after_ln, after_flat = observe(h)
        assert_flat_identical(after_flat, flat, "an input handle", check_props=True)
        for x, y in zip(after_paths, paths):
            assert_flat_identical(x, y, "shortest_path of an input")
        for x, y in zip(after_dists, dists):
            np.testing.assert_array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32))
        assert after_ln == ln


@pytest.mark.gpu
def test_driver_messages_name_replace(gpu_ctx, monkeypatch):
    """the driver's own KO names the operation that ran it: an arena asked to start beyond what it can index"""
    import rustfst_amd
    g = golden()
    c = g["cases"][0]
    monkeypatch.setenv("WFST_WIDE_EST_STATES", str(3 << 30))
    with pytest.raises(rustfst_amd.WfstError, match="replace: result too large"):
        rustfst_amd.replace(c["root"], dev_pairs(golden_pairs(c, g), gpu_ctx), True)
    # the arena's growths go to replace's counter and leave compose's alone; the level kernels are counted
    monkeypatch.setenv("WFST_WIDE_EST_STATES", "64")
    retries = gpu_ctx.stats()["compose_retries"]
    rustfst_amd.replace(99, dev_pairs(wide_input(), gpu_ctx), True)
    st = gpu_ctx.replace_stats()
    assert st["arena_grows"] >= 2 and gpu_ctx.stats()["compose_retries"] == retries
    assert st["level_launches"] >= 3 * st["levels"] and st["level_launches"] % 3 == 0


@pytest.mark.gpu
def test_surface_and_ko_messages(gpu_ctx, wfst_lib):
    """VectorFst items give a VectorFst, DeviceFst items a DeviceFst; every KO of the header's list, before any launch"""
    import rustfst_amd
    from rustfst_amd import _lib
    g = golden()
    c = next(c for c in g["cases"] if c["name"] == "word_full_ilabel")  # (a word with bits in it: it travels both ways)
    pairs = golden_pairs(c, g)
    handles = dev_pairs(pairs, gpu_ctx)
    exp = fst_to_flat(golden_fst(c["expected"]))
    on_device = rustfst_amd.replace(99, handles, False)
    assert isinstance(on_device, rustfst_amd.DeviceFst)
    vecs = [(label, h.to_vector_fst()) for label, h in handles]
    as_vector = rustfst_amd.replace(99, vecs, False)
    assert isinstance(as_vector, rustfst_amd.VectorFst)
    assert_flat_identical(on_device.to_flat(), exp, "DeviceFst items", check_props=True)
    assert as_vector.properties() & ALL == exp["props"]
    assert_flat_identical(as_vector.to_device(gpu_ctx).to_flat(), exp, "VectorFst items", check_props=True)
    with pytest.raises(rustfst_amd.WfstError, match=re.escape(MSG_ROOT.format(5))):
        rustfst_amd.replace(5, handles, True)
    with pytest.raises(rustfst_amd.WfstError, match=re.escape(MSG_ROOT.format(99))):
        rustfst_amd.replace(99, [], True)
    raw = (_lib.LabelFstPair * 2)()
    for i, (label, h) in enumerate(handles):
        raw[i].label, raw[i].fst = label, h._h.value if isinstance(h._h, C.c_void_p) else h._h
    out = C.c_void_p(1)
    assert "null" in helpers.ko_message(wfst_lib.wfst_replace(gpu_ctx._h, 99, None, 2, 1, C.byref(out)))
    assert out.value is None
    assert "null" in helpers.ko_message(wfst_lib.wfst_replace(gpu_ctx._h, 99, raw, 2, 1, None))
    raw[1].fst = None
    assert helpers.ko_message(wfst_lib.wfst_replace(gpu_ctx._h, 99, raw, 2, 1, C.byref(out))) == "item 1: null FST in list"
    other = rustfst_amd.Context(0)
    foreign = dev(pairs[1][1], other)
    from rustfst_amd import fst as fst_module
    with pytest.raises(rustfst_amd.WfstError, match="replace: item 1 belongs to another context"):
        fst_module._device_replace(99, [handles[0], (100, foreign)], True, gpu_ctx)
    assert wfst_lib.wfst_ctx_get_replace_stats(gpu_ctx._h, *[None] * 11) == 0
