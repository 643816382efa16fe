"""top_sort and state_sort (wfst_top_sort, wfst_state_sort, wfst_ctx_get_top_sort_stats): the C-ABI surface without a GPU, a
literal sequential Python restatement of rustfst's dfs_visit.rs:97-187 with top_sort.rs's TopOrderVisitor, of
state_sort.rs:16-78 (cycle by cycle, as the reference permutes) and of top_sort.rs:76-94 (oracle/model/top_sort.py), checked against the hand-traced
K19 known answers, and on the device bit-exact parity with the restatement: states, arc order, weights by bit pattern,
finals, start state and property word.

wfst_state_sort's size check needs a handle, which needs a device: without a GPU the message is checked on the restatement
(K19 state_sort_bad_size) and the NULL arguments on the library; with one, the same message comes from the library
(test_ko_messages_and_the_context_afterwards)."""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import model
from oracle.model import (ACCEPTOR, ACCESSIBLE, ACYCLIC, COACCESSIBLE, CYCLIC, INITIAL_ACYCLIC, MSG_ACYCLIC, NOT_STRING,
                          NOT_TOP_SORTED, TOP_SORTED, dfs_top_order, fold_ref, fst_to_flat, norm, optimize_ref,
                          state_sort_ref, top_sort_ref)
import helpers
from helpers import ROOT, _vector_fst, assert_flat_identical, dev, enumerate_paths, golden_fst, make_fst
import minimize_cases as mc
from inputs import chain, random_shuffled_dag, top_sort_golden

NEW_SYMBOLS = ("wfst_state_sort", "wfst_top_sort", "wfst_ctx_get_top_sort_stats")
MSG_PERMUTATION = "state_sort: order is not a permutation of the states"


def is_permutation(order, n):
    return sorted(int(x) for x in order) == list(range(n))


def run_dev(c, g, ctx):
    h = dev(golden_fst(g["machines"][c["arg"]]), ctx)
    return h.top_sort() if c["op"] == "top_sort" else h.state_sort(c["order"])


def run_ref(c, g):
    m = golden_fst(g["machines"][c["arg"]])
    return top_sort_ref(m) if c["op"] == "top_sort" else state_sort_ref(copy.deepcopy(m), c["order"])


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
    m = re.search(r"#define\s+WFST_ABI_VERSION\s+7\b(.*)", header)
    assert m and all(name in m.group(1).split("; 6:")[0] for name in NEW_SYMBOLS) and wfst_lib.wfst_abi_version() == 7


def test_argument_validation_without_gpu(wfst_lib):
    out = C.c_void_p(1)
    order = (C.c_uint32 * 2)(1, 0)
    assert "null" in helpers.ko_message(wfst_lib.wfst_top_sort(None, None, C.byref(out)))
    assert out.value is None
    out = C.c_void_p(1)
    assert "null" in helpers.ko_message(wfst_lib.wfst_state_sort(None, None, order, 2, C.byref(out)))
    assert out.value is None
    assert "null" in helpers.ko_message(wfst_lib.wfst_top_sort(None, None, None))
    assert "null" in helpers.ko_message(wfst_lib.wfst_state_sort(None, None, order, 2, None))
    assert "null" in helpers.ko_message(wfst_lib.wfst_ctx_get_top_sort_stats(None, *[None] * 10))


def test_python_surface():
    import rustfst_amd
    for name in ("top_sort", "state_sort"):
        assert callable(getattr(rustfst_amd, name)), name
        assert name in rustfst_amd.__all__
        for cls in (rustfst_amd.DeviceFst, rustfst_amd.VectorFst):
            assert callable(getattr(cls, name)), (cls, name)
    assert callable(rustfst_amd.Context.top_sort_stats)
    from rustfst_amd import build
    assert "top_sort.hip" in build.SOURCES


def test_k19_restatement_reproduces_the_derivations():
    """the hand traces of K19_DERIVATION.md, replayed by this file's restatement (checks the restatement itself)"""
    g = top_sort_golden()
    assert len(g["cases"]) == 12
    for c in g["cases"]:
        m = golden_fst(g["machines"][c["arg"]])
        if c["op"] == "top_sort":
            acyclic, order = dfs_top_order(m)
            assert acyclic == (c["order"] is not None), c["name"]
            assert not acyclic or order == c["order"], c["name"]
        if "error" in c:
            with pytest.raises(ValueError, match=re.escape(c["error"])):
                run_ref(c, g)
            continue
        assert_flat_identical(fst_to_flat(run_ref(c, g)), fst_to_flat(golden_fst(c["expected"])), c["name"], check_props=True)


def test_cyclic_keeps_a_stale_acyclic_word():
    """top_sort.rs:88-91: p equals its own mask, so CYCLIC | NOT_TOP_SORTED are set and nothing is cleared"""
    g = top_sort_golden()
    got = top_sort_ref(golden_fst(g["machines"]["self_loop"]))
    assert got["props"] == ACCEPTOR | ACYCLIC | INITIAL_ACYCLIC | TOP_SORTED | CYCLIC | NOT_TOP_SORTED


def test_restated_result_is_top_sorted():
    """every arc of the restated result goes from a lower to a higher state, the order is a permutation, and the result is
    the input renamed: state order[s] holds s's arcs in their stored order"""
    rng = np.random.default_rng(1901)
    for i in range(300):
        n = int(rng.integers(1, 15))
        m = random_shuffled_dag(rng, n)
        acyclic, order = dfs_top_order(m)
        assert acyclic and is_permutation(order, n), i
        got = top_sort_ref(m)
        assert got["start"] == order[m["start"]]
        for s, row in enumerate(got["rows"]):
            assert all(ns > s for _, _, _, ns in row), (i, s)
        for s in range(n):
            assert got["rows"][order[s]] == [[il, ol, w, order[ns]] for il, ol, w, ns in m["rows"][s]], (i, s)
            assert got["finals"][order[s]] == m["finals"][s], (i, s)
        assert got["props"] == ACYCLIC | INITIAL_ACYCLIC | TOP_SORTED


def test_start_is_not_always_numbered_zero():
    """the start state is the first root, but a later root finishes later still and takes a lower number: the start becomes
    state 0 only when it is the only root (K19 root_with_predecessor is the counterexample)"""
    g = top_sort_golden()
    c = {c["name"]: c for c in g["cases"]}
    assert c["root_with_predecessor"]["expected"]["start"] == 1 and c["reference_python_test"]["expected"]["start"] == 0


# ================================================================ on the device
def _check_case(c, g, ctx):
    import rustfst_amd
    if "error" in c:
        with pytest.raises(rustfst_amd.WfstError, match=re.escape(c["error"])):
            run_dev(c, g, ctx)
        return
    got = run_dev(c, g, ctx).to_flat()
    assert_flat_identical(got, fst_to_flat(golden_fst(c["expected"])), c["name"], check_props=True)


@pytest.mark.gpu
def test_k19_on_the_device(gpu_ctx):
    g = top_sort_golden()
    for c in g["cases"]:
        _check_case(c, g, gpu_ctx)
        if c["op"] == "top_sort" and "error" not in c:
            assert gpu_ctx.top_sort_stats()["cyclic"] == (1 if c["order"] is None else 0), c["name"]


WORDS = ("content_word", "word_0", "stale_cyclic")


@pytest.mark.gpu
@pytest.mark.parametrize("word", WORDS)
@pytest.mark.parametrize("where", ("start_0", "start_last", "start_middle"))
def test_random_dags_against_the_restatement(gpu_ctx, word, where):
    rng = np.random.default_rng(1902 + WORDS.index(word))
    for i in range(40):
        n = int(rng.integers(1, 60)) if i else 1
        m = random_shuffled_dag(rng, n, start={"start_0": 0, "start_last": n - 1, "start_middle": n // 2}[where])
        if word == "content_word":
            m["props"] = model.content_word(m)
        elif word == "stale_cyclic":
            m["props"] = (model.content_word(m) & ~(ACYCLIC | INITIAL_ACYCLIC)) | CYCLIC
        exp = top_sort_ref(m)
        h = dev(m, gpu_ctx)
        before = h.to_flat()
        assert_flat_identical(h.top_sort().to_flat(), fst_to_flat(exp), f"{word} {where} dag {i}", check_props=True)
        assert_flat_identical(h.to_flat(), before, "the input after top_sort", check_props=True)
        assert exp["props"] & (ACYCLIC | INITIAL_ACYCLIC | TOP_SORTED) == ACYCLIC | INITIAL_ACYCLIC | TOP_SORTED
        if word == "stale_cyclic":
            assert exp["props"] & CYCLIC


@pytest.mark.gpu
def test_random_cyclic_inputs_come_back_as_copies(gpu_ctx):
    rng = np.random.default_rng(1903)
    for i in range(20):
        n = int(rng.integers(2, 40))
        m = random_shuffled_dag(rng, n)
        a, b = (int(x) for x in rng.choice(n, 2, replace=False))
        _, order = dfs_top_order(m)
        lo, hi = (a, b) if order[a] < order[b] else (b, a)
        m["rows"][hi].append([1, 1, 0.0, lo])  # an arc against the order ...
        m["rows"][lo].append([2, 2, 0.0, hi])  # ... and one along it: a cycle
        m["props"] = ACYCLIC | TOP_SORTED | INITIAL_ACYCLIC if i % 2 else 0
        exp = top_sort_ref(m)
        assert exp["props"] == m["props"] | CYCLIC | NOT_TOP_SORTED and exp["rows"] == m["rows"]
        assert_flat_identical(dev(m, gpu_ctx).top_sort().to_flat(), fst_to_flat(exp), f"cyclic {i}", check_props=True)
        assert gpu_ctx.top_sort_stats()["cyclic"] == 1


@pytest.mark.gpu
def test_state_sort_cases(gpu_ctx):
    import rustfst_amd
    rng = np.random.default_rng(1904)
    for n in (1, 2, 7, 300, 1000):
        m = chain(n, rng, fan=3, start=int(rng.integers(0, n))) if n > 1 else make_fst([[]], [0.5], 0)
        m["props"] = model.content_word(m)
        h = dev(m, gpu_ctx)
        for name, order in (("random", rng.permutation(n).tolist()), ("identity", list(range(n)))):
            exp = state_sort_ref(copy.deepcopy(m), order)
            assert_flat_identical(h.state_sort(order).to_flat(), fst_to_flat(exp), f"state_sort {name} n={n}", check_props=True)
        if n > 1:
            for bad in ([0] * n, list(range(1, n + 1)), [0] + list(range(n - 1))):
                with pytest.raises(rustfst_amd.WfstError, match=re.escape(MSG_PERMUTATION)):
                    h.state_sort(bad)
        assert_flat_identical(h.to_flat(), fst_to_flat(m), "the input after state_sort", check_props=True)
    # start-less: a copy, word unchanged, whatever the order says
    m = make_fst([[[1, 1, 0.5, 1]], [], [[2, 3, 0.0, 0]]], [None, 0.25, None], None, ACCEPTOR | TOP_SORTED | NOT_STRING)
    assert_flat_identical(dev(m, gpu_ctx).state_sort([2, 0, 1]).to_flat(), fst_to_flat(m), "start-less state_sort", check_props=True)
    empty = make_fst([], [], None, ACCEPTOR)
    assert_flat_identical(dev(empty, gpu_ctx).state_sort([]).to_flat(), fst_to_flat(empty), "state_sort without states", check_props=True)


@pytest.mark.gpu
def test_ko_messages_and_the_context_afterwards(gpu_ctx, monkeypatch):
    import rustfst_amd
    from rustfst_amd import _lib
    L = _lib.lib()
    g = top_sort_golden()
    diamond = golden_fst(g["machines"]["diamond"])
    h = dev(diamond, gpu_ctx)
    out = C.c_void_p(1)
    order = (C.c_uint32 * 3)(0, 1, 2)
    assert helpers.ko_message(L.wfst_state_sort(gpu_ctx._h, h._h, order, 3, C.byref(out))) == "StateSort : Bad order vector size : 3. Expected 4"
    assert out.value is None
    assert "null" in helpers.ko_message(L.wfst_state_sort(gpu_ctx._h, h._h, None, 4, C.byref(out)))
    assert "null" in helpers.ko_message(L.wfst_top_sort(gpu_ctx._h, h._h, None))
    with pytest.raises(rustfst_amd.WfstError, match=re.escape(MSG_PERMUTATION)):
        h.state_sort([0, 1, 1, 3])
    with pytest.raises(rustfst_amd.WfstError, match=re.escape(MSG_PERMUTATION)):
        h.state_sort([0, 1, 2, 4])
    no_start = dev(golden_fst(g["machines"]["two_states_no_start"]), gpu_ctx)
    with pytest.raises(rustfst_amd.WfstError, match=re.escape("StateSort : Bad order vector size : 0. Expected 2")):
        no_start.top_sort()
    monkeypatch.setenv("WFST_TOP_SORT_PATH", "sideways")
    with pytest.raises(rustfst_amd.WfstError, match="WFST_TOP_SORT_PATH"):
        h.top_sort()
    monkeypatch.delenv("WFST_TOP_SORT_PATH")
    # ... and the same context, the same handle, successful calls
    cases = {c["name"]: c for c in g["cases"]}
    assert_flat_identical(h.top_sort().to_flat(), fst_to_flat(golden_fst(cases["diamond_second_arc_first"]["expected"])),
                          "top_sort after the KOs", check_props=True)
    assert_flat_identical(h.state_sort([2, 3, 0, 1]).to_flat(), fst_to_flat(golden_fst(cases["state_sort_two_cycles"]["expected"])),
                          "state_sort after the KOs", check_props=True)


@pytest.mark.gpu
def test_vector_fst_and_module_surface(gpu_ctx):
    """rustfst-python's test_top_sort: in place, returns self, the start moves from the second state to the first"""
    import rustfst_amd
    g = top_sort_golden()
    cases = {c["name"]: c for c in g["cases"]}
    m = golden_fst(g["machines"]["reference_python_test"])
    expected = _vector_fst(golden_fst(cases["reference_python_test"]["expected"]))
    f = _vector_fst(m)
    assert f.start() == 1
    assert f.top_sort() is f
    assert f.start() == 0 and f == expected
    f2 = _vector_fst(m)
    assert rustfst_amd.top_sort(f2) is f2 and f2 == expected
    assert rustfst_amd.state_sort(f2, [1, 0]) is f2 and f2 == _vector_fst(m)
    f3 = _vector_fst(m)
    assert f3.state_sort([0, 1]) is f3 and f3 == _vector_fst(m)


@pytest.mark.gpu
def test_union_of_nbest_paths_top_sort_then_optimize(gpu_ctx, oracle):
    """the chain this was built for: union_list of the n best strings -> top_sort -> optimize.  optimize straight on the
    union is still KO (union_properties never holds TOP_SORTED, and rm_epsilon's set_trs bookkeeping then drops ACYCLIC);
    after top_sort the word holds TOP_SORTED and ACYCLIC and the restated optimize accepts it, as the device does."""
    import rustfst_amd
    rng = np.random.default_rng(1806)
    word = ACCEPTOR | ACYCLIC | INITIAL_ACYCLIC | ACCESSIBLE | COACCESSIBLE
    lattice = mc.random_dag(rng, 12, 4)
    paths = sorted(enumerate_paths(lattice))[:5]
    assert len(paths) == 5
    strings = []
    for w, il, _ in paths:
        il = list(il) or [1]
        rows = [[[x, x, w if i == 0 else 0.0, i + 1]] for i, x in enumerate(il)] + [[]]
        strings.append(make_fst(rows, [None] * len(il) + [0.0], 0, word))
    union = rustfst_amd.union_list([dev(s, gpu_ctx) for s in strings])
    union_ref = fold_ref(model.union_ref, strings)
    with pytest.raises(rustfst_amd.WfstError, match=re.escape(MSG_ACYCLIC)):
        union.optimize()
    sorted_ref = top_sort_ref(union_ref)
    sorted_dev = union.top_sort()
    assert_flat_identical(sorted_dev.to_flat(), fst_to_flat(sorted_ref), "top_sort(union_list(n-best))", check_props=True)
    exp = optimize_ref(fst_to_flat(sorted_ref), oracle)  # (raises Unsupported if the restatement itself answers KO)
    got = sorted_dev.optimize()
    assert exp["n_states"] < len(union_ref["rows"])
    assert_flat_identical(norm(got.to_flat()), norm(exp), "optimize(top_sort(union_list(n-best)))", check_props=True)
