"""union, concat, closure and the list forms (wfst_union, wfst_concat, wfst_closure, wfst_union_list, wfst_concat_list): the
C-ABI surface without a GPU, a literal sequential Python restatement of rustfst's union_static.rs, concat_static.rs and
closure_static.rs with the property functions they call (union_properties, concat_properties, closure_properties,
compute_and_update_properties(INITIAL_ACYCLIC)) (oracle/model/rational.py) checked against the hand-derived K18 known answers,
the closed forms of the list folds checked against the literal folds, and on the device bit-exact parity with the
restatement: states, offsets, arcs (weights by bit pattern), finals, start state and property word.

The restatement reuses the per-mutation property functions, the DFS facts and the flat <-> fst conversions of
oracle/model/props.py and oracle/model/fst.py.

Shapes of the list tests, and why: the copy kernel covers the concatenation of all items' states (and arcs) with tiles of
TILE = 256 elements, one lane per element, and finds a lane's item between the first items of two neighbouring tiles.  So
the lists hold an item smaller than a tile next to items without arcs and to FSTs without states, an item of more than
three tiles, a row that begins 16 arcs before a tile edge, a row of more than two tiles, an item whose final states all
lie in its last tile, and once more items than a tile has lanes."""
import copy
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from oracle import model
from oracle.model import (ACCEPTOR, ACCESSIBLE, ACYCLIC, COACCESSIBLE, EPSILONS, INITIAL_ACYCLIC, I_EPSILONS,
                          MSG_ACYCLIC, O_EPSILONS, PLUS, STAR, closure_ref, concat_list_closed, concat_properties,
                          concat_ref, content_word, fold_ref, fst_to_flat, m_add_state, m_add_tr, m_set_final,
                          m_set_start, norm, optimize_ref, union_list_closed, union_properties, union_ref)
from helpers import (_vector_fst, assert_flat_identical, dev, enumerate_paths, golden_fst, ko_message, make_fst,
                     to_device)
import minimize_cases as mc
from inputs import chain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "k18_rational.json")
NEW_SYMBOLS = ("wfst_union", "wfst_concat", "wfst_closure", "wfst_union_list", "wfst_concat_list")
F32, INF = np.float32, np.float32(np.inf)
TILE = 256  # rustfst_amd/csrc/rational.hip
MAX_STATES, MAX_ARCS = 2 ** 31 - 2, 2 ** 32 - 1


# ---------------------------------------------------------------- inputs
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def run_ref(op, args, closure_type=None):
    args = [copy.deepcopy(a) for a in args]
    if op == "union":
        return union_ref(*args)
    if op == "concat":
        return concat_ref(*args)
    if op == "closure":
        return closure_ref(args[0], closure_type)
    return fold_ref(union_ref if op == "union_list" else concat_ref, args)


SHAPES = ("empty", "no_start", "one_state", "start_last", "start_no_arcs", "start_self_loop", "start_cycle3",
          "unreachable_into_start", "all_final", "none_final")


def shape_fst(name, rng):
    """one operand of the pair tests.  Arcs on cycles carry weight one or zero (oracle.model's compute_and_update does not
    restate the SCC test of WEIGHTED_CYCLES); final weights and the arcs of the acyclic shapes are weighted."""
    def lab():
        return int(rng.integers(0, 4))

    def arc(ns, w=None):
        il = lab()
        return [il, il if rng.random() < 0.6 else lab(), float(rng.integers(1, 9)) / 4 if w is None else w, ns]

    def fin(p=0.5):
        return float(rng.integers(0, 8)) / 4 if rng.random() < p else None
    if name == "empty":
        return make_fst([], [], None)
    if name == "no_start":
        return make_fst([[arc(1), arc(2)], [arc(3)], [arc(3), arc(1, 0.0)], []], [None, fin(), 0.5, fin()], None)
    if name == "one_state":
        return make_fst([[]], [0.5], 0)
    if name == "start_last":
        return make_fst([[arc(1), arc(2)], [arc(3)], [arc(3)], [], [arc(0), arc(2), arc(3)]], [None, fin(), None, 1.25, fin()], 4)
    if name == "start_no_arcs":
        return make_fst([[], [arc(2)], [arc(0)]], [0.75, None, fin()], 0)
    if name == "start_self_loop":
        return make_fst([[arc(0, 0.0), arc(1, 0.0)], [arc(2, 0.0)], []], [fin(), None, 2.0], 0)
    if name == "start_cycle3":
        return make_fst([[arc(2, 0.0)], [arc(3, 0.0), arc(0, 0.0)], [arc(1, 0.0)], [arc(4, 0.0)], []], [None, None, fin(), None, 0.25], 1)
    if name == "unreachable_into_start":
        return make_fst([[arc(1), arc(2)], [arc(2)], [], [arc(0), arc(2)]], [None, fin(), 1.0, None], 0)
    if name == "all_final":
        return make_fst([[arc(1), arc(2)], [arc(2)], []], [0.0, 0.5, 1.5], 0)
    assert name == "none_final"
    return make_fst([[arc(1), arc(2)], [arc(2)], []], [None, None, None], 0)


def fat_row(k, rng):
    """two states, the first with k arcs"""
    return make_fst([[[int(rng.integers(1, 50)), int(rng.integers(1, 50)), float(rng.integers(0, 16)) / 8, int(rng.integers(0, 2))]
                      for _ in range(k)], []], [0.5, 0.25], 0)


def list_items(n, rng, with_empties):
    """see the module docstring; n = 1, 2, 3 take the first items"""
    no_states = make_fst([], [], None)
    no_arcs = make_fst([[]], [1.5], 0)
    items = [chain(3, rng, fan=2),                        # smaller than a tile
             no_arcs, no_states if with_empties else no_arcs, no_arcs,
             chain(TILE - 16 - 3, rng, fan=1),            # brings the arc count to 16 below the tile edge ...
             fat_row(40, rng),                            # ... so that this row crosses it
             chain(3 * TILE + 37, rng, fan=2),            # more than three tiles of states, more than six of arcs
             fat_row(2 * TILE + 9, rng),                  # one row longer than a tile
             chain(2 * TILE + 88, rng, finals_from=2 * TILE + 5, fan=1)]  # final states in the last tile only
    while len(items) < n:
        pick = int(rng.integers(0, 4))
        items.append([no_arcs, no_states if with_empties else no_arcs, chain(2, rng), chain(5, rng, fan=2)][pick])
    return items[:n]


LIST_SIZES = (1, 2, 3, 65, TILE + 44)


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


def test_tile_constant_is_the_kernels():
    with open(os.path.join(ROOT, "rustfst_amd", "csrc", "rational.hip")) as f:
        m = re.search(r"constexpr uint32_t TILE = (\d+);", f.read())
    assert m and int(m.group(1)) == TILE


def test_argument_validation_without_gpu(wfst_lib):
    out = C.c_void_p(1)
    assert "null" in ko_message(wfst_lib.wfst_union(None, None, None, C.byref(out)))
    assert out.value is None
    assert "null" in ko_message(wfst_lib.wfst_concat(None, None, None, C.byref(out)))
    assert "null" in ko_message(wfst_lib.wfst_closure(None, None, 0, C.byref(out)))
    assert "closure_type" in ko_message(wfst_lib.wfst_closure(None, None, 2, C.byref(out)))
    arr = (C.c_void_p * 2)()
    for fn in (wfst_lib.wfst_union_list, wfst_lib.wfst_concat_list):
        assert ko_message(fn(None, arr, 0, C.byref(out))) == "fsts must be at least of len 1"
        assert "null" in ko_message(fn(None, arr, 2, C.byref(out)))
        assert "null" in ko_message(fn(None, None, 2, C.byref(out)))
        assert "null" in ko_message(fn(None, arr, 2, None))


def _check_sizes(lib, op, states, arcs):
    ns, na = np.array(states, dtype=np.uint64), np.array(arcs, dtype=np.uint64)
    return lib.wfst_rational_check_sizes(op, ns.ctypes.data, na.ctypes.data, len(states))


def test_overflow_guard_on_bare_counts(wfst_lib):
    """wfst_rational_check_sizes IS the function each of the five calls runs first (rational.hip rational_check_sizes), here on
    bare counts (no 2^32-arc allocation).  States: the sum, + 1 for union and closure star; arcs by their upper bound: the sum,
    + n for union, + the states of every operand but the last for concat, + the states (+ 1 for star) for closure."""
    assert _check_sizes(wfst_lib, 0, [1000, 2000], [5000, 7000]) == 0
    # union: states
    assert _check_sizes(wfst_lib, 0, [MAX_STATES - 10, 9], [5, 5]) == 0                 # + the new start state: the limit
    msg = ko_message(_check_sizes(wfst_lib, 0, [MAX_STATES - 10, 10], [5, 5]))
    assert msg == f"union: result too large: up to {MAX_STATES + 1} states, the limit is {MAX_STATES}"
    # union: arcs, + n
    assert _check_sizes(wfst_lib, 0, [10, 10], [2 ** 31, 2 ** 31 - 3]) == 0
    msg = ko_message(_check_sizes(wfst_lib, 0, [10, 10], [2 ** 31, 2 ** 31 - 2]))
    assert msg == f"union: result too large: up to {MAX_ARCS + 1} arcs, the limit is {MAX_ARCS}"
    assert _check_sizes(wfst_lib, 0, [1, 1, 1], [2 ** 31, 2 ** 31 - 4, 0]) == 0
    assert "arcs" in ko_message(_check_sizes(wfst_lib, 0, [1, 1, 1], [2 ** 31, 2 ** 31 - 3, 0]))
    # concat: the last operand's states append nothing
    assert _check_sizes(wfst_lib, 1, [10, 1000], [2 ** 31, 2 ** 31 - 11]) == 0
    msg = ko_message(_check_sizes(wfst_lib, 1, [10, 1000], [2 ** 31, 2 ** 31 - 10]))
    assert msg == f"concat: result too large: up to {MAX_ARCS + 1} arcs, the limit is {MAX_ARCS}"
    assert _check_sizes(wfst_lib, 1, [2 ** 30, 2 ** 30 - 2], [0, 0]) == 0
    assert "states" in ko_message(_check_sizes(wfst_lib, 1, [2 ** 30, 2 ** 30 - 1], [0, 0]))
    # closure: star adds a state and an arc
    assert _check_sizes(wfst_lib, 3, [MAX_STATES], [5]) == 0
    assert "closure: result too large" in ko_message(_check_sizes(wfst_lib, 2, [MAX_STATES], [5]))
    assert _check_sizes(wfst_lib, 3, [100], [MAX_ARCS - 100]) == 0
    assert "arcs" in ko_message(_check_sizes(wfst_lib, 2, [100], [MAX_ARCS - 100]))
    assert "arcs" in ko_message(_check_sizes(wfst_lib, 3, [100], [MAX_ARCS - 99]))
    assert _check_sizes(wfst_lib, 0, [5, 5], [5, 5]) == 0                               # and the library works afterwards


def test_entry_points_call_the_one_size_rule():
    """the five calls have no size arithmetic of their own: each goes through check_sizes_of -> rational_check_sizes, and
    nothing else in the file throws the "too large" message"""
    with open(os.path.join(ROOT, "rustfst_amd", "csrc", "rational.hip")) as f:
        src = f.read()
    assert src.count("too large") == 1 and src.count("rational_check_sizes(op, ns.data(), na.data(), n)") == 1
    for fn, call in (("union_fst", "check_sizes_of(0, both, 2)"), ("concat_fst", "check_sizes_of(1, both, 2)"),
                     ("closure_fst", "check_sizes_of(star ? 2 : 3, &f, 1)"),
                     ("union_list_fst", 'check_list(ctx, fsts, n, "union_list", 0)'),
                     ("concat_list_fst", 'check_list(ctx, fsts, n, "concat_list", 1)')):
        body = src[src.index("wfst_fst* " + fn + "("):]
        body = body[:body.index("\n}\n")]
        assert call in body, fn
        first_launch = min([body.index(k) for k in ("run_plan", "word_with_initial_pair", "ensure_", "copy_with_props") if k in body])
        assert body.index(call) < first_launch, fn
    assert "check_sizes_of(size_op, fsts, n)" in src


def test_python_surface():
    import rustfst_amd
    assert [m.name for m in rustfst_amd.ClosureType] == ["CLOSURE_STAR", "CLOSURE_PLUS"]
    assert rustfst_amd.ClosureType.CLOSURE_STAR.value == 0 and rustfst_amd.ClosureType.CLOSURE_PLUS.value == 1
    for name in ("union", "concat", "closure", "union_list", "concat_list"):
        assert callable(getattr(rustfst_amd, name)), name
        assert name in rustfst_amd.__all__
    for cls in (rustfst_amd.DeviceFst, rustfst_amd.VectorFst):
        for name in ("union", "concat", "closure"):
            assert callable(getattr(cls, name)), (cls, name)
    for fn in (rustfst_amd.union_list, rustfst_amd.concat_list):
        with pytest.raises(ValueError, match="fsts must be at least of len 1"):
            fn([])


def _golden_args(g, c):
    return [golden_fst(g["machines"][a]) for a in c["args"]]


def test_k18_restatement_reproduces_the_derivations():
    """the hand derivations of K18_DERIVATION.md, replayed by this file's restatement (checks the restatement itself)"""
    g = golden()
    assert len(g["cases"]) == 15
    for c in g["cases"]:
        got = run_ref(c["op"], _golden_args(g, c), c.get("closure_type"))
        assert_flat_identical(fst_to_flat(got), fst_to_flat(golden_fst(c["expected"])), c["name"], check_props=True)


def test_the_reference_test_words_are_the_incremental_ones():
    """the two machines of rustfst-python's test_union / test_concat_fst carry the word their add_state / set_start / set_final
    / add_tr calls leave (K18_DERIVATION.md derives it by hand)"""
    g = golden()
    for name in ("ref_union_1", "ref_union_2", "ref_concat_2"):
        m = golden_fst(g["machines"][name])
        f = dict(rows=[], finals=[], start=None, props=model.NULL_PROPS)
        for _ in m["rows"]:
            m_add_state(f)
        m_set_start(f, m["start"])
        for s, w in enumerate(m["finals"]):
            if w is not None:
                m_set_final(f, s, w)
        for s, row in enumerate(m["rows"]):
            for tr in row:
                m_add_tr(f, s, tr)
        assert f["props"] == m["props"], name


def random_small(rng):
    n = int(rng.integers(0, 5))
    rows = [[[int(rng.integers(0, 3)), int(rng.integers(0, 3)), float(rng.integers(0, 4)) / 2, int(rng.integers(0, n))]
             for _ in range(int(rng.integers(0, 3)))] for _ in range(n)]
    finals = [float(rng.integers(0, 4)) / 2 if rng.random() < 0.5 else None for _ in range(n)]
    start = int(rng.integers(0, n)) if n and rng.random() < 0.8 else None
    return make_fst(rows, finals, start, 0)


def test_closed_forms_equal_the_literal_folds():
    rng = np.random.default_rng(18)
    checked = [0, 0]
    for _ in range(1500):
        fsts = [random_small(rng) for _ in range(int(rng.integers(2, 6)))]
        if fsts[0]["start"] is not None:
            lit = fold_ref(union_ref, fsts)
            rows, finals, start = union_list_closed(fsts)
            assert (lit["rows"], lit["finals"], lit["start"]) == (rows, finals, start)
            checked[0] += 1
        if all(f["start"] is not None for f in fsts):
            lit = fold_ref(concat_ref, fsts)
            rows, finals, start = concat_list_closed(fsts)
            assert (lit["rows"], lit["finals"], lit["start"]) == (rows, finals, start)
            checked[1] += 1
    assert checked[0] > 800 and checked[1] > 200


# ================================================================ GPU
def run_dev(op, handles, closure_type=None):
    import rustfst_amd
    if op == "union":
        return handles[0].union(handles[1])
    if op == "concat":
        return handles[0].concat(handles[1])
    if op == "closure":
        return handles[0].closure(rustfst_amd.ClosureType(closure_type))
    return (rustfst_amd.union_list if op == "union_list" else rustfst_amd.concat_list)(handles)


def check_op(op, args, ctx, what, closure_type=None):
    """the device result against the restatement, and the operands unchanged"""
    handles = [dev(a, ctx) for a in args]
    before = [h.to_flat() for h in handles]
    got = run_dev(op, handles, closure_type)
    exp = run_ref(op, args, closure_type)
    assert_flat_identical(got.to_flat(), fst_to_flat(exp), what, check_props=True)
    for h, b, i in zip(handles, before, range(len(handles))):
        assert_flat_identical(h.to_flat(), b, f"{what}: operand {i} after the call", check_props=True)
    return got


@pytest.mark.gpu
def test_k18_on_the_device(gpu_ctx):
    g = golden()
    for c in g["cases"]:
        args = _golden_args(g, c)
        got = run_dev(c["op"], [dev(a, gpu_ctx) for a in args], c.get("closure_type"))
        assert_flat_identical(got.to_flat(), fst_to_flat(golden_fst(c["expected"])), c["name"], check_props=True)
        if c["op"] in ("union", "concat"):  # the pairwise cases through the list entry points as well
            got = run_dev(c["op"] + "_list", [dev(a, gpu_ctx) for a in args])
            assert_flat_identical(got.to_flat(), fst_to_flat(golden_fst(c["expected"])), c["name"] + " (list)", check_props=True)


@pytest.mark.gpu
@pytest.mark.parametrize("full_word", (True, False), ids=("content_word", "word_0"))
@pytest.mark.parametrize("op", ("union", "concat"))
def test_pairs_over_the_operand_shapes(gpu_ctx, op, full_word):
    """word 0 forces the device INITIAL_ACYCLIC search and the merge_dfs of the word"""
    rng = np.random.default_rng(1801)
    for na in SHAPES:
        for nb in SHAPES:
            a, b = shape_fst(na, rng), shape_fst(nb, rng)
            if full_word:
                a["props"], b["props"] = content_word(a), content_word(b)
            check_op(op, [a, b], gpu_ctx, f"{op}({na}, {nb})")


@pytest.mark.gpu
@pytest.mark.parametrize("full_word", (True, False), ids=("content_word", "word_0"))
def test_closure_over_the_operand_shapes(gpu_ctx, full_word):
    rng = np.random.default_rng(1802)
    for name in SHAPES:
        for ct in (STAR, PLUS):
            f = shape_fst(name, rng)
            if full_word:
                f["props"] = content_word(f)
            check_op("closure", [f], gpu_ctx, f"closure({name}, {ct})", ct)


@pytest.mark.gpu
@pytest.mark.parametrize("n", LIST_SIZES)
@pytest.mark.parametrize("op", ("union_list", "concat_list"))
def test_lists_against_the_fold(gpu_ctx, op, n):
    rng = np.random.default_rng(1803 + n)
    items = list_items(n, rng, with_empties=(op == "union_list"))
    check_op(op, items, gpu_ctx, f"{op} of {n}")


@pytest.mark.gpu
@pytest.mark.parametrize("cap", (1, 3))
def test_blocks_stride_over_tiles(gpu_ctx, monkeypatch, cap):
    """WFST_RATIONAL_MAX_BLOCKS caps the grid: with 1 and 3 blocks for more than twenty tiles every block handles several
    tiles of both passes, the trailing append tiles of concat and closure included"""
    monkeypatch.setenv("WFST_RATIONAL_MAX_BLOCKS", str(cap))
    rng = np.random.default_rng(1807)
    check_op("union_list", list_items(65, rng, with_empties=True), gpu_ctx, f"union_list, {cap} blocks")
    check_op("concat_list", list_items(65, rng, with_empties=False), gpu_ctx, f"concat_list, {cap} blocks")
    big = chain(3 * TILE + 37, rng, finals_from=5, fan=2)
    check_op("closure", [big], gpu_ctx, f"closure, {cap} blocks", STAR)
    check_op("concat", [big, make_fst([], [], None)], gpu_ctx, f"concat with an empty second operand, {cap} blocks")


@pytest.mark.gpu
def test_lists_with_an_initial_cyclic_first_item_and_fallbacks(gpu_ctx):
    rng = np.random.default_rng(1804)
    cyc = shape_fst("start_cycle3", rng)
    tail = list_items(12, rng, with_empties=True)
    check_op("union_list", [cyc] + tail, gpu_ctx, "union_list, initial-cyclic first item")         # the new state behind item 1
    check_op("union_list", [cyc, make_fst([], [], None), tail[0]], gpu_ctx, "union_list, item 1 without start")
    check_op("union_list", [cyc, make_fst([], [], None)], gpu_ctx, "union_list, nothing survives")
    no_start = shape_fst("no_start", rng)
    check_op("union_list", [no_start] + tail[:4], gpu_ctx, "union_list, first item without start")  # the pairwise fallback
    check_op("concat_list", [tail[0], no_start, tail[4], tail[5]], gpu_ctx, "concat_list, an item without start")
    check_op("concat_list", [no_start, tail[0]], gpu_ctx, "concat_list, first item without start")


def string3(w=0.5):
    return make_fst([[[1, 1, w, 1]], [[2, 2, 0.0, 2]], []], [None, None, 0.0], 0, ACCEPTOR | ACYCLIC | INITIAL_ACYCLIC)


@pytest.mark.gpu
def test_closed_form_at_scale(gpu_ctx):
    import rustfst_amd
    h = dev(string3(), gpu_ctx)
    # union_list of 1000 copies: the root is state 0, its row = its arc + 999 arcs 0:0/One -> 3 k
    n = 1000
    u = rustfst_amd.union_list([h] * n).to_flat()
    assert (u["n_states"], len(u["arcs"]), u["start"]) == (3 * n, 2 * n + n - 1, 0)
    root = u["arcs"][u["offsets"][0]:u["offsets"][1]]
    assert len(root) == n and tuple(root[0]) == (1, 1, 0.5, 1)
    np.testing.assert_array_equal(root["nextstate"][1:], 3 * np.arange(1, n))
    assert not root["ilabel"][1:].any() and not root["olabel"][1:].any() and not root["weight"][1:].any()
    off = n - 1 + np.repeat(np.arange(n) * 2, 3) + np.tile([0, 1, 2], n)  # rows behind the root start n - 1 arcs later
    off[0] = 0
    np.testing.assert_array_equal(u["offsets"], np.r_[off, 3 * n - 1])
    tails = (3 * np.arange(1, n))[:, None] + np.array([1, 2])  # copy k: its two arcs into 3 k + 1 and 3 k + 2
    np.testing.assert_array_equal(u["arcs"]["nextstate"][n:], np.concatenate([[2], tails.ravel()]))
    p = string3()["props"]
    word = p
    for _ in range(n - 1):
        word = union_properties(word, p)
    assert u["props"] == word == ACCEPTOR | ACYCLIC | INITIAL_ACYCLIC | EPSILONS | I_EPSILONS | O_EPSILONS
    # concat_list of 200: state 3 k + 2 loses its final weight for 0:0/0 -> 3 (k + 1)
    n = 200
    c = rustfst_amd.concat_list([h] * n).to_flat()
    assert (c["n_states"], len(c["arcs"]), c["start"]) == (3 * n, 3 * n - 1, 0)
    np.testing.assert_array_equal(c["offsets"], np.minimum(np.arange(3 * n + 1), 3 * n - 1))
    np.testing.assert_array_equal(c["arcs"]["nextstate"], np.arange(1, 3 * n))
    np.testing.assert_array_equal(c["arcs"]["ilabel"], np.tile([1, 2, 0], n)[:-1])
    np.testing.assert_array_equal(c["arcs"]["weight"], np.tile(np.array([0.5, 0, 0], dtype=np.float32), n)[:-1])
    assert np.isinf(c["finals"][:-1]).all() and c["finals"][-1] == 0.0
    word = p
    for _ in range(n - 1):
        word = concat_properties(word, p)
    assert c["props"] == word == ACCEPTOR | ACYCLIC | INITIAL_ACYCLIC


@pytest.mark.gpu
def test_operand_still_answers_shortest_path(gpu_ctx):
    rng = np.random.default_rng(1805)
    a = chain(300, rng, fan=3)
    a["props"] = ACYCLIC | INITIAL_ACYCLIC
    b = chain(40, rng, fan=2)
    fresh = dev(a, gpu_ctx).shortest_path().to_flat()
    ha, hb = dev(a, gpu_ctx), dev(b, gpu_ctx)
    first = ha.shortest_path().to_flat()      # (the second query of a handle builds its cached transpose)
    ha.union(hb)
    ha.concat(hb)
    ha.closure(0)
    for _ in range(2):
        assert_flat_identical(ha.shortest_path().to_flat(), fresh, "shortest_path after the rational calls")
    assert_flat_identical(first, fresh, "shortest_path")


@pytest.mark.gpu
def test_union_of_nbest_paths_then_optimize(gpu_ctx, oracle):
    """the use this was built for: the n best paths of a lattice as strings, their union, optimize"""
    import rustfst_amd
    rng = np.random.default_rng(1806)
    word = ACCEPTOR | ACYCLIC | INITIAL_ACYCLIC | ACCESSIBLE | COACCESSIBLE
    lattice = mc.random_dag(rng, 12, 4)
    paths = sorted(enumerate_paths(lattice))[:5]  # (the lattice is deterministic: distinct paths, distinct strings)
    assert len(paths) == 5
    strings = []
    for w, il, _ in paths:
        il = list(il) or [1]
        rows = [[[x, x, w if i == 0 else 0.0, i + 1]] for i, x in enumerate(il)] + [[]]
        strings.append(make_fst(rows, [None] * len(il) + [0.0], 0, word))
    from helpers import to_oracle
    union = rustfst_amd.union_list([dev(s, gpu_ctx) for s in strings])
    union_flat = fst_to_flat(fold_ref(union_ref, strings))
    assert_flat_identical(union.to_flat(), union_flat, "union_list(n-best)", check_props=True)
    # optimize straight away is KO here as in the restatement: union_properties never holds TOP_SORTED, and without it the
    # set_trs bookkeeping of rm_epsilon (rm_epsilon_static.rs:148-167) drops ACYCLIC, which wfst_optimize's step 4 needs
    with pytest.raises(model.Unsupported, match=re.escape(MSG_ACYCLIC)):
        optimize_ref(union_flat, oracle)
    with pytest.raises(rustfst_amd.WfstError, match=re.escape(MSG_ACYCLIC)):
        union.optimize()
    # the caller knows that a union of acyclic machines is acyclic: rm_epsilon, ACYCLIC back into the word, optimize
    no_eps = union.rm_epsilon().to_flat()
    no_eps_ref = norm(to_oracle(oracle, norm(union_flat)).rm_epsilon().to_flat())
    assert_flat_identical(norm(no_eps), no_eps_ref, "rm_epsilon(union_list(n-best))", check_props=True)
    got = to_device(dict(no_eps, props=no_eps["props"] | ACYCLIC), gpu_ctx).optimize()
    exp = optimize_ref(dict(no_eps_ref, props=no_eps_ref["props"] | ACYCLIC), oracle)
    assert exp["n_states"] < union_flat["n_states"]
    assert_flat_identical(norm(got.to_flat()), norm(exp), "optimize(rm_epsilon(union_list(n-best)))", check_props=True)


@pytest.mark.gpu
def test_ko_messages_and_the_context_afterwards(gpu_ctx):
    import rustfst_amd
    from rustfst_amd import _lib
    L = _lib.lib()
    a, b = dev(string3(), gpu_ctx), dev(string3(1.5), gpu_ctx)
    out = C.c_void_p()
    def raw(f):
        return f._h.value if isinstance(f._h, C.c_void_p) else f._h
    arr = (C.c_void_p * 3)(raw(a), None, raw(b))
    for fn in (L.wfst_union_list, L.wfst_concat_list):
        assert "item 1: null FST in list" in ko_message(fn(gpu_ctx._h, arr, 3, C.byref(out)))
        assert out.value is None
    other = rustfst_amd.Context(0)
    foreign = dev(string3(), other)
    for call in (lambda: a.union(foreign), lambda: a.concat(foreign), lambda: rustfst_amd.union_list([a, b, foreign]),
                 lambda: rustfst_amd.concat_list([a, foreign])):
        with pytest.raises(rustfst_amd.WfstError, match="belongs to another context"):
            call()
    with pytest.raises(rustfst_amd.WfstError, match="closure_type"):
        check = _lib.check
        check(L.wfst_closure(gpu_ctx._h, a._h, 7, C.byref(out)))
    assert "result too large" in ko_message(_check_sizes(L, 0, [MAX_STATES, 1], [1, 1]))
    # ... and the same context, the same handles, a successful call
    exp = fst_to_flat(union_ref(string3(), string3(1.5)))
    assert_flat_identical(a.union(b).to_flat(), exp, "union after the KOs", check_props=True)
    assert_flat_identical(foreign.union(dev(string3(1.5), other)).to_flat(), exp, "union on the other context", check_props=True)


@pytest.mark.gpu
def test_vector_fst_and_module_surface(gpu_ctx):
    """rustfst-python's test_union / test_concat_fst: in place, returns self, == the expected machine"""
    import rustfst_amd
    g = golden()
    cases = {c["name"]: c for c in g["cases"]}
    for name, method, fn in (("reference_test_union", "union", rustfst_amd.union),
                             ("reference_test_concat_fst", "concat", rustfst_amd.concat)):
        c = cases[name]
        m1, m2 = (golden_fst(g["machines"][a]) for a in c["args"])
        expected = _vector_fst(golden_fst(c["expected"]))
        f1, f2, f2_copy = _vector_fst(m1), _vector_fst(m2), _vector_fst(m2)
        assert getattr(f1, method)(f2) is f1
        assert f1 == expected and f2 == f2_copy
        g1 = _vector_fst(m1)
        assert fn(g1, f2) is g1 and g1 == expected
        lst = (rustfst_amd.union_list if method == "union" else rustfst_amd.concat_list)([_vector_fst(m1), f2])
        assert isinstance(lst, rustfst_amd.VectorFst) and lst == expected
    c = cases["closure_star_two_finals"]
    f = _vector_fst(golden_fst(g["machines"]["two_finals"]))
    assert f.closure(rustfst_amd.ClosureType.CLOSURE_STAR) is f and f == _vector_fst(golden_fst(c["expected"]))
    f = _vector_fst(golden_fst(g["machines"]["two_finals"]))
    assert rustfst_amd.closure(f, rustfst_amd.ClosureType.CLOSURE_PLUS) is f
    assert f == _vector_fst(golden_fst(cases["closure_plus_two_finals"]["expected"]))
    # rustfst-python's test_union_list / test_concat_list: three empty FSTs
    for fn in (rustfst_amd.union_list, rustfst_amd.concat_list):
        assert fn([rustfst_amd.VectorFst(), rustfst_amd.VectorFst(), rustfst_amd.VectorFst()]).num_states() == 0
