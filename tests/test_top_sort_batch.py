"""wfst_top_sort_batch / wfst_ctx_get_top_sort_batch_counters: the C-ABI and Python surface without a GPU, the search of
csrc/top_sort_dfs.h as a stand-alone program under the address and undefined-behaviour sanitizers against
oracle.model's dfs_top_order, a host predictor of the in_kernel flag with one input on each side of every limit; and on the
device parity of every batch item with oracle.model's top_sort_ref AND with top_sort() on the same handle, bit for bit
including the property word, the flags against the predictor, the counters against the list, untouched inputs and the KOs.

Shapes, and why: rows without arcs, a grey target at depth 1, a cycle that only a later root finds; a diamond whose
depth-first order is not its Kahn order, with the arcs of state 0 both ways round; a chain of 4096 states (the stack as deep
as the rule allows) and of 4097 (the single call); 16384 arcs (cursors and offsets at the top of what the kernel keeps in 16
bits) and 16385; one row of 300 arcs walked by one cursor; 300 items are more workgroups than one wave of blocks holds."""
import ctypes as C
import functools
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import model
from oracle.model import (ACYCLIC, CYCLIC, INITIAL_ACYCLIC, NOT_TOP_SORTED, TOP_SORTED, dfs_top_order, fold_ref,
                          fst_to_flat, top_sort_ref, union_ref)
import helpers
from helpers import ROOT, assert_flat_identical, dev, golden_fst, make_fst
from inputs import random_shuffled_dag, top_sort_golden

MAX_STATES, MAX_ARCS = 4096, 16384  # include/wfst.h: the in_kernel rule
SIGNATURES = {
    "wfst_top_sort_batch": "wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, wfst_fst** outs, uint8_t* in_kernel",
    "wfst_ctx_get_top_sort_batch_counters": "wfst_ctx* ctx, uint64_t* launches, uint64_t* items_in_kernel, uint64_t* items_single",
}
TSD_ACYCLIC, TSD_CYCLIC, TSD_STEPS = 0, 1, 2  # csrc/top_sort_dfs.h


def predict_in_kernel(m):
    """wfst.h: a start state, at most 4096 states and at most 16384 arcs; an item with neither states nor a start state
    counts as in the kernel; states without a start state are the single call's (its KO)"""
    n, e = len(m["rows"]), sum(len(r) for r in m["rows"])
    if m["start"] is None:
        return int(n == 0)
    return int(n <= MAX_STATES and e <= MAX_ARCS)


def same(got, exp, what):
    assert_flat_identical(got, exp, what, check_props=True)


# ---------------------------------------------------------------- inputs
def k19_machines():
    g = top_sort_golden()
    return [("k19 " + name, golden_fst(m)) for name, m in g["machines"].items()]


@functools.lru_cache(maxsize=None)
def random_dags():
    """random_dag, 40 seeds, n in 1..40; every other one under the word its content gives"""
    out = []
    for seed in range(40):
        rng = np.random.default_rng(2100 + seed)
        m = random_shuffled_dag(rng, 1 + seed)
        if seed % 2:
            m["props"] = model.content_word(m)
        out.append(("dag %d" % seed, m))
    return out


def tiny_shapes():
    skew = [[[1, 1, 0.5, 1], [2, 2, 0.25, 2]], [[3, 3, 0.0, 3]], [[4, 4, 1.0, 1]], []]     # 0->1, 0->2, 2->1, 1->3
    diamond = [[[1, 1, 0.5, 1], [2, 2, 0.25, 2]], [[3, 3, 0.0, 3]], [[4, 4, 1.0, 3]], []]  # 0->1, 0->2, 1->3, 2->3
    fin = [None, None, None, 0.75]

    def flipped(rows):
        return [list(reversed(rows[0]))] + rows[1:]
    return [("one state, no arc", make_fst([[]], [0.5], 0)),
            ("one state, a self loop", make_fst([[[1, 1, 0.0, 0]]], [0.0], 0)),
            ("a cycle the start cannot reach", make_fst([[[1, 1, 0.0, 1]], [[2, 2, 0.0, 0]], []], [None, None, 0.0], 2)),
            ("skew diamond, 0->1 first", make_fst(skew, fin, 0)),
            ("skew diamond, 0->2 first", make_fst(flipped(skew), fin, 0)),
            ("diamond, 0->1 first", make_fst(diamond, fin, 0)),
            ("diamond, 0->2 first", make_fst(flipped(diamond), fin, 0))]


def chain_of(n):
    """n states in a row, numbered against the order so that every state moves; the start is the last id"""
    rows = [[[1 + s % 5, 1 + s % 3, (s % 8) / 4, s - 1]] if s else [] for s in range(n)]
    return make_fst(rows, [0.0] + [None] * (n - 1), n - 1)


def block_of_arcs(total, per_state=128):
    """`total` arcs, per_state to a state, all into one sink (state 0); the arcs beyond whole states go to the last one"""
    k = total // per_state
    rows = [[]] + [[[1 + j, 1 + s, (j % 7) / 2, 0] for j in range(per_state)] for s in range(k)]
    rows[-1] += [[900 + j, 1, 0.0, 0] for j in range(total - k * per_state)]
    return make_fst(rows, [0.25] + [None] * k, k)


def wide_row():
    """one state with 300 arcs, many to the same target, finals on every state"""
    rows = [[[1 + j % 50, 2, (j % 11) / 4, 1 + (j * 7) % 5] for j in range(300)], [[3, 3, 0.5, 3]], [], [], [[4, 4, 0.0, 5]], []]
    return make_fst(rows, [s / 4 for s in range(6)], 0)


@functools.lru_cache(maxsize=None)
def limit_families():
    """(name, FST): one input on each side of every limit"""
    return [("states 4096", chain_of(MAX_STATES)), ("states 4097", chain_of(MAX_STATES + 1)),
            ("arcs 16384", block_of_arcs(MAX_ARCS)), ("arcs 16385", block_of_arcs(MAX_ARCS + 1))]


@functools.lru_cache(maxsize=None)
def many_small(count=300):
    out = []
    for k in range(count):
        rng = np.random.default_rng(3000 + k)
        out.append(("small %d" % k, random_shuffled_dag(rng, 2 + k % 19)))
    return out


def with_cycle(m, rng):
    """m with one arc against its order and one along it"""
    m = dict(m, rows=[[list(t) for t in r] for r in m["rows"]])
    n = len(m["rows"])
    a, b = (int(x) for x in rng.choice(n, 2, replace=False))
    _, order = dfs_top_order(m)
    lo, hi = (a, b) if order[a] < order[b] else (b, a)
    m["rows"][hi].append([1, 1, 0.0, lo])
    m["rows"][lo].append([2, 2, 0.0, hi])
    return m


@functools.lru_cache(maxsize=None)
def mixed_list():
    """many_small with every third item cyclic and the two items beyond the limits in the middle"""
    rng = np.random.default_rng(3999)
    items = [(name + " cyclic", with_cycle(m, rng)) if k % 3 == 0 else (name, m) for k, (name, m) in enumerate(many_small())]
    fams = dict(limit_families())
    return items[:100] + [("states 4097", fams["states 4097"])] + items[100:200] + [("arcs 16385", fams["arcs 16385"])] + items[200:]


_REF = {}


def reference(name, m):
    """top_sort_ref's answer as flat arrays, computed once per item and left unchanged"""
    if name not in _REF:
        _REF[name] = fst_to_flat(top_sort_ref(m))
    return _REF[name]


# ================================================================ no GPU
def test_new_symbols_declared_exported_and_bound(wfst_lib):
    from rustfst_amd import _lib
    with open(os.path.join(ROOT, "include", "wfst.h")) as f:
        header = f.read()
    vp, u64 = C.c_void_p, C.POINTER(C.c_uint64)
    args = {"wfst_top_sort_batch": [vp, C.POINTER(vp), C.c_size_t, C.POINTER(vp), vp],
            "wfst_ctx_get_top_sort_batch_counters": [vp, u64, u64, u64]}
    bound = {name: a for name, _, a in _lib.SYMBOLS}
    for name, want in SIGNATURES.items():
        assert helpers.header_params(header, name) == want, name
        assert bound[name] == args[name] and hasattr(wfst_lib, name), name
    assert _lib.TOP_SORT_BATCH_COUNTERS == _lib._BATCH == ("launches", "items_in_kernel", "items_single")
    m = re.search(r"#define\s+WFST_ABI_VERSION\s+7\b(.*)", header)
    assert m and all(name in m.group(1).split("; 6:")[0] for name in SIGNATURES) and wfst_lib.wfst_abi_version() == 7
    text = header[header.index("top_sort of n FSTs in one call"):header.index("wfst_status wfst_top_sort_batch")]
    assert "4096 states" in text and "16384 arcs" in text and "start state" in text and "occupies no workgroup" in text


def test_argument_validation_without_gpu(wfst_lib):
    ko = helpers.ko_message
    fn = wfst_lib.wfst_top_sort_batch
    outs = (C.c_void_p * 3)(1, 1, 1)
    fsts = (C.c_void_p * 3)()
    assert fn(None, None, 0, None, None) == 0  # n == 0: OK
    assert "null" in ko(fn(None, fsts, 3, outs, None))  # NULL ctx
    assert [outs[i] for i in range(3)] == [None] * 3
    assert "null" in ko(fn(None, fsts, 3, None, None))  # NULL outs
    outs = (C.c_void_p * 3)(1, 1, 1)
    assert "null" in ko(fn(None, None, 3, outs, None))  # NULL fsts with n > 0
    assert [outs[i] for i in range(3)] == [None] * 3
    assert "null" in ko(wfst_lib.wfst_ctx_get_top_sort_batch_counters(None, None, None, None))
    # a NULL entry is reported with its index before anything else is done with the context: no context can be made
    # without a device, so this one is zeroed memory, and the call may do no more with it than clear its counters
    ctx = C.create_string_buffer(1 << 20)
    outs = (C.c_void_p * 3)(1, 1, 1)
    assert ko(fn(C.cast(ctx, C.c_void_p), fsts, 3, outs, None)) == "item 0: null FST in batch"
    assert [outs[i] for i in range(3)] == [None] * 3 and ctx.raw == bytes(1 << 20)


def test_python_surface():
    import rustfst_amd
    for name in ("top_sort_batch", "top_sort_batch_stats"):
        assert name in rustfst_amd.__all__ and callable(getattr(rustfst_amd, name))
    p = inspect.signature(rustfst_amd.top_sort_batch).parameters
    assert list(p) == ["fsts", "ctx", "return_in_kernel"]
    assert p["ctx"].default is None and p["return_in_kernel"].default is False
    assert rustfst_amd.top_sort_batch([]) == []
    res, flags = rustfst_amd.top_sort_batch([], return_in_kernel=True)
    assert res == [] and flags.dtype == np.uint8 and len(flags) == 0
    p = inspect.signature(rustfst_amd.top_sort_batch_stats).parameters
    assert list(p) == ["ctx"] and p["ctx"].default is None
    with open(os.path.join(ROOT, "include", "wfst.hpp")) as f:
        assert re.search(r"\btop_sort_batch\(std::vector<VectorFst>&", f.read())


def test_predictor_on_both_sides_of_every_limit():
    fams = dict(limit_families())
    sizes = {name: (len(m["rows"]), sum(len(r) for r in m["rows"])) for name, m in fams.items()}
    assert sizes["states 4096"][0] == MAX_STATES and sizes["states 4097"][0] == MAX_STATES + 1
    assert sizes["arcs 16384"][1] == MAX_ARCS and sizes["arcs 16385"][1] == MAX_ARCS + 1
    assert all(e <= MAX_ARCS for _, e in (sizes["states 4096"], sizes["states 4097"]))  # (only the states decide these two)
    assert all(n <= MAX_STATES for n, _ in (sizes["arcs 16384"], sizes["arcs 16385"]))  # (only the arcs decide these two)
    assert [predict_in_kernel(fams[k]) for k in ("states 4096", "states 4097", "arcs 16384", "arcs 16385")] == [1, 0, 1, 0]
    # the start state: without states in the kernel's count, with states the single call's
    assert predict_in_kernel(make_fst([], [], None)) == 1
    assert predict_in_kernel(make_fst([[]], [0.0], None)) == 0 and predict_in_kernel(make_fst([[]], [0.0], 0)) == 1
    assert all(predict_in_kernel(m) for _, m in many_small() + random_dags() + tiny_shapes())
    assert [predict_in_kernel(m) for _, m in mixed_list()].count(0) == 2
    cyc = [dfs_top_order(m)[0] for _, m in mixed_list()]
    assert cyc.count(False) == 100


def dfs_case(m):
    """one case of top_sort_dfs_check's stdin, and the line it has to print"""
    n = len(m["rows"])
    off = np.concatenate([[0], np.cumsum([len(r) for r in m["rows"]])]).astype(int).tolist()
    words = [n, m["start"]] + off + [t[3] for r in m["rows"] for t in r]
    acyclic, order = dfs_top_order(m)
    want = [TSD_ACYCLIC] + order if acyclic else [TSD_CYCLIC] + list(range(n))
    return " ".join(str(w) for w in words), " ".join(str(w) for w in want)


def test_search_header_against_the_restatement(tmp_path):
    """csrc/top_sort_dfs.h — what one lane of top_sort_batch_kernel runs — in a stand-alone program on heap arrays of exactly
    the documented sizes, under the address and undefined-behaviour sanitizers: every K19 machine that has a start state (the
    others never reach the search), the 40 random DAGs, the small and the limit shapes that stay in the kernel and the 300
    items of the mixed list; then the step bound, reached by passing a smaller one."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "top_sort_dfs_check"
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "rustfst_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "top_sort_dfs_check.cpp")])
    items = [x for x in k19_machines() if x[1]["start"] is not None] + random_dags() + tiny_shapes()
    items += [x for x in limit_families() if predict_in_kernel(x[1])] + [("wide row", wide_row())]
    items += [x for x in mixed_list() if predict_in_kernel(x[1])]
    assert len(items) > 350 and all(predict_in_kernel(m) for _, m in items)
    cases = [dfs_case(m) for _, m in items]
    out = subprocess.run([str(exe)], input="%d\n%s\n" % (len(cases), "\n".join(c for c, _ in cases)), capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(cases)
    for (name, _), (_, want), got in zip(items, cases, lines):
        assert got == want, name
    assert sum(1 for _, w in cases if w.startswith("1")) >= 100  # (the cyclic exit was among them)
    # a chain of 10 states takes 20 steps: 10 pushes, 10 pops
    chain, want = dfs_case(chain_of(10))
    for bound, line in ((20, want), (10, str(TSD_STEPS)), (0, str(TSD_STEPS))):
        out = subprocess.run([str(exe), str(bound)], input="1\n" + chain + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        assert out.stdout.strip() == line, bound


# ================================================================ GPU
def _stats(ctx):
    import rustfst_amd
    return rustfst_amd.top_sort_batch_stats(ctx)


def check_list(items, ctx, launches=None):
    """one batch call; every result against the restatement and the single call on the same handle, the flags against the
    predictor, the counters against the list, the inputs unchanged.  Returns (results, handles)."""
    import rustfst_amd
    devs = [dev(m, ctx) for _, m in items]
    outs, flags = rustfst_amd.top_sort_batch(devs, ctx, return_in_kernel=True)
    st = _stats(ctx)
    got = [o.to_flat() for o in outs]
    want = [predict_in_kernel(m) for _, m in items]
    print("flags %s\nstats %s" % ([int(x) for x in flags], st))
    assert [int(x) for x in flags] == want
    occupied = sum(1 for (_, m), w in zip(items, want) if w and m["rows"])
    assert st == dict(launches=(1 if occupied else 0) if launches is None else launches, items_in_kernel=sum(want),
                      items_single=len(want) - sum(want))
    for k, ((name, m), g) in enumerate(zip(items, got)):
        same(g, reference(name, m), f"item {k} ({name}) vs the restatement")
        same(g, devs[k].top_sort().to_flat(), f"item {k} ({name}) vs the single call")
        same(devs[k].to_flat(), fst_to_flat(m), f"item {k} ({name}): the input after the calls")
    return got, devs


@pytest.mark.gpu
def test_k19_machines_in_one_list(gpu_ctx):
    items = [x for x in k19_machines() if x[0] != "k19 two_states_no_start"]
    got, _ = check_list(items, gpu_ctx)
    g = top_sort_golden()
    by = dict(zip((name for name, _ in items), got))
    for c in g["cases"]:
        if c["op"] == "top_sort" and "error" not in c:
            same(by["k19 " + c["arg"]], fst_to_flat(golden_fst(c["expected"])), c["name"])
    assert by["k19 no_states"]["n_states"] == 0


@pytest.mark.gpu
def test_random_dags_in_one_list(gpu_ctx):
    items = random_dags()
    got, _ = check_list(items, gpu_ctx)
    bits = ACYCLIC | INITIAL_ACYCLIC | TOP_SORTED
    for (name, m), g in zip(items, got):
        assert g["props"] & bits == bits and g["start"] == dfs_top_order(m)[1][m["start"]], name
        assert np.all(g["arcs"]["nextstate"] > np.repeat(np.arange(g["n_states"]), np.diff(g["offsets"].astype(np.int64)))), name


@pytest.mark.gpu
def test_small_shapes_and_the_order_of_the_search(gpu_ctx):
    items = tiny_shapes() + [("wide row", wide_row())]
    got, _ = check_list(items, gpu_ctx)
    by = dict(zip((name for name, _ in items), got))
    for name in ("one state, a self loop", "a cycle the start cannot reach"):
        assert by[name]["props"] & (CYCLIC | NOT_TOP_SORTED) == CYCLIC | NOT_TOP_SORTED, name
    # the order is the search's, not the levels': the diamond's levels are {0}, {1, 2}, {3} whichever arc of state 0 is
    # stored first, but the search numbers last the branch it takes first; the skew diamond has one order either way
    orders = {name: dfs_top_order(m)[1] for name, m in items if "diamond" in name}
    assert orders == {"skew diamond, 0->1 first": [0, 2, 1, 3], "skew diamond, 0->2 first": [0, 2, 1, 3],
                      "diamond, 0->1 first": [0, 2, 1, 3], "diamond, 0->2 first": [0, 1, 2, 3]}
    assert by["diamond, 0->1 first"]["arcs"]["nextstate"].tolist() == [2, 1, 3, 3]
    assert by["diamond, 0->2 first"]["arcs"]["nextstate"].tolist() == [2, 1, 3, 3]
    assert by["diamond, 0->1 first"]["arcs"]["ilabel"].tolist() == [1, 2, 4, 3]
    assert by["diamond, 0->2 first"]["arcs"]["ilabel"].tolist() == [2, 1, 3, 4]
    assert np.all(by["wide row"]["finals"] != np.inf) and int(np.diff(by["wide row"]["offsets"].astype(np.int64)).max()) == 300


@pytest.mark.gpu
def test_both_sides_of_every_limit(gpu_ctx):
    fams = limit_families()
    got, _ = check_list(fams, gpu_ctx, launches=1)
    assert _stats(gpu_ctx) == dict(launches=1, items_in_kernel=2, items_single=2)  # (the single calls since left it alone)
    by = dict(zip((name for name, _ in fams), got))
    assert by["states 4096"]["start"] == 0 and by["states 4096"]["arcs"]["nextstate"].tolist() == list(range(1, MAX_STATES))


@pytest.mark.gpu
def test_list_of_300_items(gpu_ctx):
    got, _ = check_list(many_small(), gpu_ctx, launches=1)
    assert len(got) == 300 and _stats(gpu_ctx) == dict(launches=1, items_in_kernel=300, items_single=0)


@pytest.mark.gpu
def test_list_of_300_items_with_cyclic_and_oversized_ones(gpu_ctx):
    items = mixed_list()
    got, _ = check_list(items, gpu_ctx, launches=1)
    assert _stats(gpu_ctx) == dict(launches=1, items_in_kernel=300, items_single=2)
    cyclic = [bool(g["props"] & CYCLIC) for g in got]
    assert cyclic.count(True) == 100 and all(c == (" cyclic" in name) for c, (name, _) in zip(cyclic, items))


@pytest.mark.gpu
def test_lists_of_one_of_none_and_of_empty_fsts(gpu_ctx):
    import rustfst_amd
    check_list(random_dags()[7:8], gpu_ctx, launches=1)
    from rustfst_amd import _lib
    assert rustfst_amd.top_sort_batch([], gpu_ctx) == []  # (the Python side answers an empty list itself)
    assert _lib.lib().wfst_top_sort_batch(gpu_ctx._h, None, 0, None, None) == 0
    assert _stats(gpu_ctx) == dict(launches=0, items_in_kernel=0, items_single=0)
    empty = make_fst([], [], None, model.ACCEPTOR)
    got, _ = check_list([("empty a", empty), ("empty b", dict(empty, props=0)), ("empty c", empty)], gpu_ctx, launches=0)
    assert all(g["n_states"] == 0 and g["props"] & TOP_SORTED for g in got)
    # the same handle twice, and an item between the two
    devs = [dev(m, gpu_ctx) for _, m in random_dags()[20:22]]
    outs = rustfst_amd.top_sort_batch([devs[0], devs[1], devs[0]], gpu_ctx)
    for o, k in zip(outs, (20, 21, 20)):
        same(o.to_flat(), reference(*random_dags()[k]), "the same handle twice")
    assert _stats(gpu_ctx) == dict(launches=1, items_in_kernel=3, items_single=0)


@pytest.mark.gpu
def test_getter_pointer_by_pointer(gpu_ctx):
    """any pointer after ctx may be NULL, and each one alone receives the counter of its position"""
    from rustfst_amd import _lib
    check_list(mixed_list()[95:105], gpu_ctx, launches=1)  # 9 items in the kernel, one beyond the limits
    full = _stats(gpu_ctx)
    assert full == dict(launches=1, items_in_kernel=9, items_single=1)
    fn, names, sentinel = _lib.lib().wfst_ctx_get_top_sort_batch_counters, _lib.TOP_SORT_BATCH_COUNTERS, 0xA5A5A5A5A5A5A5A5
    assert fn(gpu_ctx._h, None, None, None) == 0
    for i, name in enumerate(names):
        vals = [C.c_uint64(sentinel) for _ in names]
        assert fn(gpu_ctx._h, *[C.byref(v) if k == i else None for k, v in enumerate(vals)]) == 0
        assert [v.value for v in vals] == [full[name] if k == i else sentinel for k in range(len(names))], name


@pytest.mark.gpu
def test_counters_of_the_single_call_describe_the_last_single_call(gpu_ctx):
    """wfst_ctx_get_top_sort_stats: a batch without a fallback item leaves it alone, one with such an item leaves that item's"""
    import rustfst_amd
    small = dev(random_dags()[30][1], gpu_ctx)
    small.top_sort()
    before = gpu_ctx.top_sort_stats()
    assert before["levels"] > 0
    rustfst_amd.top_sort_batch([small, small], gpu_ctx)
    assert gpu_ctx.top_sort_stats() == before
    big = dev(dict(limit_families())["states 4097"], gpu_ctx)
    rustfst_amd.top_sort_batch([small, big], gpu_ctx)
    assert gpu_ctx.top_sort_stats()["levels"] == MAX_STATES + 1
    assert _stats(gpu_ctx) == dict(launches=1, items_in_kernel=1, items_single=1)


@pytest.mark.gpu
def test_no_start_state_is_the_loops_ko_and_the_context_works_afterwards(gpu_ctx):
    import rustfst_amd
    from rustfst_amd import _lib
    items = [m for _, m in random_dags()[10:18]]
    items[3] = dict(items[3], start=None)
    items[7] = dict(items[7], start=None)
    n3 = len(items[3]["rows"])
    assert n3 > 0 and len(items[7]["rows"]) not in (0, n3)
    devs = [dev(m, gpu_ctx) for m in items]
    arr = (C.c_void_p * 8)(*[d._h.value for d in devs])
    outs = (C.c_void_p * 8)(*[1] * 8)
    flags = (C.c_uint8 * 8)(*[9] * 8)
    status = _lib.lib().wfst_top_sort_batch(gpu_ctx._h, arr, 8, outs, flags)
    assert helpers.ko_message(status) == "item 3: StateSort : Bad order vector size : 0. Expected %d" % n3
    assert [outs[i] for i in range(8)] == [None] * 8
    with pytest.raises(rustfst_amd.WfstError, match=re.escape("item 3: StateSort : Bad order vector size : 0. Expected %d" % n3)):
        rustfst_amd.top_sort_batch(devs, gpu_ctx)
    with pytest.raises(rustfst_amd.WfstError, match=re.escape("StateSort : Bad order vector size : 0. Expected %d" % n3)):
        devs[3].top_sort()  # the loop's message, without the index
    check_list(random_dags()[10:18], gpu_ctx, launches=1)


@pytest.mark.gpu
def test_foreign_handle_is_ko_before_any_launch(gpu_ctx):
    import rustfst_amd
    from rustfst_amd import _lib
    items = random_dags()[2:6]
    devs = [dev(m, gpu_ctx) for _, m in items]
    other = rustfst_amd.Context(0)
    foreign = dev(items[1][1], other)
    hs = [d._h.value for d in devs]
    for handles, text in ((hs[:1] + [foreign._h.value] + hs[2:], "item 1: top_sort_batch: the FST belongs to another context"),
                          (hs[:3] + [None], "item 3: null FST in batch")):
        arr = (C.c_void_p * 4)(*handles)
        outs = (C.c_void_p * 4)(1, 1, 1, 1)
        status = _lib.lib().wfst_top_sort_batch(gpu_ctx._h, arr, 4, outs, None)
        assert helpers.ko_message(status) == text
        assert [outs[i] for i in range(4)] == [None] * 4
        assert _stats(gpu_ctx) == dict(launches=0, items_in_kernel=0, items_single=0)
    del foreign
    check_list(items, gpu_ctx, launches=1)
    assert _lib.lib().wfst_top_sort_batch(gpu_ctx._h, None, 0, None, None) == 0
    assert _stats(gpu_ctx) == dict(launches=0, items_in_kernel=0, items_single=0)


@pytest.mark.gpu
def test_unions_of_nbest_paths_top_sort_batch_then_optimize_batch(gpu_ctx):
    """the recipe of INTEGRATION.md end to end: union_list of n-best strings (its word holds neither ACYCLIC nor TOP_SORTED,
    and optimize_batch answers KO) -> top_sort_batch -> optimize_batch, equal item by item to top_sort then optimize"""
    import rustfst_amd
    rng = np.random.default_rng(2206)
    word = model.ACCEPTOR | ACYCLIC | INITIAL_ACYCLIC | model.ACCESSIBLE | model.COACCESSIBLE
    unions, refs = [], []
    for _ in range(6):
        strings = []
        for k in range(int(rng.integers(2, 6))):
            labels = [int(x) for x in rng.integers(1, 4, size=int(rng.integers(1, 7)))]
            rows = [[[x, x, float(rng.integers(0, 9)) / 4 if i == 0 else 0.0, i + 1]] for i, x in enumerate(labels)] + [[]]
            strings.append(make_fst(rows, [None] * len(labels) + [0.0], 0, word))
        unions.append(rustfst_amd.union_list([dev(s, gpu_ctx) for s in strings]))
        refs.append(fold_ref(union_ref, strings))
    with pytest.raises(rustfst_amd.WfstError, match="does not hold ACYCLIC"):
        rustfst_amd.optimize_batch(unions, gpu_ctx)
    sorted_devs, flags = rustfst_amd.top_sort_batch(unions, gpu_ctx, return_in_kernel=True)
    assert flags.tolist() == [1] * 6 and _stats(gpu_ctx) == dict(launches=1, items_in_kernel=6, items_single=0)
    for k, (s, u, r) in enumerate(zip(sorted_devs, unions, refs)):
        same(s.to_flat(), fst_to_flat(top_sort_ref(r)), f"top_sort_batch(union {k}) vs the restatement")
        same(s.to_flat(), u.top_sort().to_flat(), f"top_sort_batch(union {k}) vs the single call")
    optimized = rustfst_amd.optimize_batch(sorted_devs, gpu_ctx)
    for k, (o, u) in enumerate(zip(optimized, unions)):
        same(o.to_flat(), u.top_sort().optimize().to_flat(), f"optimize_batch(top_sort_batch(union {k}))")
        assert o.to_flat()["n_states"] <= u.to_flat()["n_states"]
