"""wfst_rm_epsilon_batch: the C-ABI and Python surface without a GPU, a predictor of the in_kernel flag built from
test_rm_epsilon's restatement (the needs of every rewritten state and a cycle check of the epsilon graph) with one input
family on each side of every limit of the rule; and on the device parity of every batch item with the oracle AND with the
single call on the same handle, bit for bit including the property word, the flags against the prediction, arena growth,
launch counts that depend neither on the list's length nor on the epsilon depth, untouched inputs, every KO, and the chain
rm_epsilon_batch -> determinize_batch -> minimize_batch against the loop of single calls.

Weights are on the 1/512 grid, where the exact minimum the kernels compute is the reference's distance (test_rm_epsilon)."""
import ctypes as C
import functools
import inspect
import json
import os
import re

import numpy as np
import pytest

from rustfst_amd._lib import TR_DTYPE
from oracle.model import (ACCEPTOR, ACCESSIBLE, ACYCLIC, COACCESSIBLE, INITIAL_ACYCLIC, fold_ref, fst_to_flat,
                          union_ref)
import helpers
from helpers import (assert_flat_identical, empty_flat, enumerate_paths, make_fst, random_fst_flat, to_device,
                     to_oracle)
import determinize_cases as dc
import minimize_cases as mc
import rm_epsilon_cases as rc
from rm_epsilon_cases import Builder, chain, fan, par, rm_epsilon_model, wide

ROOT = helpers.ROOT
INF = np.float32(np.inf)
MAX_STATES, MAX_ARCS = 4096, 16384  # include/wfst.h: the in_kernel rule of wfst_rm_epsilon_batch
CAPS = rc.THREAD_RUNGS[-1]         # ... and the last rung of the single call's one-thread kernel
NEW_SYMBOLS = ("wfst_rm_epsilon_batch", "wfst_ctx_get_rm_epsilon_batch_stats")


def has_start(flat):
    return flat["start"] is not None and flat["start"] >= 0


def item_needs(flat):
    """{rewritten state: (closure, stack, arcs)}, or None when the epsilon graph has a cycle"""
    try:
        return rm_epsilon_model(flat)[1]
    except ValueError:
        return None


def predict_in_kernel(flat):
    """wfst.h: an item without a start state or without states counts as in the kernel; otherwise at most 4096 states and
    16384 arcs, no epsilon cycle, and every rewritten state within (64, 128, 128)"""
    if not has_start(flat) or flat["n_states"] == 0:
        return 1
    if flat["n_states"] > MAX_STATES or len(flat["arcs"]) > MAX_ARCS:
        return 0
    needs = item_needs(flat)
    return int(needs is not None and all(x <= c for need in needs.values() for x, c in zip(need, CAPS)))


def same(got, exp, what):
    assert_flat_identical(got, exp, what, check_props=True)


# ---------------------------------------------------------------- inputs
def long_chain(n):
    """n states in a row, every fourth arc epsilon:epsilon, the others labelled: closures of two states"""
    b = Builder()
    states = [b.state() for _ in range(n - 1)] + [b.state(final=256)]
    for i in range(n - 1):
        if i % 4 == 3:
            b.eps(states[i], 1 + i % 3, states[i + 1])
        else:
            b.arc(states[i], 1 + i % 5, 1 + i % 7, (i * 13) % 97, states[i + 1])
    return b.flat()


def many_arcs(total, n=160):
    """`total` arcs over a row of n states: parallel arcs with distinct labels into the next state, and one epsilon arc
    into the final state at the end (so that no rewritten state gains arcs)"""
    b = Builder()
    states = [b.state() for _ in range(n - 1)] + [b.state(final=256)]
    b.eps(states[n - 2], 3, states[n - 1])
    for j in range(total - 1):
        s = j % (n - 1)
        b.arc(states[s], 1 + j // (n - 1), 1 + j // (n - 1), (j * 13) % 97, states[s + 1])
    f = b.flat()
    assert len(f["arcs"]) == total and f["n_states"] == n
    return f


def two_cycle():
    """an epsilon 2-cycle without a self loop"""
    b = Builder()
    hub, a, c, sink = b.state(), b.state(), b.state(final=9), b.state(final=256)
    b.arc(hub, 1, 1, 1, a)
    b.eps(a, 2, c)
    b.eps(c, 3, a)
    b.arc(a, 3, 3, 7, sink)
    b.arc(c, 4, 4, 8, sink)
    return b.flat()


def hung_chain(length):
    """an epsilon chain of `length` arcs whose every state has a labelled arc from a hub (so every depth is rewritten) and
    the SAME labelled arc into the sink (combined at the first occurrence: no rewritten state gains an arc)"""
    b = Builder()
    hub = b.state()
    states = [b.state() for _ in range(length + 1)]
    sink = b.state(final=256)
    for i, s in enumerate(states):
        b.arc(hub, 10 + i, 10 + i, i % 7, s)
        b.arc(s, 4, 5, 77 + i % 3, sink)
        if i < length:
            b.eps(s, 1 + i % 3, states[i + 1])
    return b.flat()


# (name, flat, expected flag, the check of the edge on the needs of the start state / the sizes)
@functools.lru_cache(maxsize=None)
def limit_families():
    def start_need(f):
        return item_needs(f)[0]
    out = [("states 4096", long_chain(MAX_STATES), 1), ("states 4097", long_chain(MAX_STATES + 1), 0),
           ("arcs 16384", many_arcs(MAX_ARCS), 1), ("arcs 16385", many_arcs(MAX_ARCS + 1), 0),
           ("closure 64 (fan)", fan(63), 1), ("closure 65 (fan)", fan(64), 0),
           ("closure 64 (chain)", chain(63), 1), ("closure 65 (chain)", chain(64), 0),
           ("stack 128", par(128), 1), ("stack 129", par(129), 0),
           ("arcs of a state 128", wide(128), 1), ("arcs of a state 129", wide(129), 0),
           ("self loop", rc.value_cases()["self_loop"][0], 0), ("two-cycle", two_cycle(), 0)]
    edges = {"closure 64 (fan)": (64, 63, 63), "closure 65 (fan)": (65, 64, 64), "closure 64 (chain)": (64, 1, 1),
             "closure 65 (chain)": (65, 1, 1), "stack 128": (2, 128, 1), "stack 129": (2, 129, 1),
             "arcs of a state 128": (2, 1, 128), "arcs of a state 129": (2, 1, 129)}
    for name, f, _ in out:
        if name in edges:
            assert start_need(f) == edges[name], name
    return out


def k11_flat():
    with open(os.path.join(ROOT, "tests", "golden", "k11_rm_epsilon.json")) as fh:
        g = json.load(fh)["fst"]
    rows = [[] for _ in range(g["n_states"])]
    for s, il, ol, w, ns in g["arcs"]:
        rows[s].append((il, ol, w, ns))
    finals = np.full(g["n_states"], np.inf, np.float32)
    for s, w in g["finals"]:
        finals[s] = w
    return dict(n_states=g["n_states"], start=g["start"], offsets=np.cumsum([0] + [len(r) for r in rows]).astype(np.uint32),
                arcs=np.array([t for r in rows for t in r], dtype=TR_DTYPE), finals=finals, props=0)


def nbest_union_flat():
    """test_rational_ops' pipeline: the five best paths of a lattice as strings, their union (epsilon arcs from the start)"""
    rng = np.random.default_rng(1806)
    word = ACCEPTOR | ACYCLIC | INITIAL_ACYCLIC | ACCESSIBLE | COACCESSIBLE
    lattice = mc.random_dag(rng, 12, 4)
    paths = sorted(enumerate_paths(lattice))[:5]
    strings = []
    for w, il, _ in paths:
        il = list(il) or [1]
        rows = [[[x, x, w if i == 0 else 0.0, i + 1]] for i, x in enumerate(il)] + [[]]
        strings.append(make_fst(rows, [None] * len(il) + [0.0], 0, word))
    return fst_to_flat(fold_ref(union_ref, strings))


@functools.lru_cache(maxsize=None)
def parity_items():
    """[(name, flat)]: the mixed batch"""
    rng = np.random.default_rng(2611)
    items = [("k11", k11_flat())]
    for k, p in enumerate((0.1, 0.2, 0.3, 0.4, 0.5) * 3):
        acyclic = k % 3 != 2
        f = random_fst_flat(rng, int(rng.integers(5, 60)), 3, 3, p_eps_i=p, p_eps_o=p, p_final=0.3, acyclic=acyclic,
                            sort=("none", "ilabel")[k % 2])
        if not np.isfinite(f["finals"]).any():
            f["finals"][-1] = 1.0
        if k % 2 == 0:  # an acceptor: its epsilon:epsilon arcs have probability p, a transducer's p * p
            f["arcs"]["olabel"] = f["arcs"]["ilabel"]
        items.append(("random %d p %.1f %s %s" % (k, p, "acyclic" if acyclic else "cyclic", "acceptor" if k % 2 == 0 else "transducer"), f))
    items.append(("union of n-best", nbest_union_flat()))
    items += rc.props_random_inputs()[:6] + rc.props_hand_made()  # words with / without TOP_SORTED and ACCEPTOR
    items.append(("no start", dict(fan(15), start=-1)))
    items.append(("no states", empty_flat(start=-1)))
    items.append(("no arcs", rc.value_cases()["start_without_arcs"][0]))
    b = Builder()
    root, u, v = b.state(), b.state(), b.state()
    b.eps(root, 3, u)
    b.arc(u, 1, 1, 5, v)
    items.append(("trims to nothing", b.flat()))
    f = random_fst_flat(rng, 30, 3, 3, p_final=0.3, acyclic=True)
    f["finals"][-1] = 1.0
    items.append(("no epsilon at all", f))
    items += [(name, flat) for name, (flat, _) in sorted(rc.value_cases().items())]
    return items


_REF = {}


def oracle_rm_epsilon(oracle, name, flat):
    """the oracle's answer, computed once per item and left unchanged"""
    if name not in _REF:
        ref = to_oracle(oracle, flat)
        ref.rm_epsilon()
        _REF[name] = ref.to_flat()
    return _REF[name]


# ================================================================ no GPU
def test_new_symbols_declared_exported_and_bound(wfst_lib):
    from rustfst_amd import _lib
    with open(os.path.join(ROOT, "include", "wfst.h")) as f:
        header = f.read()
    want = {"wfst_rm_epsilon_batch": "wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, wfst_fst** outs, uint8_t* in_kernel",
            "wfst_ctx_get_rm_epsilon_batch_stats": "wfst_ctx* ctx, uint64_t* launches, uint64_t* items_in_kernel, uint64_t* items_single"}
    vp, u64 = C.c_void_p, C.POINTER(C.c_uint64)
    args = {"wfst_rm_epsilon_batch": [vp, C.POINTER(vp), C.c_size_t, C.POINTER(vp), vp],
            "wfst_ctx_get_rm_epsilon_batch_stats": [vp, u64, u64, u64]}
    bound = {name: a for name, _, a in _lib.SYMBOLS}
    for name in NEW_SYMBOLS:
        m = re.search(r"\bwfst_status\s+%s\s*\(([^)]*)\)" % name, header)
        assert m and " ".join(m.group(1).split()) == want[name], name
        assert bound[name] == args[name] and hasattr(wfst_lib, name), name
    assert re.search(r"#define\s+WFST_ABI_VERSION\s+7\b", header) and wfst_lib.wfst_abi_version() == 7
    text = header[header.index("rm_epsilon of n FSTs in one call"):header.index("wfst_status wfst_rm_epsilon_batch")]
    assert "at most 4096 states" in text and "16384 arcs" in text and "64 / 128 / 128" in text
    assert "WFST_RM_EPSILON_BATCH_ARENA" in text and "split the list" in text


def test_argument_validation_without_gpu(wfst_lib):
    ko = helpers.ko_message
    outs = (C.c_void_p * 3)(1, 1, 1)
    fsts = (C.c_void_p * 3)()
    assert wfst_lib.wfst_rm_epsilon_batch(None, None, 0, None, None) == 0  # n == 0: OK
    assert "null" in ko(wfst_lib.wfst_rm_epsilon_batch(None, fsts, 3, outs, None))  # NULL ctx
    assert [outs[i] for i in range(3)] == [None] * 3
    assert "null" in ko(wfst_lib.wfst_rm_epsilon_batch(None, fsts, 3, None, None))  # NULL outs
    outs = (C.c_void_p * 3)(1, 1, 1)
    assert "null" in ko(wfst_lib.wfst_rm_epsilon_batch(None, None, 3, outs, None))  # NULL fsts with n > 0
    assert [outs[i] for i in range(3)] == [None] * 3
    assert "null" in ko(wfst_lib.wfst_ctx_get_rm_epsilon_batch_stats(None, None, None, None))


def test_null_entry_is_ko_before_the_context_is_used(wfst_lib):
    """a NULL entry is reported with its index before anything else is done with the context.  No context can be made
    without a device, so the one here is a block of zeroed memory, as in test_minimize_batch: the call may do no more with
    it, before it has checked the list, than clear its three counters."""
    ctx = C.create_string_buffer(1 << 20)
    outs = (C.c_void_p * 3)(1, 1, 1)
    fsts = (C.c_void_p * 3)()
    msg = helpers.ko_message(wfst_lib.wfst_rm_epsilon_batch(C.cast(ctx, C.c_void_p), fsts, 3, outs, None))
    assert msg == "item 0: null FST in batch" and [outs[i] for i in range(3)] == [None] * 3
    assert ctx.raw == bytes(1 << 20)


def test_python_surface():
    import rustfst_amd
    for name in ("rm_epsilon_batch", "rm_epsilon_batch_stats"):
        assert name in rustfst_amd.__all__ and callable(getattr(rustfst_amd, name))
    p = inspect.signature(rustfst_amd.rm_epsilon_batch).parameters
    assert list(p) == ["fsts", "ctx", "return_in_kernel"]
    assert p["ctx"].default is None and p["return_in_kernel"].default is False
    p = inspect.signature(rustfst_amd.rm_epsilon_batch_stats).parameters
    assert list(p) == ["ctx"] and p["ctx"].default is None
    assert rustfst_amd.rm_epsilon_batch([]) == []
    res, flags = rustfst_amd.rm_epsilon_batch([], return_in_kernel=True)
    assert res == [] and flags.dtype == np.uint8 and len(flags) == 0


def test_limit_families_sit_on_their_edges():
    """every family's needs exactly on its edge (asserted while the families are built), sizes on theirs, and the predictor
    on both sides of every limit"""
    assert CAPS == (64, 128, 128)
    fams = {name: (f, want) for name, f, want in limit_families()}
    assert fams["states 4096"][0]["n_states"] == MAX_STATES and fams["states 4097"][0]["n_states"] == MAX_STATES + 1
    assert len(fams["arcs 16384"][0]["arcs"]) == MAX_ARCS and len(fams["arcs 16385"][0]["arcs"]) == MAX_ARCS + 1
    for name in ("states 4096", "states 4097", "arcs 16384", "arcs 16385"):  # (only the size decides these four)
        needs = item_needs(fams[name][0])
        assert all(x <= c for need in needs.values() for x, c in zip(need, CAPS)), name
        assert len(fams[name][0]["arcs"]) <= MAX_ARCS + 1 and fams[name][0]["n_states"] <= MAX_STATES + 1
    assert item_needs(fams["self loop"][0]) is None and item_needs(fams["two-cycle"][0]) is None
    for name, (f, want) in fams.items():
        assert predict_in_kernel(f) == want, name


def test_prediction_of_the_degenerate_items():
    assert predict_in_kernel(empty_flat(start=-1)) == 1 and predict_in_kernel(dict(fan(64), start=-1)) == 1
    assert predict_in_kernel(dict(long_chain(MAX_STATES + 1), start=None)) == 1
    items = dict(parity_items())
    assert predict_in_kernel(items["k11"]) == 0  # (an epsilon self loop)
    flags = [predict_in_kernel(f) for f in items.values()]
    assert 0 in flags and flags.count(1) > len(flags) // 2 and len(flags) >= 40


def test_hung_chains_rewrite_every_depth_without_gaining_arcs():
    for length in (2, 40):
        f = hung_chain(length)
        model, needs, stats = rm_epsilon_model(f)
        assert stats["batches"] == length + 1 and len(model["arcs"]) <= len(f["arcs"])
        # (a rewritten successor has no epsilon arcs left: every closure is the state and the next one)
        assert max(c for c, _, _ in needs.values()) == 2 and predict_in_kernel(f) == 1


@functools.lru_cache(maxsize=None)
def chain_lattices():
    """32 acyclic acceptor lattices, each with epsilon arcs"""
    rng = np.random.default_rng(67)
    lats = []
    while len(lats) < 32:
        f = dc.random_acceptor(rng, int(rng.integers(10, 50)), 3, 3, p_eps_i=0.2, acyclic=True, weight_grid=1, max_w=4)
        f["finals"][-1] = 0.0
        if (f["arcs"]["ilabel"] == 0).any():
            lats.append(f)
    return lats


def test_chain_lattices_have_epsilons_and_stay_in_the_kernel():
    lats = chain_lattices()
    assert len(lats) == 32 and all(predict_in_kernel(f) for f in lats)
    assert all(((f["arcs"]["ilabel"] == 0) & (f["arcs"]["olabel"] == 0)).any() and f["props"] & ACCEPTOR for f in lats)


# ================================================================ GPU
def _batch(devs, ctx):
    import rustfst_amd
    outs, flags = rustfst_amd.rm_epsilon_batch(devs, ctx, return_in_kernel=True)
    return [o.to_flat() for o in outs], [int(x) for x in flags]


def _stats(ctx):
    import rustfst_amd
    return rustfst_amd.rm_epsilon_batch_stats(ctx)


def check_list(items, ctx, oracle, single=True):
    """one batch call; every result against the oracle and the single call on the same handle, the flags against the
    prediction, the counters against the flags.  Returns (results, flags, handles)."""
    devs = [to_device(f, ctx) for _, f in items]
    got, flags = _batch(devs, ctx)
    want = [predict_in_kernel(f) for _, f in items]
    print("flags %s\nstats %s" % (flags, _stats(ctx)))
    assert flags == want
    st = _stats(ctx)
    assert st["items_in_kernel"] == sum(want) and st["items_single"] == len(want) - sum(want)
    for k, ((name, flat), g) in enumerate(zip(items, got)):
        same(g, oracle_rm_epsilon(oracle, name, flat), f"item {k} ({name}) vs the oracle")
        if single:
            same(g, devs[k].rm_epsilon().to_flat(), f"item {k} ({name}) vs the single call")
    return got, flags, devs


@pytest.mark.gpu
def test_parity_of_one_mixed_batch(gpu_ctx, oracle):
    import rustfst_amd
    items = parity_items()
    assert len(items) >= 40
    got, flags, devs = check_list(items, gpu_ctx, oracle)
    by = dict(zip((name for name, _ in items), got))
    assert by["no states"]["n_states"] == 0 and by["trims to nothing"]["n_states"] == 0
    assert by["no start"]["n_states"] == fan(15)["n_states"] and by["no start"]["start"] in (None, -1)
    assert 0 in flags and 1 in flags
    # the same handle twice, and an item between the two
    outs = rustfst_amd.rm_epsilon_batch([devs[1], devs[2], devs[1]], gpu_ctx)
    same(outs[0].to_flat(), got[1], "the same handle twice: first")
    same(outs[2].to_flat(), got[1], "the same handle twice: second")
    same(outs[1].to_flat(), got[2], "the same handle twice: between")


@pytest.mark.gpu
def test_both_sides_of_every_limit(gpu_ctx, oracle):
    fams = limit_families()
    items = [(name, f) for name, f, _ in fams]
    got, flags, _ = check_list(items, gpu_ctx, oracle, single=False)
    assert flags == [want for _, _, want in fams]
    assert _stats(gpu_ctx)["items_in_kernel"] == flags.count(1) and _stats(gpu_ctx)["items_single"] == flags.count(0)


@pytest.mark.gpu
def test_arena_growth(gpu_ctx, oracle, monkeypatch):
    import rustfst_amd
    items = parity_items()
    devs = [to_device(f, gpu_ctx) for _, f in items]
    plain, flags0 = _batch(devs, gpu_ctx)
    monkeypatch.setenv("WFST_RM_EPSILON_BATCH_ARENA", "min")
    grown, flags = _batch(devs, gpu_ctx)
    st = _stats(gpu_ctx)
    print("min arenas: %s" % st)
    assert st["launches"] > 1 and flags == flags0 == [predict_in_kernel(f) for _, f in items]
    for k, ((name, flat), g, p) in enumerate(zip(items, grown, plain)):
        same(g, p, f"item {k} ({name}) grown vs not")
        same(g, oracle_rm_epsilon(oracle, name, flat), f"item {k} ({name}) grown vs the oracle")
    monkeypatch.setenv("WFST_RM_EPSILON_BATCH_ARENA", "max")
    with pytest.raises(rustfst_amd.WfstError, match="WFST_RM_EPSILON_BATCH_ARENA: expected min"):
        rustfst_amd.rm_epsilon_batch(devs[:2], gpu_ctx)
    monkeypatch.delenv("WFST_RM_EPSILON_BATCH_ARENA")
    # results no larger than the inputs: one launch
    small = [(name, f) for name, f in items if has_start(f) and f["n_states"] and predict_in_kernel(f)
             and len(rm_epsilon_model(f)[0]["arcs"]) <= len(f["arcs"])]
    assert len(small) >= 10
    _batch([to_device(f, gpu_ctx) for _, f in small], gpu_ctx)
    assert _stats(gpu_ctx) == dict(launches=1, items_in_kernel=len(small), items_single=0)


@pytest.mark.gpu
def test_launches_depend_neither_on_the_list_nor_on_the_depth(gpu_ctx, oracle):
    f = dict(parity_items())["random 0 p 0.1 acyclic acceptor"]
    assert predict_in_kernel(f) == 1
    dev = to_device(f, gpu_ctx)
    launches = []
    for n in (1, 8, 64):
        got, flags = _batch([dev] * n, gpu_ctx)
        assert flags == [1] * n
        same(got[-1], oracle_rm_epsilon(oracle, "random 0 p 0.1 acyclic acceptor", f), f"n = {n}")
        launches.append(_stats(gpu_ctx)["launches"])
    assert launches[0] == launches[1] == launches[2] >= 1
    per_depth = []
    for length in (2, 40):
        h = hung_chain(length)
        got, flags = _batch([to_device(h, gpu_ctx)], gpu_ctx)
        assert flags == [1]
        same(got[0], oracle_rm_epsilon(oracle, "hung chain %d" % length, h), f"hung chain {length}")
        per_depth.append(_stats(gpu_ctx)["launches"])
    assert per_depth[0] == per_depth[1] >= 1


@pytest.mark.gpu
def test_inputs_are_left_as_they_are(gpu_ctx):
    items = parity_items()
    devs = [to_device(f, gpu_ctx) for _, f in items]
    before = [d.to_flat() for d in devs]
    probe = [name for name, _ in items].index("random 3 p 0.4 acyclic transducer")
    path_before = devs[probe].shortest_path().to_flat()  # (builds the handle's cached derived data)
    _batch(devs, gpu_ctx)
    _batch(devs, gpu_ctx)
    for (name, _), d, b in zip(items, devs, before):
        same(d.to_flat(), b, f"{name}: the input after two batch calls")
    same(devs[probe].shortest_path().to_flat(), path_before, "shortest_path on an input after the batch calls")


def _raw_batch(handles, ctx):
    from rustfst_amd import _lib
    n = len(handles)
    arr = (C.c_void_p * n)(*handles)
    outs = (C.c_void_p * n)(*([1] * n))
    return _lib.lib().wfst_rm_epsilon_batch(ctx._h, arr, n, outs, None), outs


@pytest.mark.gpu
def test_errors(gpu_ctx, oracle):
    import rustfst_amd
    from rustfst_amd import _lib
    items = parity_items()[:12]
    devs = [to_device(f, gpu_ctx) for _, f in items]
    good, _ = _batch(devs, gpu_ctx)
    assert _stats(gpu_ctx)["launches"] >= 1
    hs = [d._h.value for d in devs]
    # a NULL entry: the message carries the index
    status, outs = _raw_batch(hs[:5] + [None] + hs[6:], gpu_ctx)
    assert status == 1 and helpers.ko_message(1) == "item 5: null FST in batch"
    assert [outs[i] for i in range(12)] == [None] * 12
    assert _stats(gpu_ctx) == dict(launches=0, items_in_kernel=0, items_single=0)
    for g, e in zip(_batch(devs, gpu_ctx)[0], good):
        same(g, e, "after the NULL entry")
    # a handle of a second context: KO before anything is launched
    other = rustfst_amd.Context(0)
    foreign = to_device(items[3][1], other)
    status, outs = _raw_batch(hs[:3] + [foreign._h.value] + hs[4:], gpu_ctx)
    msg = helpers.ko_message(status)
    assert "item 3" in msg and "another context" in msg
    assert [outs[i] for i in range(12)] == [None] * 12
    assert _stats(gpu_ctx) == dict(launches=0, items_in_kernel=0, items_single=0)
    for g, e in zip(_batch(devs, gpu_ctx)[0], good):
        same(g, e, "after the foreign handle")
    del foreign
    # n == 0
    assert _lib.lib().wfst_rm_epsilon_batch(gpu_ctx._h, None, 0, None, None) == 0
    assert _stats(gpu_ctx) == dict(launches=0, items_in_kernel=0, items_single=0)
    assert rustfst_amd.rm_epsilon_batch([], gpu_ctx) == []


@pytest.mark.gpu
def test_chain_of_the_three_batch_calls(gpu_ctx):
    import rustfst_amd
    rng = np.random.default_rng(67)
    lats = chain_lattices()
    devs = [to_device(f, gpu_ctx) for f in lats]
    no_eps, flags = rustfst_amd.rm_epsilon_batch(devs, gpu_ctx, return_in_kernel=True)
    assert [int(x) for x in flags] == [1] * 32
    minis = rustfst_amd.minimize_batch(rustfst_amd.determinize_batch(no_eps, None, gpu_ctx), None, gpu_ctx)
    for k, (d, m) in enumerate(zip(devs, minis)):
        same(m.to_flat(), d.rm_epsilon().determinize().minimize().to_flat(), f"lattice {k}: the chain vs three single calls")
