"""wfst_minimize_batch: the C-ABI and Python surface without a GPU, and on the device parity of every batch item with the
Python restatement of minimize_with_config (oracle.model's minimize_ref) AND with the single call on the same handle, bit for
bit including the property word: known answers and degenerate items, mixed random lists of three lengths (one launch
each), shapes that cross the kernel's internal boundaries (more states / arcs / levels than the workgroup has threads,
fan-out above 64 and above 256), the edges of the in_kernel rule, more items than workgroups can be resident, the
determinize_batch -> minimize_batch pipeline, every KO of the single call at a given index, and untouched inputs."""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest

from rustfst_amd._lib import TR_DTYPE
from oracle import model
import helpers
from helpers import assert_flat_identical, empty_flat, golden_flat, to_device
import determinize_cases as dc
import minimize_cases as mc
from oracle.model import minimize_ref

ROOT = helpers.ROOT
INF = float("inf")
F32 = np.float32
MAX_STATES, MAX_ARCS = 4096, 16384  # include/wfst.h: the in_kernel rule of wfst_minimize_batch
DELTAS = (1e-6, 1.0 / 1024.0)
KNOWN_W = model.ACCEPTOR | model.I_DETERMINISTIC | model.WEIGHTED | model.ACYCLIC | model.INITIAL_ACYCLIC
KNOWN_U = model.ACCEPTOR | model.I_DETERMINISTIC | model.UNWEIGHTED | model.ACYCLIC | model.INITIAL_ACYCLIC
INITIAL_CYCLIC = model.INITIAL_CYCLIC


def predict_in_kernel(flat):
    """wfst.h: 1 exactly when the item has at most 4096 states and at most 16384 arcs (a word that says INITIAL_CYCLIC is
    handed to the single call)"""
    return int(flat["n_states"] <= MAX_STATES and len(flat["arcs"]) <= MAX_ARCS and not flat["props"] & INITIAL_CYCLIC)


def same(got, exp, what):
    assert_flat_identical(got, exp, what, check_props=True)


def with_true_word(flat):
    """the item with a word that knows every fact minimize asks for (truthfully)"""
    w = np.concatenate([flat["arcs"]["weight"], flat["finals"][np.isfinite(flat["finals"])]])
    weighted = bool(np.any(np.abs(w) > model.KDELTA))
    return dict(flat, props=KNOWN_W if weighted else KNOWN_U)


# ================================================================ no GPU
NEW_SYMBOLS = ("wfst_minimize_batch", "wfst_ctx_get_minimize_batch_stats")


def test_new_symbols_declared_exported_and_bound(wfst_lib):
    from rustfst_amd import _lib
    with open(os.path.join(ROOT, "include", "wfst.h")) as f:
        header = f.read()
    bound = {name for name, _, _ in _lib.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert re.search(r"\bwfst_status\s+%s\s*\(" % name, header), name
        assert name in bound and hasattr(wfst_lib, name), name
    assert re.search(r"#define\s+WFST_ABI_VERSION\s+7\b", header) and wfst_lib.wfst_abi_version() == 7
    # the limits the in_kernel flag is defined by are part of the header
    assert "at most 4096 states" in header and "16384 arcs" in header


def test_argument_validation_without_gpu(wfst_lib):
    from rustfst_amd import _lib
    ko = helpers.ko_message
    outs = (C.c_void_p * 3)(1, 1, 1)
    fsts = (C.c_void_p * 3)()
    assert wfst_lib.wfst_minimize_batch(None, None, 0, None, None, None) == 0  # n == 0: OK
    assert "null" in ko(wfst_lib.wfst_minimize_batch(None, fsts, 3, None, outs, None))  # NULL ctx
    assert [outs[i] for i in range(3)] == [None] * 3
    assert "null" in ko(wfst_lib.wfst_minimize_batch(None, fsts, 3, None, None, None))  # NULL outs
    outs = (C.c_void_p * 3)(1, 1, 1)
    assert "null" in ko(wfst_lib.wfst_minimize_batch(None, None, 3, None, outs, None))  # NULL fsts with n > 0
    assert [outs[i] for i in range(3)] == [None] * 3
    for d in (0.0, -1e-3, float("nan"), float("inf")):
        cfg = _lib.MinimizeConfig(d, 0)
        outs = (C.c_void_p * 3)(1, 1, 1)
        assert "delta" in ko(wfst_lib.wfst_minimize_batch(None, fsts, 3, C.byref(cfg), outs, None))
        assert [outs[i] for i in range(3)] == [None] * 3
        assert "delta" in ko(wfst_lib.wfst_minimize_batch(None, None, 0, C.byref(cfg), None, None))
    assert "null" in ko(wfst_lib.wfst_ctx_get_minimize_batch_stats(None, None, None, None))


def test_null_entry_is_ko(wfst_lib):
    """a NULL entry is reported with its index before anything else is done with the context.  No context can be made without
    a device, so the one here is a block of zeroed memory: THIS TEST DEPENDS ON THE LAYOUT OF wfst_ctx, in that the struct
    must stay smaller than the block (1 MiB) and the call must do no more with the context, before it has checked the
    list, than clear its three stat words (which keeps "all 0 after a KO before any launch" true for this KO too)."""
    ko = helpers.ko_message
    ctx = C.create_string_buffer(1 << 20)
    outs = (C.c_void_p * 3)(1, 1, 1)
    fsts = (C.c_void_p * 3)()
    msg = ko(wfst_lib.wfst_minimize_batch(C.cast(ctx, C.c_void_p), fsts, 3, None, outs, None))
    assert "item 0" in msg and "null" in msg and [outs[i] for i in range(3)] == [None] * 3
    assert ctx.raw == bytes(1 << 20)


def test_python_surface():
    import rustfst_amd
    for name in ("minimize_batch", "minimize_batch_stats"):
        assert name in rustfst_amd.__all__ and callable(getattr(rustfst_amd, name))
    p = inspect.signature(rustfst_amd.minimize_batch).parameters
    assert list(p) == ["fsts", "config", "ctx", "return_in_kernel"]
    assert p["config"].default is None and p["ctx"].default is None and p["return_in_kernel"].default is False
    assert list(inspect.signature(rustfst_amd.minimize_batch_stats).parameters) == ["ctx"]
    assert rustfst_amd.minimize_batch([]) == []
    res, flags = rustfst_amd.minimize_batch([], return_in_kernel=True)
    assert res == [] and flags.dtype == np.uint8 and len(flags) == 0


def test_prediction_of_the_rule():
    f = model.make_flat(2, 0, [[(1, 1, 0.0, 1)], []], [INF, 0.0])
    assert predict_in_kernel(f) == 1 and predict_in_kernel(empty_flat()) == 1
    assert predict_in_kernel(dict(f, n_states=MAX_STATES)) == 1 and predict_in_kernel(dict(f, n_states=MAX_STATES + 1)) == 0
    assert predict_in_kernel(dict(f, arcs=np.zeros(MAX_ARCS, TR_DTYPE))) == 1
    assert predict_in_kernel(dict(f, arcs=np.zeros(MAX_ARCS + 1, TR_DTYPE))) == 0


# ================================================================ GPU
def _cfg(delta=None, allow_nondet=False):
    import rustfst_amd
    return None if delta is None and not allow_nondet else rustfst_amd.MinimizeConfig(delta, allow_nondet)


def _batch(devs, ctx, delta=None):
    import rustfst_amd
    outs, flags = rustfst_amd.minimize_batch(devs, _cfg(delta), ctx, return_in_kernel=True)
    return [o.to_flat() for o in outs], [int(x) for x in flags]


def _stats(ctx):
    import rustfst_amd
    return rustfst_amd.minimize_batch_stats(ctx)


def check_list(items, ctx, delta=None, single=True, upload_many=False):
    """items: [(name, flat)].  One batch call; every result against the restatement and (single: all, or an index list)
    against the single call on the same handle; the flags against the rule; the stats.  Returns the results."""
    import rustfst_amd
    flats = [f for _, f in items]
    devs = rustfst_amd.DeviceFst.upload_many(flats, ctx) if upload_many else [to_device(f, ctx) for f in flats]
    got, flags = _batch(devs, ctx, delta)
    want = [predict_in_kernel(f) for f in flats]
    assert flags == want
    st = _stats(ctx)
    assert st["items_in_kernel"] == sum(want) and st["items_single"] == len(want) - sum(want)
    assert st["launches"] == (1 if any(w and f["n_states"] for w, f in zip(want, flats)) else 0)
    d = model.KSHORTESTDELTA if delta is None else delta
    which = range(len(items)) if single is True else single
    for k, ((name, flat), g) in enumerate(zip(items, got)):
        same(g, minimize_ref(flat, d), f"item {k} ({name}) delta {d} vs the restatement")
    for k in which:
        same(got[k], devs[k].minimize(_cfg(delta)).to_flat(), f"item {k} ({items[k][0]}) delta {d} vs the single call")
    return got, devs


@pytest.mark.gpu
def test_known_answers_and_degenerate_items(gpu_ctx):
    groups = {}
    for c in mc.golden_cases():
        delta, nondet = mc.cfg_of(c)
        if not nondet:
            groups.setdefault(delta, []).append((c["name"], golden_flat(c), golden_flat(c, "expected")))
    assert sum(len(g) for g in groups.values()) >= 8
    gone, gone_known = mc.no_start_cases()[0][0], mc.no_start_cases()[1][0]
    degenerate = [
        ("no states", empty_flat()), ("no states, known word", empty_flat(KNOWN_U)),
        ("no start, unweighted", model.make_flat(2, None, [[(1, 1, 0.0, 1)], []], [INF, 0.0], model.ACCEPTOR)),
        ("no start, unweighted, word 0", model.make_flat(2, None, [[(1, 1, 0.0, 1)], []], [INF, 0.0], 0)),
        ("no start, weighted, all-one pushed", gone), ("no start, weighted, known word", gone_known),
        ("one final state", model.make_flat(1, 0, [[]], [0.0], 0)), ("one final state, weight 2", model.make_flat(1, 0, [[]], [2.0], 0)),
        ("trims to nothing", model.make_flat(3, 0, [[(1, 1, 1.0, 1)], [(1, 1, 2.0, 2)], []], [INF, INF, INF], model.ACCEPTOR)),
        ("trims to nothing, unweighted", model.make_flat(3, 0, [[(1, 1, 0.0, 1)], [(2, 2, 0.0, 2)], []], [INF, INF, INF], 0)),
        ("final state out of reach", model.make_flat(3, 0, [[(1, 1, 1.0, 1)], [], [(1, 1, 0.5, 1)]], [INF, INF, 1.0], 0)),
    ]
    for delta, cases in groups.items():
        items = [(name, flat) for name, flat, _ in cases] + degenerate
        got, devs = check_list(items, gpu_ctx, delta)
        for (name, _, expected), g in zip(cases, got):
            same(g, expected, f"{name}: the known answer")
        for (name, _), g in zip(degenerate, got[len(cases):]):
            assert (g["n_states"] == 0 and g["start"] is None) == (not name.startswith("one final state")), name
        # the same handle twice, and an item between the two
        import rustfst_amd
        twice = [devs[0], devs[1], devs[0]]
        outs = rustfst_amd.minimize_batch(twice, _cfg(delta), gpu_ctx)
        same(outs[0].to_flat(), got[0], "the same handle twice: first")
        same(outs[2].to_flat(), got[0], "the same handle twice: second")
        same(outs[1].to_flat(), got[1], "the same handle twice: between")
    # allow_nondet reaches the items (a deterministic input gives the same answer)
    import rustfst_amd
    f = dict(degenerate)["one final state, weight 2"]
    out = rustfst_amd.minimize_batch([to_device(f, gpu_ctx)], _cfg(1e-6, True), gpu_ctx)[0]
    same(out.to_flat(), minimize_ref(f, 1e-6, True), "allow_nondet")


@pytest.mark.gpu
def test_mixed_random_lists_take_one_launch_each(gpu_ctx):
    launches = []
    for seed, count in ((41, 64), (42, 8), (43, 200)):
        items = []
        for k, (name, flat) in enumerate(mc.random_cases(seed, count)):
            items.append((name, with_true_word(flat) if k % 3 == 2 else flat))
        kinds = {name for name, _ in items}
        assert {"trie-w", "trie-u", "dag-w", "dag-u"} <= kinds
        assert any(f["props"] == 0 for _, f in items) and any(f["props"] in (KNOWN_W, KNOWN_U) for _, f in items)
        assert all(predict_in_kernel(f) for _, f in items)
        check_list(items, gpu_ctx, single=True if count <= 64 else range(0, count, 7))
        launches.append(_stats(gpu_ctx)["launches"])
    assert launches == [1, 1, 1]


def chain(n, weighted, real=False, seed=1):
    rng = np.random.default_rng(seed)
    rows = [[(1 + s % 3, 1 + s % 3, float(F32(rng.random() * 3)) if real else (float(s % 4) if weighted else 0.0), s + 1)]
            for s in range(n - 1)] + [[]]
    finals = [INF] * (n - 1) + [1.0 if weighted else 0.0]
    return model.make_flat(n, 0, rows, finals, model.ACCEPTOR if weighted else 0)


def hubs(width, weighted):
    """two hub states of `width` arcs with distinct labels in random order that merge, next to one that differs in a single
    target (test_minimize.test_fan_out_above_64 at another width)"""
    rng = np.random.default_rng(width)
    labs = rng.permutation(np.arange(1, width + 1))
    rows = [[(1, 1, 0.0, 1), (2, 2, 0.0, 2), (3, 3, 0.0, 3)], [], [], [], [], [], [], [], [(7, 7, 1.0, 4)], [(7, 7, 1.0, 5)]]
    odd = width // 2
    for k, lab in enumerate(labs):
        t = (4, 6, 8)[k % 3]
        w = float(k % 2) if weighted else 0.0
        rows[1].append((int(lab), int(lab), w, t))
        rows[2].append((int(lab), int(lab), w, t + 1))
        rows[3].append((int(lab), int(lab), w, t + 1 if k != odd else 4 + (k + 1) % 3 * 2))
    if not weighted:
        rows[8], rows[9] = [(7, 7, 0.0, 4)], [(7, 7, 0.0, 5)]
    finals = [INF] * 4 + ([0.0, 0.0, 1.0, 1.0] if weighted else [0.0] * 4) + [INF, INF]
    return model.make_flat(10, 0, rows, finals, model.ACCEPTOR if weighted else 0)


def real_dag(n):
    """a random DAG with real-valued weights of which a good part survives connect"""
    for seed in range(100):
        f = mc.random_dag(np.random.default_rng(seed), n, 4, True, real=True)
        fst = model.flat_to_fst(f)
        model.connect(fst)
        if 3 * len(fst["rows"]) >= n:
            return f
    raise AssertionError("no seed gives a connected part")


@functools.lru_cache(maxsize=None)
def boundary_items():
    rng = np.random.default_rng(77)
    trie = mc.trie_flat(rng, 800, 10, 10, True)
    trie_u = mc.trie_flat(rng, 800, 10, 10, False)
    assert 2500 <= trie["n_states"] <= MAX_STATES and 2500 <= trie_u["n_states"] <= MAX_STATES
    m = mc.closed_form_base(np.random.default_rng(33))
    all_final = mc.random_dag(rng, 120, 4, True, real=True)
    all_final["finals"] = (rng.permutation(120).astype(np.float32) / F32(7.0) + F32(0.01)).astype(np.float32)
    one_tuple = model.make_flat(40, 0, [[(1, 1, 0.0, s + 1)] for s in range(39)] + [[]], [INF] * 39 + [1.0], 0)
    one_tuple_u = model.make_flat(40, 0, [[(1, 1, 0.0, s + 1)] for s in range(39)] + [[]], [INF] * 39 + [0.0], 0)
    items = [("chain 1500 weighted", chain(1500, True)), ("chain 1500 unweighted", chain(1500, False)),
             ("chain 700 real", chain(700, True, real=True)),
             ("hubs 300", hubs(300, True)), ("hubs 1100", hubs(1100, True)), ("hubs 1100 unweighted", hubs(1100, False)),
             ("trie", trie), ("trie unweighted", trie_u),
             ("blow_up 3", mc.blow_up(rng, m, 3)), ("blow_up 7", mc.blow_up(rng, m, 7)),
             ("every state final", all_final), ("one tuple", one_tuple), ("one tuple unweighted", one_tuple_u),
             ("real dag", real_dag(300))]
    return items


@pytest.mark.gpu
@pytest.mark.parametrize("delta", DELTAS)
def test_shapes_across_the_kernel_boundaries(gpu_ctx, delta):
    items = boundary_items()
    assert all(predict_in_kernel(f) for _, f in items)
    got, _ = check_list(items, gpu_ctx, delta)
    by = {name: g for (name, _), g in zip(items, got)}
    assert by["chain 1500 weighted"]["n_states"] == 1500  # deeper than the workgroup has threads, nothing merges
    assert by["hubs 1100"]["n_states"] < 10 and len(by["hubs 1100"]["arcs"]) > 2 * 1100
    assert by["every state final"]["n_states"] >= 90 and by["real dag"]["n_states"] >= 50
    m = mc.closed_form_base(np.random.default_rng(33))
    assert by["blow_up 7"]["n_states"] == m["n_states"] < dict(items)["blow_up 7"]["n_states"] // 6


def dag_with(n_states, n_arcs, seed, weighted=True):
    """a deterministic DAG with exactly n_states states and n_arcs arcs: a binary tree (state s into 2s + 1 and 2s + 2,
    so that the Python restatement stays shallow) and the other arcs spread over the first states, labels distinct per
    state; the states without arcs are final"""
    rng = np.random.default_rng(seed)
    assert n_arcs >= n_states - 1
    rows = [[] for _ in range(n_states)]
    for s in range(1, n_states):
        p = (s - 1) // 2
        rows[p].append((1 + (s - 1) % 2, 1 + (s - 1) % 2, float(s % 3) if weighted else 0.0, s))
    extra = n_arcs - (n_states - 1)
    heads = max(1, min(n_states - 2, 120))
    for j in range(extra):
        s = j % heads
        t = int(rng.integers(s + 1, n_states))
        rows[s].append((3 + j // heads, 3 + j // heads, float((s + j) % 2) if weighted else 0.0, t))
    finals = [0.0 if not r else INF for r in rows]
    f = model.make_flat(n_states, 0, rows, finals, model.ACCEPTOR)
    assert f["n_states"] == n_states and len(f["arcs"]) == n_arcs
    return f


@pytest.mark.gpu
def test_edges_of_the_in_kernel_rule(gpu_ctx):
    import rustfst_amd
    items = [("states at the limit", dag_with(MAX_STATES, MAX_STATES + 50, 1)),
             ("states past the limit", dag_with(MAX_STATES + 1, MAX_STATES + 50, 1)),
             ("arcs at the limit", dag_with(300, MAX_ARCS, 2)), ("arcs past the limit", dag_with(300, MAX_ARCS + 1, 2)),
             ("both at the limit", dag_with(MAX_STATES, MAX_ARCS, 3, weighted=False)),
             ("small", dag_with(20, 60, 4))]
    assert [predict_in_kernel(f) for _, f in items] == [1, 0, 1, 0, 1, 1]
    check_list(items, gpu_ctx)
    st = _stats(gpu_ctx)
    assert st == dict(launches=1, items_in_kernel=4, items_single=2)
    # only items for the single path: no launch of the batch kernel
    check_list(items[1:2], gpu_ctx)
    assert _stats(gpu_ctx) == dict(launches=0, items_in_kernel=0, items_single=1)
    # the one exception to the rule: a word that says INITIAL_CYCLIC (here against ACYCLIC and the content) sends a small item
    # to the single call, whose answer, or KO, is the batch call's
    odd = dict(items[5][1], props=(KNOWN_W & ~model.INITIAL_ACYCLIC) | INITIAL_CYCLIC)
    assert predict_in_kernel(odd) == 0 and odd["n_states"] == 20
    devs = [to_device(items[5][1], gpu_ctx), to_device(odd, gpu_ctx)]
    try:
        want = devs[1].minimize().to_flat()
    except rustfst_amd.WfstError as e:
        with pytest.raises(rustfst_amd.WfstError, match=re.escape("item 1: " + str(e).split(": ", 1)[-1])):
            _batch(devs, gpu_ctx)
    else:
        got, flags = _batch(devs, gpu_ctx)
        assert flags == [1, 0] and _stats(gpu_ctx) == dict(launches=1, items_in_kernel=1, items_single=1)
        same(got[1], want, "INITIAL_CYCLIC word vs the single call")
        same(got[0], minimize_ref(items[5][1]), "the item beside it")


@pytest.mark.gpu
def test_more_items_than_resident_workgroups(gpu_ctx):
    rng = np.random.default_rng(3000)
    items = []
    for k in range(3000):
        n = int(rng.integers(1, 9))
        flat = mc.random_dag(rng, n, 3, weighted=k % 2 == 0, props=model.ACCEPTOR if k % 3 else 0, real=k % 5 == 0)
        items.append((f"tiny {k}", flat))
    assert max(f["n_states"] for _, f in items) <= 8
    check_list(items, gpu_ctx, single=[int(i) for i in rng.choice(3000, size=50, replace=False)], upload_many=True)
    assert _stats(gpu_ctx) == dict(launches=1, items_in_kernel=3000, items_single=0)


@pytest.mark.gpu
def test_determinize_batch_then_minimize_batch(gpu_ctx):
    import rustfst_amd
    rng = np.random.default_rng(66)
    lats = [dc.random_acceptor(rng, int(rng.integers(10, 50)), 3, 3, acyclic=True, weight_grid=1, max_w=4) for _ in range(32)]
    for f in lats:
        f["finals"][-1] = 0.0
    devs = [to_device(f, gpu_ctx) for f in lats]
    dets = rustfst_amd.determinize_batch(devs, None, gpu_ctx)
    minis, flags = rustfst_amd.minimize_batch(dets, None, gpu_ctx, return_in_kernel=True)
    assert [int(x) for x in flags] == [1] * 32 and _stats(gpu_ctx)["launches"] == 1
    shrunk = 0
    for k, (det, mini) in enumerate(zip(dets, minis)):
        det_flat, got = det.to_flat(), mini.to_flat()
        same(got, det.minimize().to_flat(), f"lattice {k} vs the single call")
        same(got, minimize_ref(det_flat), f"lattice {k} vs the restatement")
        shrunk += got["n_states"] < det_flat["n_states"]
        if k % 4 == 0:
            mc.check_invariants(det_flat, mini, model.KSHORTESTDELTA, gpu_ctx, rng, f"lattice {k}")
    assert shrunk >= 4


def bad_items():
    cyc = model.make_flat(3, 0, [[(1, 1, 1.0, 1)], [(1, 1, 0.0, 2), (2, 2, 0.0, 0)], []], [INF, INF, 0.0], 0)
    # states 3 and 4 form a cycle nothing reaches: connect would remove it
    hidden = model.make_flat(5, 0, [[(1, 1, 1.0, 1)], [(1, 1, 0.0, 2)], [], [(1, 1, 0.0, 4)], [(1, 1, 0.0, 3)]],
                          [INF, INF, 0.0, INF, INF], model.ACCEPTOR)
    nd = model.make_flat(3, 0, [[(1, 1, 0.0, 1), (1, 1, 1.0, 2)], [], []], [INF, 0.0, 0.0], 0)
    tr = model.make_flat(2, 0, [[(1, 2, 0.0, 1)], []], [INF, 0.0], 0)
    far = mc.far_apart_cases()[0]
    stays = mc.no_start_cases()[2][0]
    return [("cyclic", cyc, "cyclic inputs"), ("hidden cycle", hidden, "cyclic inputs"), ("non-deterministic", nd, "Refusing"),
            ("transducer", tr, "transducers"), ("far apart", far, "further than 1/1024 apart"),
            ("start-less with a leftover weight", stays, "FST is not an unweighted acceptor")]


def _single_message(dev, ctx, allow_nondet=False):
    from rustfst_amd import _lib
    out = C.c_void_p()
    cfg = _lib.MinimizeConfig(1e-6, 1 if allow_nondet else 0)
    assert _lib.lib().wfst_minimize(ctx._h, dev._h, C.byref(cfg), C.byref(out)) == 1 and out.value is None
    return helpers.ko_message(1)


def _raw_batch(devs, ctx, allow_nondet=False):
    from rustfst_amd import _lib
    n = len(devs)
    arr = (C.c_void_p * n)(*[d._h.value for d in devs])
    outs = (C.c_void_p * n)(*([1] * n))
    cfg = _lib.MinimizeConfig(1e-6, 1 if allow_nondet else 0)
    status = _lib.lib().wfst_minimize_batch(ctx._h, arr, n, C.byref(cfg), outs, None)
    return status, outs


@pytest.mark.gpu
def test_errors(gpu_ctx):
    import rustfst_amd
    goods = [f for _, f in mc.random_cases(5, 12)]
    devs = [to_device(f, gpu_ctx) for f in goods]
    good, _ = _batch(devs, gpu_ctx)
    assert _stats(gpu_ctx)["launches"] == 1
    bads = bad_items()
    bad_devs = [to_device(f, gpu_ctx) for _, f, _ in bads]
    for k, ((name, flat, pattern), bad) in enumerate(zip(bads, bad_devs)):
        for nondet in ((False, True) if name == "non-deterministic" else (False,)):
            single = _single_message(bad, gpu_ctx, nondet)
            assert re.search("non-deterministic inputs are not supported" if nondet else pattern, single), (name, single)
            mixed = devs[:5] + [bad] + devs[6:]
            status, outs = _raw_batch(mixed, gpu_ctx, nondet)
            assert status == 1 and helpers.ko_message(1) == "item 5: " + single, name
            assert [outs[i] for i in range(12)] == [None] * 12, name
            # a second bad item further on: the lowest index is reported
            mixed[9] = bad_devs[(k + 1) % len(bads)]
            status, outs = _raw_batch(mixed, gpu_ctx, nondet)
            assert status == 1 and helpers.ko_message(1) == "item 5: " + single, name
            assert [outs[i] for i in range(12)] == [None] * 12, name
            # the context works afterwards
            for g, e in zip(_batch(devs, gpu_ctx)[0], good):
                same(g, e, f"after the KO of {name}")
    with pytest.raises(rustfst_amd.WfstError, match="item 5: .*cyclic inputs are not supported"):
        rustfst_amd.minimize_batch(devs[:5] + [bad_devs[0]] + devs[6:], None, gpu_ctx)
    # a handle of another context: KO before anything is launched
    other = rustfst_amd.Context(0)
    foreign = to_device(goods[3], other)
    status, outs = _raw_batch(devs[:3] + [foreign] + devs[4:], gpu_ctx)
    msg = helpers.ko_message(status)
    assert "item 3" in msg and "another context" in msg
    assert [outs[i] for i in range(12)] == [None] * 12
    assert _stats(gpu_ctx) == dict(launches=0, items_in_kernel=0, items_single=0)
    for g, e in zip(_batch(devs, gpu_ctx)[0], good):
        same(g, e, "after the foreign handle")
    del foreign


@pytest.mark.gpu
def test_inputs_are_left_as_they_are(gpu_ctx):
    items = [(name, with_true_word(f) if k % 2 else f) for k, (name, f) in enumerate(mc.random_cases(9, 24))]
    items += [("no start", mc.no_start_cases()[0][0]), ("empty", empty_flat()), ("hubs", hubs(300, True))]
    devs = [to_device(f, gpu_ctx) for _, f in items]
    before = [d.to_flat() for d in devs]
    for (name, f), b in zip(items, before):
        same(b, dict(f, props=b["props"]), f"{name}: upload")
    _batch(devs, gpu_ctx)
    _batch(devs, gpu_ctx, 1.0 / 1024.0)
    for (name, _), d, b in zip(items, devs, before):
        same(d.to_flat(), b, f"{name}: the input after two batch calls")
