"""wfst_optimize_batch: the C-ABI and Python surface without a GPU; on the device parity of every item of a mixed list with
test_optimize's restatement (optimize_ref) AND with the loop of optimize calls on the same handles, bit for bit including
the property word; the K17 known answers as a list; the in_kernel flags and the transducer count; launch counts that do not
depend on the list's length; the KO order of the loop of single calls (a later stage may fail at a lower index than an
earlier one); and the four batch stages chained by hand against the one call.

Items have 8 to 40 states (optimize_cases.optimize_input: acyclic by construction, integer weights, eps:eps and parallel
arcs, the word computed from the content); only the two items that leave the tr_sum kernel by size are larger."""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest
from oracle import model
from oracle.model import (ACCEPTOR, ACYCLIC, INF, I_DETERMINISTIC, MSG_ACYCLIC, NOT_I_DETERMINISTIC, NO_EPSILONS,
                          branch_of, content_word_of_flat, optimize_ref, rows_flat)
import helpers
from helpers import assert_flat_identical, golden_flat, to_device
import optimize_cases as oc
from optimize_cases import optimize_input

ROOT = helpers.ROOT
STAGES = ("rm_epsilon", "tr_sum", "determinize", "minimize")
SIGNATURES = {
    "wfst_optimize_batch": "wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, wfst_fst** outs, uint8_t* in_kernel",
    "wfst_ctx_get_optimize_batch_stats": "wfst_ctx* ctx, uint64_t* launches /* [4]: rm_epsilon, tr_sum, determinize, "
                                         "minimize */, uint64_t* items_in_kernel, uint64_t* items_single, "
                                         "uint64_t* items_transducer",
}


def same(got, exp, what):
    assert_flat_identical(got, exp, what, check_props=True)


# ---------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def mixed_items():
    """[(name, flat, kind)]: kind is what the item is in the list for"""
    rng = np.random.default_rng(1710)
    out = []

    def draw(transducer, want_eps, **kw):  # (an eps:eps arc is drawn per state with probability 0.2: draw until one is there)
        while True:
            f = optimize_input(rng, int(rng.integers(8, 41)), transducer, **kw)
            if has_eps(f) == want_eps:
                return f
    for k in range(4):
        out.append((f"acceptor with epsilons {k}", draw(False, True), "eps"))
        out.append((f"acceptor without epsilons {k}", draw(False, False, eps=False), "no-eps"))
        out.append((f"deterministic {k}", draw(False, False, deterministic=True), "det"))
        out.append((f"transducer {k}", draw(True, k % 2 == 0, eps=(k % 2 == 0)), "trans"))
    out.append(("no start state", dict(optimize_input(rng, 12, False), start=None), "start-less"))
    dead = rows_flat([[(1, 1, 1.0, 1), (1, 1, 2.0, 1), (0, 0, 0.0, 2)], [(2, 2, 0.0, 2)], []] + [[]] * 5, [INF] * 8)
    out.append(("trims to nothing", dict(dead, props=content_word_of_flat(dead)), "dead"))
    return out


def is_transducer(flat):
    return not flat["props"] & ACCEPTOR


_REF = {}


def reference(name, flat, oracle):
    """optimize_ref's answer, computed once per item and left unchanged"""
    if name not in _REF:
        _REF[name] = optimize_ref(flat, oracle)
    return _REF[name]


def wide_state_acceptor():
    """a deterministic acceptor whose start state has 257 arcs: beyond the tr_sum kernel's rank sort"""
    rows = [[(1 + j, 1 + j, float(j % 3), 1 + j % 7) for j in range(257)]] + [[(1, 1, 1.0, 8)] for _ in range(7)] + [[]]
    f = rows_flat(rows, [INF] * 8 + [0.0])
    return dict(f, props=content_word_of_flat(f))


def long_chain(n=4097):
    rows = [[(1 + s % 5, 1 + s % 5, float(s % 3), s + 1)] for s in range(n - 1)] + [[]]
    f = rows_flat(rows, [INF] * (n - 1) + [0.0])
    return dict(f, props=int(model.ACCEPTOR | I_DETERMINISTIC | NO_EPSILONS | ACYCLIC | model.INITIAL_ACYCLIC | model.WEIGHTED))


def nondeterministic_acceptor(rng, n):
    while True:
        f = optimize_input(rng, n, False, eps=False)
        if f["props"] & NOT_I_DETERMINISTIC and f["props"] & NO_EPSILONS and f["props"] & ACYCLIC:
            return f


def two_state_cycle(props):
    """0 -1-> 1 -2-> 0, state 1 final: deterministic, an acceptor, cyclic"""
    return rows_flat([[(1, 1, 1.0, 1)], [(2, 2, 0.0, 0)]], [INF, 0.0], props=int(props))


# ================================================================ no GPU
def test_new_symbols_declared_exported_and_bound(wfst_lib):
    from rustfst_amd import _lib
    with open(os.path.join(ROOT, "include", "wfst.h")) as f:
        header = f.read()
    vp, u64 = C.c_void_p, C.POINTER(C.c_uint64)
    args = {"wfst_optimize_batch": [vp, C.POINTER(vp), C.c_size_t, C.POINTER(vp), vp],
            "wfst_ctx_get_optimize_batch_stats": [vp, u64, u64, u64, u64]}
    bound = {name: a for name, _, a in _lib.SYMBOLS}
    version = header[header.index("#define WFST_ABI_VERSION"):header.index("6: wfst_ctx_set_resident_share")]
    for name, want in SIGNATURES.items():
        m = re.search(r"\bwfst_status\s+%s\s*\(([^)]*)\)" % name, header)
        assert m, name
        assert " ".join(m.group(1).split()) == want, name
        assert bound[name] == args[name] and hasattr(wfst_lib, name), name
        assert re.search(r"\b%s\b" % name, version), name + " in the version-7 list"
    assert re.search(r"#define\s+WFST_ABI_VERSION\s+7\b", header) and wfst_lib.wfst_abi_version() == 7
    text = header[header.index("optimize of n FSTs in one call"):header.index("wfst_status wfst_optimize_batch")]
    assert "split the list" in text and "did not converge" in text and "LOWEST failing index" in text
    assert "4096 states" in text and "16384 arcs" in text and "256 arcs" in text


def test_argument_validation_without_gpu(wfst_lib):
    ko = helpers.ko_message
    fn = wfst_lib.wfst_optimize_batch
    outs = (C.c_void_p * 3)(1, 1, 1)
    fsts = (C.c_void_p * 3)()
    assert fn(None, None, 0, None, None) == 0  # n == 0: OK
    assert "null" in ko(fn(None, fsts, 3, outs, None))  # NULL ctx
    assert [outs[i] for i in range(3)] == [None] * 3
    assert "null" in ko(fn(None, fsts, 3, None, None))  # NULL outs
    outs = (C.c_void_p * 3)(1, 1, 1)
    assert "null" in ko(fn(None, None, 3, outs, None))  # NULL fsts with n > 0
    assert [outs[i] for i in range(3)] == [None] * 3
    assert "null" in ko(wfst_lib.wfst_ctx_get_optimize_batch_stats(None, None, None, None, None))
    # a NULL entry is reported with its index before anything else is done with the context (zeroed memory here: no context
    # can be made without a device); the call may do no more with it than clear its counters
    ctx = C.create_string_buffer(1 << 20)
    outs = (C.c_void_p * 3)(1, 1, 1)
    assert ko(fn(C.cast(ctx, C.c_void_p), fsts, 3, outs, None)) == "item 0: null FST in batch"
    assert [outs[i] for i in range(3)] == [None] * 3 and ctx.raw == bytes(1 << 20)


def test_python_surface():
    import rustfst_amd
    for name in ("optimize_batch", "optimize_batch_stats"):
        assert name in rustfst_amd.__all__ and callable(getattr(rustfst_amd, name))
    p = inspect.signature(rustfst_amd.optimize_batch).parameters
    assert list(p) == ["fsts", "ctx", "return_in_kernel"]
    assert p["ctx"].default is None and p["return_in_kernel"].default is False
    p = inspect.signature(rustfst_amd.optimize_batch_stats).parameters
    assert list(p) == ["ctx"] and p["ctx"].default is None
    assert rustfst_amd.optimize_batch([]) == []
    res, flags = rustfst_amd.optimize_batch([], return_in_kernel=True)
    assert res == [] and flags.dtype == np.uint8 and len(flags) == 0


def test_mixed_list_reaches_every_branch(oracle):
    """the inputs of the device tests, on the CPU: sizes, words and the branch each item is in the list for"""
    items = mixed_items()
    want = {"eps": "det-min", "no-eps": "det-min", "det": "min", "trans": "encode"}
    for name, f, kind in items:
        assert 8 <= f["n_states"] <= 40, name
        if kind in want:
            assert branch_of(f, oracle) == want[kind], name
        assert bool(f["props"] & NO_EPSILONS) == (not has_eps(f)), name
        if kind in want:
            assert has_eps(f) == (kind == "eps" or (kind == "trans" and name[-1] in "02")), name
        assert is_transducer(f) == (kind == "trans"), name
        reference(name, f, oracle)
    assert reference("trims to nothing", dict((n, f) for n, f, _ in items)["trims to nothing"], oracle)["n_states"] == 0
    assert any(has_eps(f) for _, f, k in items if k == "eps") and any(has_eps(f) for _, f, k in items if k == "trans")
    assert wide_state_acceptor()["props"] & I_DETERMINISTIC and int(np.diff(wide_state_acceptor()["offsets"]).max()) == 257
    assert long_chain()["n_states"] == 4097


def has_eps(f):
    return bool(((f["arcs"]["ilabel"] == 0) & (f["arcs"]["olabel"] == 0)).any())


# ================================================================ GPU
def _batch(devs, ctx):
    import rustfst_amd
    outs, flags = rustfst_amd.optimize_batch(devs, ctx, return_in_kernel=True)
    return [o.to_flat() for o in outs], [int(x) for x in flags]


def _stats(ctx):
    import rustfst_amd
    return rustfst_amd.optimize_batch_stats(ctx)


def _raw_batch(devs, ctx):
    from rustfst_amd import _lib
    n = len(devs)
    arr = (C.c_void_p * n)(*[d._h.value if d is not None else None for d in devs])
    outs = (C.c_void_p * n)(*([1] * n))
    status = _lib.lib().wfst_optimize_batch(ctx._h, arr, n, outs, None)
    return status, [outs[i] for i in range(n)]


def _single_message(dev, ctx):
    from rustfst_amd import _lib
    out = C.c_void_p(1)
    assert _lib.lib().wfst_optimize(ctx._h, dev._h, C.byref(out)) == 1 and out.value is None
    return helpers.ko_message(1)


@pytest.mark.gpu
def test_parity_of_one_mixed_list(gpu_ctx, oracle):
    import rustfst_amd
    items = mixed_items()
    devs = [to_device(f, gpu_ctx) for _, f, _ in items]
    before = [d.to_flat() for d in devs]
    got, flags = _batch(devs, gpu_ctx)
    st = _stats(gpu_ctx)
    print("flags %s\nstats %s" % (flags, st))
    for k, ((name, flat, kind), g) in enumerate(zip(items, got)):
        same(g, reference(name, flat, oracle), f"item {k} ({name}) vs the restatement")
        same(g, devs[k].optimize().to_flat(), f"item {k} ({name}) vs the single call")
        assert flags[k] == (0 if kind == "trans" else 1), name  # small acceptors: every stage in its batch kernel
    n_trans = sum(kind == "trans" for _, _, kind in items)
    assert st["items_transducer"] == n_trans == 4
    assert st["items_in_kernel"] == len(items) - n_trans and st["items_single"] == n_trans
    assert all(st["launches"][s] >= 1 for s in STAGES)
    by = dict(zip((name for name, _, _ in items), got))
    assert by["trims to nothing"]["n_states"] == 0
    for (name, _, _), d, b in zip(items, devs, before):
        same(d.to_flat(), b, f"{name}: the input after the batch call")
    # the same handle twice, and an item between the two
    outs = rustfst_amd.optimize_batch([devs[0], devs[3], devs[0]], gpu_ctx)
    same(outs[0].to_flat(), got[0], "the same handle twice: first")
    same(outs[2].to_flat(), got[0], "the same handle twice: second")
    same(outs[1].to_flat(), got[3], "the same handle twice: between")
    assert rustfst_amd.optimize_batch([], gpu_ctx) == []


@pytest.mark.gpu
def test_k17_as_a_list(gpu_ctx, oracle):
    cases = [c for c in oc.golden_cases() if c["op"] == "optimize"]
    good = [c for c in cases if "error" not in c]
    bad = [c for c in cases if "error" in c]
    assert len(good) >= 3
    devs = [to_device(golden_flat(c), gpu_ctx) for c in good]
    got, _ = _batch(devs, gpu_ctx)
    for c, g in zip(good, got):
        assert_flat_identical(g, golden_flat(c, "expected"), c["name"])
    for c in bad:  # behind the good ones: the index in front of the single call's message
        dev = to_device(golden_flat(c), gpu_ctx)
        single = _single_message(dev, gpu_ctx)
        assert c["error"] in single
        status, outs = _raw_batch(devs + [dev], gpu_ctx)
        assert status == 1 and helpers.ko_message(1) == "item %d: %s" % (len(devs), single), c["name"]
        assert outs == [None] * (len(devs) + 1)
    again, _ = _batch(devs, gpu_ctx)
    for c, g in zip(good, again):
        assert_flat_identical(g, golden_flat(c, "expected"), c["name"] + " after the KO calls")


@pytest.mark.gpu
def test_flags_and_counts(gpu_ctx):
    items = mixed_items()
    small = [f for _, f, kind in items if kind in ("eps", "no-eps", "det")][:4]
    trans = next(f for _, f, kind in items if kind == "trans")
    listed = small + [trans, wide_state_acceptor(), long_chain()]
    devs = [to_device(f, gpu_ctx) for f in listed]
    got, flags = _batch(devs, gpu_ctx)
    st = _stats(gpu_ctx)
    print("flags %s\nstats %s" % (flags, st))
    assert flags == [1, 1, 1, 1, 0, 0, 0]
    assert st["items_transducer"] == 1 and st["items_in_kernel"] == 4 and st["items_single"] == 3
    for k, (d, g) in enumerate(zip(devs, got)):
        same(g, d.optimize().to_flat(), f"item {k} vs the single call")


@pytest.mark.gpu
def test_launches_do_not_depend_on_the_length_of_the_list(gpu_ctx):
    four = [f for _, f, kind in mixed_items() if kind == "eps"]
    assert len(four) == 4
    devs = [to_device(f, gpu_ctx) for f in four]
    got4, flags = _batch(devs, gpu_ctx)
    first = _stats(gpu_ctx)
    assert flags == [1] * 4 and all(first["launches"][s] >= 1 for s in STAGES)
    got64, flags = _batch(devs * 16, gpu_ctx)
    second = _stats(gpu_ctx)
    print("4 items %s\n64 items %s" % (first, second))
    assert flags == [1] * 64 and second["launches"] == first["launches"]
    assert second["items_in_kernel"] == 64 and first["items_in_kernel"] == 4
    for k, g in enumerate(got64):
        same(g, got4[k % 4], f"item {k} of the repeated list")


@pytest.mark.gpu
def test_ko_is_the_loop_of_single_calls(gpu_ctx):
    """the lowest failing index with the single call's message, although the stages run on sublists"""
    rng = np.random.default_rng(99)
    goods = [optimize_input(rng, int(rng.integers(8, 41)), k % 3 == 1, deterministic=(k % 3 == 2)) for k in range(8)]
    devs = [to_device(f, gpu_ctx) for f in goods]
    good, _ = _batch(devs, gpu_ctx)
    nd = nondeterministic_acceptor(rng, 12)
    no_acyclic = to_device(dict(nd, props=nd["props"] & ~ACYCLIC), gpu_ctx)  # KO on the word after tr_sum
    word = model.ACCEPTOR | I_DETERMINISTIC | NO_EPSILONS
    lying = to_device(two_state_cycle(word | ACYCLIC), gpu_ctx)  # its word sends it to minimize, which finds the cycle
    silent = to_device(two_state_cycle(word), gpu_ctx)           # ... and here minimize has to look for itself
    assert _single_message(no_acyclic, gpu_ctx) == MSG_ACYCLIC
    lying_msg, silent_msg = _single_message(lying, gpu_ctx), _single_message(silent, gpu_ctx)
    assert "cyclic" in lying_msg and "cyclic" in silent_msg

    def check(listed, want):
        status, outs = _raw_batch(listed, gpu_ctx)
        assert status == 1 and helpers.ko_message(1) == want
        assert outs == [None] * len(listed)
        for k, (g, e) in enumerate(zip(_batch(devs, gpu_ctx)[0], good)):  # a following valid call succeeds
            same(g, e, f"item {k} after the KO '{want}'")
    # item 5 lacks ACYCLIC
    check(devs[:5] + [no_acyclic] + devs[6:], "item 5: " + MSG_ACYCLIC)
    # ... and item 2 fails in a later stage: the loop of single calls reports item 2
    check(devs[:2] + [lying] + devs[3:5] + [no_acyclic] + devs[6:], "item 2: " + lying_msg)
    # a stage's own item error (minimize_batch's, at the index of its sublist) comes back with the list's index
    check(devs[:6] + [silent] + devs[7:], "item 6: " + silent_msg)
    check(devs[:2] + [silent] + devs[3:5] + [no_acyclic] + devs[6:], "item 2: " + silent_msg)
    # the argument checks come first
    status, outs = _raw_batch(devs[:5] + [no_acyclic, None] + devs[7:], gpu_ctx)
    assert status == 1 and helpers.ko_message(1) == "item 6: null FST in batch" and outs == [None] * 8
    import rustfst_amd
    other = rustfst_amd.Context(0)
    foreign = to_device(goods[3], other)
    status, outs = _raw_batch(devs[:3] + [foreign] + devs[4:], gpu_ctx)
    msg = helpers.ko_message(status)
    assert msg == "item 3: optimize_batch: the FST belongs to another context" and outs == [None] * 8
    assert _stats(gpu_ctx) == dict(launches=dict.fromkeys(STAGES, 0), items_in_kernel=0, items_single=0, items_transducer=0)
    del foreign
    for k, (g, e) in enumerate(zip(_batch(devs, gpu_ctx)[0], good)):
        same(g, e, f"item {k} after the foreign handle")


@pytest.mark.gpu
def test_the_four_batch_stages_chained_by_hand(gpu_ctx, oracle):
    import rustfst_amd
    rng = np.random.default_rng(314)
    lats = []
    while len(lats) < 12:
        f = optimize_input(rng, int(rng.integers(8, 41)), False)
        if not f["props"] & NO_EPSILONS and branch_of(f, oracle) == "det-min":
            lats.append(f)
    devs = [to_device(f, gpu_ctx) for f in lats]
    a = rustfst_amd.rm_epsilon_batch(devs, gpu_ctx)
    b = rustfst_amd.tr_sum_batch(a, gpu_ctx)
    c = rustfst_amd.determinize_batch(b, None, gpu_ctx)
    d = rustfst_amd.minimize_batch(c, None, gpu_ctx)
    got, flags = _batch(devs, gpu_ctx)
    assert flags == [1] * 12
    for k, (g, h) in enumerate(zip(got, d)):
        same(g, h.to_flat(), f"lattice {k}: the one call vs the four batch calls")
