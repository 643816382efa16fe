"""wfst_compose_batch / wfst_ctx_get_compose_batch_counters.  Without a GPU: the C-ABI and Python surface, the argument
checks that need no device, where every generator of compose_batch_cases lands, and the routing restatement's prediction
of the in_kernel flags and the seven counters for every list the device tests use.  On the device: every item of every list
against the oracle's compose(connect, compose_filter) bit for bit, the property word included, AND against
DeviceFst.compose on the same handles; flags and counters against the prediction.

Shapes, and why: pairs of 2..30 states with epsilons on both tapes of both sides (every filter decides differently);
untrimmed results of exactly S_0 = 1280 states / A_0 = 5120 arcs and one more; one level of 4031 / 4032 arcs into one state
(H_0 = 4096); 64 and 65 new states in one level (where the single call hands over and a list does not); 3 840 / 3 841
states on both sides (S_0 = 16384 / 16388); an 80 x 80 product (past S_1); 300 items: more workgroups than one wave of
blocks.

WFST_COMPOSE_BATCH_ARENA=min starts every item at S = 64, A = 128: an item whose untrimmed composition has at most 64
states and 128 arcs fits and does not grow, so the test asks for what the restatement predicts per item (most of the
list grows, some items twice) instead of a regrowth of every item."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import helpers
from helpers import FILTERS, ROOT, analyse, assert_flat_identical, ko_message, to_device
import compose_batch_cases as cases
from compose_batch_cases import COUNTERS, SIGNATURES, predict_list

ALL_FILTERS = [0] + [f.value for f in FILTERS]
ZERO = dict.fromkeys(COUNTERS, 0)
FAKE_CTX = C.c_void_p(0x1000)  # never read: the checks it passes through come before any use of the context


def same(got, exp, what):
    assert_flat_identical(got, exp, what, check_props=True)


def _c(**kw):
    return dict(ZERO, **kw)


# ================================================================ no GPU
def test_symbols_declared_exported_and_bound(wfst_lib):
    import rustfst_amd
    from rustfst_amd import _lib
    with open(os.path.join(ROOT, "include", "wfst.h")) as f:
        header = f.read()
    for name, params in SIGNATURES.items():
        assert helpers.header_params(header, name) == params
        assert hasattr(wfst_lib, name) and name in {n for n, _, _ in _lib.SYMBOLS}
    assert _lib.COMPOSE_BATCH_COUNTERS == COUNTERS and "compose_batch" not in _lib.COUNTERS
    note = re.search(r"#define\s+WFST_ABI_VERSION\s+7\b(.*)", header).group(1).split("; 6:")[0]
    assert all(name in note for name in SIGNATURES) and wfst_lib.wfst_abi_version() == 7
    assert callable(rustfst_amd.compose_batch) and callable(rustfst_amd.compose_batch_stats)
    with open(os.path.join(ROOT, "include", "wfst.hpp")) as f:
        assert "wfst_compose_batch(" in f.read()


def test_header_states_the_routing_rule():
    with open(os.path.join(ROOT, "include", "wfst.h")) as f:
        header = f.read()
    text = header[header.index("compose of a list"):header.index("wfst_status wfst_compose_batch")]
    text = " ".join(text.replace("\n *", " ").split())
    for words in ("16384", "3840", "start state", "occupies no workgroup", "4 * max(min(n_states1, n_states2), 64) + 1024",
                  "A_k = 4 * S_k", "2 * S_k + 128", "more than 64 new states", "8 GiB", "WFST_COMPOSE_BATCH_ARENA=min",
                  "S = 64 and A = 128", "the lowest failing index wins"):
        assert words in text, words


def test_arguments_are_refused_before_any_device_work(wfst_lib):
    from rustfst_amd import _lib
    two, three = (C.c_void_p * 2)(), (C.c_void_p * 3)()

    def outs():
        return (C.c_void_p * 3)(1, 2, 3)
    o = outs()
    assert ko_message(wfst_lib.wfst_compose_batch(None, two, 2, two, 2, None, o, None)) == "null pointer" and list(o) == [None, None, 3]
    o = outs()
    assert ko_message(wfst_lib.wfst_compose_batch(FAKE_CTX, None, 3, three, 3, None, o, None)) == "null pointer" and list(o) == [None] * 3
    o = outs()
    assert ko_message(wfst_lib.wfst_compose_batch(FAKE_CTX, three, 3, None, 3, None, o, None)) == "null pointer" and list(o) == [None] * 3
    assert ko_message(wfst_lib.wfst_compose_batch(FAKE_CTX, two, 2, two, 2, None, None, None)) == "null pointer"
    o = outs()
    msg = "compose_batch: the lists hold 2 and 3 FSTs (equal lengths, or one of them 1)"
    assert ko_message(wfst_lib.wfst_compose_batch(FAKE_CTX, two, 2, three, 3, None, o, None)) == msg and list(o) == [None] * 3
    assert "hold 0 and 1 FSTs" in ko_message(wfst_lib.wfst_compose_batch(FAKE_CTX, two, 0, three, 1, None, outs(), None))
    o = outs()
    cfg = _lib.ComposeConfig(7, 1)
    assert ko_message(wfst_lib.wfst_compose_batch(FAKE_CTX, three, 3, three, 3, C.byref(cfg), o, None)) == "unknown compose_filter"
    assert list(o) == [None] * 3
    o = outs()  # a NULL entry, behind the filter check
    assert ko_message(wfst_lib.wfst_compose_batch(FAKE_CTX, three, 3, three, 1, None, o, None)) == "item 0: null FST in batch"
    assert list(o) == [None] * 3
    o = outs()  # n == 0: OK, nothing is touched
    assert wfst_lib.wfst_compose_batch(FAKE_CTX, two, 0, two, 0, None, o, None) == 0 and list(o) == [1, 2, 3]
    helpers.null_ctx_is_ko(wfst_lib, "wfst_ctx_get_compose_batch_counters", len(COUNTERS))


def test_python_refuses_matcher_configs():
    import rustfst_amd
    from rustfst_amd import ComposeConfig, ComposeFilter, MatcherConfig
    cfg = ComposeConfig(ComposeFilter.SEQUENCEFILTER, True, matcher1_config=MatcherConfig(5))
    with pytest.raises(rustfst_amd.WfstError, match="MatcherConfig"):
        rustfst_amd.compose_batch([], [], cfg)


def test_generators_sit_on_their_limits(oracle):
    sizes = {k: (analyse(oracle, *cases.arena_case(k))["full"]["n_states"], len(analyse(oracle, *cases.arena_case(k))["full"]["arcs"]))
             for k in cases.ARENA_CASES}
    s0, a0 = cases.compose_caps(1, 1280)
    assert (s0, a0, cases.hash_slots(s0)) == (1280, 5120, 4096)
    assert sizes["S"] == (s0, s0 - 1) and sizes["S+1"] == (s0 + 1, s0)
    assert sizes["A"] == (1025, a0) and sizes["A+1"] == (1025, a0 + 1)
    assert sizes["H"] == (2, 4031) and sizes["H+1"] == (2, 4032) and 1 + 4031 + 64 == cases.hash_slots(s0)
    # width: 64 and 65 new states in the first level
    assert [analyse(oracle, *cases.new_states_case(m))["levels"][0][2:] for m in (64, 65)] == [(64, 64), (65, 65)]
    # hand-over: S_0 on both sides of 16384; the product passes S_0 and S_1 on states and S_2 is beyond the kernel
    (s3841, ring), (s3840, _), (pa, pb), _ = cases.handover_list()
    assert (s3841["n_states"], s3840["n_states"], ring["n_states"]) == (3841, 3840, 3841)
    assert cases.compose_caps(3841, 3841)[0] == 16388 and cases.compose_caps(3840, 3841)[0] == 16384 == cases.WIDE_STATES
    assert analyse(oracle, s3840, ring)["full"]["n_states"] == 3840 and analyse(oracle, s3841, ring)["full"]["n_states"] == 3841
    full = analyse(oracle, pa, pb)["full"]
    s_p = cases.compose_caps(80, 80)[0]
    assert full["n_states"] == 6400 and s_p == 1344 and 4 * s_p < 6400 and 16 * s_p > cases.WIDE_STATES
    assert max(lv[3] for lv in analyse(oracle, pa, pb)["levels"]) > cases.WAVE  # (levels wider than one wave on the way)
    # the degenerate items are what they say
    d = cases.degenerate_list()
    assert [cases.has_start(a) and cases.has_start(b) for a, b in d] == [True, False, True, False, False, True, True, True, True, True]
    assert d[4][0]["n_states"] == 0 and analyse(oracle, *d[6])["trim"]["n_states"] == 0 < analyse(oracle, *d[6])["full"]["n_states"]
    assert analyse(oracle, *d[7])["full"]["n_states"] == 1
    # the random pairs: epsilons on both tapes of both sides, non-empty results among them
    ra = np.concatenate([a["arcs"] for a, _ in cases.random_pairs()])
    rb = np.concatenate([b["arcs"] for _, b in cases.random_pairs()])
    assert all((x[k] == 0).any() for x in (ra, rb) for k in ("ilabel", "olabel"))
    assert sum(analyse(oracle, a, b)["trim"]["n_states"] > 1 for a, b in cases.random_pairs()) >= 20
    assert len(cases.many_small()) == 300 and len({id(b) for _, b in cases.many_small()}) == 100


def test_predicted_flags_and_counters(oracle):
    """the restatement on both sides of every limit, for every list the device tests send"""
    n = len(cases.main_list())
    for flt in ALL_FILTERS:
        assert predict_list(oracle, cases.main_list(), flt) == ([1] * n, _c(launches=1, items_in_kernel=n))
    flags, c = predict_list(oracle, cases.degenerate_list())
    assert flags == [1] * 10 and c == _c(launches=1, items_in_kernel=10, items_no_start=3)
    flags, c = predict_list(oracle, cases.width_list())
    assert flags == [1, 1, 1] and c == _c(launches=1, items_in_kernel=3)
    flags, c = predict_list(oracle, cases.arena_list())
    assert flags == [1] * 6 and c == _c(launches=2, items_in_kernel=6, regrown_states=1, regrown_arcs=1, regrown_hash=1)
    for k, name in enumerate(cases.ARENA_CASES):  # each twin beside a small item: the ON-limit ones do not regrow
        _, c = predict_list(oracle, [cases.arena_case(name), cases.random_pairs()[0]])
        grown = {"S+1": "regrown_states", "A+1": "regrown_arcs", "H+1": "regrown_hash"}.get(name)
        assert c == _c(launches=2 if grown else 1, items_in_kernel=2, **({grown: 1} if grown else {})), name
    flags, c = predict_list(oracle, cases.handover_list())
    assert flags == [0, 1, 0, 1] and c == _c(launches=2, items_in_kernel=2, items_single=2, regrown_states=2)
    flags, c = predict_list(oracle, cases.many_small())
    assert flags == [1] * 300 and c == _c(launches=1, items_in_kernel=300)
    # a list of one, and a list with one item that has start states: the single call
    assert predict_list(oracle, cases.main_list()[:1]) == ([0], _c(items_single=1))
    d = cases.degenerate_list()
    assert predict_list(oracle, [d[1], d[0], d[3]]) == ([1, 0, 1], _c(items_in_kernel=2, items_single=1, items_no_start=2))
    assert predict_list(oracle, [d[1]]) == ([1], _c(items_in_kernel=1, items_no_start=1))
    # the smallest arenas: what fits 64 states and 128 arcs stays, the rest grows (some twice)
    flags, c = predict_list(oracle, cases.main_list(), arena_min=True)
    fits = [analyse(oracle, a, b)["full"]["n_states"] <= 64 and len(analyse(oracle, a, b)["full"]["arcs"]) <= 128 for a, b in cases.main_list()]
    assert flags == [1] * n and c["regrown_hash"] == 0 and c["regrown_states"] + c["regrown_arcs"] >= n - sum(fits) >= n // 2
    assert c["launches"] >= 2
    assert cases.wave_status([(0, 1, 10, 3)], 3, 128) == "states" and cases.wave_status([(0, 1, 10, 2)], 3, 128) == "ok"
    assert cases.wave_status([(0, 1, 65, 65), (1, 66, 65, 1)], 1280, 5120) == "ok"  # no width hand-over


# ================================================================ GPU
def _stats(ctx):
    import rustfst_amd
    st = rustfst_amd.compose_batch_stats(ctx)
    assert tuple(st) == COUNTERS
    return st


def upload(ctx, pairs):
    """one handle per distinct flat FST"""
    seen = {}
    def h(f):
        if id(f) not in seen:
            seen[id(f)] = to_device(f, ctx)
        return seen[id(f)]
    return [h(a) for a, _ in pairs], [h(b) for _, b in pairs]


def run_list(ctx, oracle, pairs, what, flt=0, connects=(True, False), handles=None, arena_min=False, single=True, forms=None):
    """ONE call for the list: every item against the oracle and against the single call on the same handles, the flags and
    the counters against the prediction"""
    import rustfst_amd
    from rustfst_amd import ComposeConfig, ComposeFilter
    h1, h2 = handles or upload(ctx, pairs)
    a1, a2 = forms or (h1, h2)
    want_flags, want = predict_list(oracle, pairs, flt, arena_min)
    for connect in connects:
        cfg = ComposeConfig(ComposeFilter(flt), connect=connect)
        outs, flags = rustfst_amd.compose_batch(a1, a2, cfg, ctx, return_in_kernel=True)
        st = _stats(ctx)
        print("%s filter=%d connect=%s: %s" % (what, flt, connect, st))
        assert len(outs) == len(pairs)
        for i, (a, b) in enumerate(pairs):
            at = "%s filter=%d connect=%s item %d" % (what, flt, connect, i)
            got = outs[i].to_flat()
            same(got, analyse(oracle, a, b, flt)["trim" if connect else "full"], at)
            if single:
                same(got, h1[i].compose(h2[i], cfg).to_flat(), at + " against the single call")
        assert flags.tolist() == want_flags and st == want, (what, flt, connect, flags.tolist(), st, want)
    return h1, h2


@pytest.mark.gpu
@pytest.mark.parametrize("flt", ALL_FILTERS)
def test_known_answers_and_random_pairs(gpu_ctx, oracle, flt):
    """the K1 pair, fst![1,2=>2,3] o fst![2,3=>3,4] and 40 random pairs, connect on and off, each as ONE call"""
    import rustfst_amd
    h1, h2 = run_list(gpu_ctx, oracle, cases.main_list(), "main", flt)
    if flt == 0:  # the stored vector itself, and cfg == NULL
        outs = rustfst_amd.compose_batch(h1, h2, None, gpu_ctx)
        exp = cases.k1_expected()
        got = outs[0].to_flat()
        assert_flat_identical(got, dict(exp, props=got["props"]), "K1 expected", check_props=False)
        for i, (a, b) in enumerate(cases.main_list()):
            same(outs[i].to_flat(), analyse(oracle, a, b)["trim"], "cfg == NULL item %d" % i)


@pytest.mark.gpu
def test_the_three_list_forms_and_a_list_of_one(gpu_ctx, oracle):
    import rustfst_amd
    pairs = cases.random_pairs()[:8]
    run_list(gpu_ctx, oracle, pairs, "n1 == n2")
    one_b = [(a, pairs[0][1]) for a, _ in pairs]
    h1, h2 = upload(gpu_ctx, one_b)
    run_list(gpu_ctx, oracle, one_b, "n2 == 1", handles=(h1, h2), forms=(h1, h2[:1]))
    run_list(gpu_ctx, oracle, one_b, "n2 a single handle", handles=(h1, h2), forms=(h1, h2[0]), connects=(True,))
    one_a = [(pairs[3][0], b) for _, b in pairs]
    h1, h2 = upload(gpu_ctx, one_a)
    run_list(gpu_ctx, oracle, one_a, "n1 == 1", handles=(h1, h2), forms=(h1[:1], h2))
    run_list(gpu_ctx, oracle, pairs[:1], "n == 1")
    assert _stats(gpu_ctx) == _c(items_single=1)
    assert rustfst_amd.compose_batch([], [], None, gpu_ctx) == []


@pytest.mark.gpu
def test_degenerate_items_inside_a_list(gpu_ctx, oracle):
    d = cases.degenerate_list()
    run_list(gpu_ctx, oracle, d, "degenerate")
    run_list(gpu_ctx, oracle, [d[1], d[0], d[3]], "one item with start states")
    run_list(gpu_ctx, oracle, [d[1]], "only an item without a start state")


@pytest.mark.gpu
def test_levels_of_64_and_65_new_states_stay_in_the_list(gpu_ctx, oracle):
    h1, h2 = run_list(gpu_ctx, oracle, cases.width_list(), "width")
    assert _stats(gpu_ctx)["items_single"] == 0
    h1[1].compose(h2[1])
    assert gpu_ctx.compose_path_stats()["switched_wide"] == 1  # the single call hands this one over


@pytest.mark.gpu
def test_growth_at_every_capacity(gpu_ctx, oracle):
    run_list(gpu_ctx, oracle, cases.arena_list(), "arena")
    assert _stats(gpu_ctx) == _c(launches=2, items_in_kernel=6, regrown_states=1, regrown_arcs=1, regrown_hash=1)
    small = cases.random_pairs()[0]
    for name in cases.ARENA_CASES:
        run_list(gpu_ctx, oracle, [cases.arena_case(name), small], "arena " + name, connects=(True,), single=False)


@pytest.mark.gpu
def test_every_item_starts_at_the_smallest_arena(gpu_ctx, oracle, monkeypatch):
    monkeypatch.setenv("WFST_COMPOSE_BATCH_ARENA", "min")
    run_list(gpu_ctx, oracle, cases.main_list(), "arena=min", single=False, arena_min=True)
    st = _stats(gpu_ctx)
    assert st["launches"] >= 2 and st["regrown_states"] + st["regrown_arcs"] >= len(cases.main_list()) // 2
    monkeypatch.setenv("WFST_COMPOSE_BATCH_ARENA", "max")
    import rustfst_amd
    h1, h2 = upload(gpu_ctx, cases.random_pairs()[:2])
    with pytest.raises(rustfst_amd.WfstError, match="WFST_COMPOSE_BATCH_ARENA: expected min"):
        rustfst_amd.compose_batch(h1, h2, None, gpu_ctx)


@pytest.mark.gpu
def test_hand_over_to_the_wide_driver(gpu_ctx, oracle):
    run_list(gpu_ctx, oracle, cases.handover_list(), "hand-over", connects=(True,))
    assert _stats(gpu_ctx) == _c(launches=2, items_in_kernel=2, items_single=2, regrown_states=2)


@pytest.mark.gpu
def test_300_items_in_one_call(gpu_ctx, oracle):
    run_list(gpu_ctx, oracle, cases.many_small(), "300 items", connects=(True,), single=False)
    assert _stats(gpu_ctx)["launches"] == 1


@pytest.mark.gpu
def test_ko_leaves_nothing_behind(gpu_ctx, oracle):
    import rustfst_amd
    from rustfst_amd import _lib, synth
    pairs = cases.random_pairs()[:8]
    h1, h2 = upload(gpu_ctx, pairs)
    bad = dict(pairs[2][0], props=helpers.NOT_O_LABEL_SORTED | synth.I_LABEL_SORTED)
    bad_b = dict(pairs[2][1], props=helpers.NOT_I_LABEL_SORTED | synth.O_LABEL_SORTED)
    u1, u2 = list(h1), list(h2)
    u1[2] = u1[5] = to_device(bad, gpu_ctx)
    u2[2] = u2[5] = to_device(bad_b, gpu_ctx)
    other = rustfst_amd.Context(0)
    foreign = list(h1)
    foreign[4] = to_device(pairs[4][0], other)
    lib = _lib.lib()

    def call(l1, l2):
        n = len(l1)
        outs = (C.c_void_p * n)(*[7] * n)
        arr1 = (C.c_void_p * n)(*[None if f is None else f._h.value for f in l1])
        arr2 = (C.c_void_p * n)(*[None if f is None else f._h.value for f in l2])
        msg = ko_message(lib.wfst_compose_batch(gpu_ctx._h, arr1, n, arr2, n, None, outs, None))
        assert list(outs) == [None] * n
        return msg

    run_list(gpu_ctx, oracle, pairs, "before", connects=(True,), handles=(h1, h2), single=False)
    good = _stats(gpu_ctx)
    msg = call(u1, u2)
    assert msg.startswith("item 2: ComposeFst: ") and "(sort?)" in msg
    assert call(foreign, h2) == "item 4: compose_batch: the FST belongs to another context"
    holes = list(h1)
    holes[3] = None
    assert call(holes, h2) == "item 3: null FST in batch"
    assert _stats(gpu_ctx) == good  # a call that refuses its arguments leaves the counters alone
    run_list(gpu_ctx, oracle, pairs, "after", connects=(True,), handles=(h1, h2), single=False)


@pytest.mark.gpu
def test_inputs_untouched_and_outputs_own_their_memory(gpu_ctx, oracle):
    import rustfst_amd
    pairs = cases.random_pairs()[:6] + [cases.arena_case("S+1")]
    h1, h2 = upload(gpu_ctx, pairs)
    before = [(a.to_flat(), b.to_flat()) for a, b in zip(h1, h2)]
    outs = rustfst_amd.compose_batch(h1, h2, None, gpu_ctx)
    for (a0, b0), a, b in zip(before, h1, h2):
        same(a.to_flat(), a0, "first operand after the call")
        same(b.to_flat(), b0, "second operand after the call")
    keep = outs[3]
    del h1, h2, a, b
    del outs
    import gc
    gc.collect()
    same(keep.to_flat(), analyse(oracle, *pairs[3])["trim"], "the one output left")


@pytest.mark.gpu
def test_pipelines_equal_the_loops_of_single_calls(gpu_ctx, oracle):
    """compose_batch -> top_sort_batch -> optimize_batch, and compose_batch -> shortest_path_batch(nshortest = 3)"""
    import rustfst_amd
    from rustfst_amd import ShortestPathConfig
    rng = np.random.default_rng(7900)
    g = helpers.random_fst_flat(rng, 12, 3, 4, p_final=0.4, sort="ilabel", weight_grid=4, max_w=20, min_fanout=1)
    g["arcs"]["olabel"] = g["arcs"]["ilabel"]  # an acceptor: what optimize takes
    lats = []
    for k in range(12):
        labels = helpers.walk_labels(rng, g, 0, "ilabel", 3 + k % 5)
        alt = labels.copy()
        alt[-1] = 1 + (int(alt[-1]) % 4)
        L = len(labels)
        rows = [[(int(labels[i]), int(labels[i]), 0.25 * (i % 3), i + 1)] + ([(int(alt[i]), int(alt[i]), 0.5, i + 1)] if i == L - 1 and alt[i] != labels[i] else [])
                for i in range(L)] + [[]]
        rows = [sorted(r, key=lambda a: a[1]) for r in rows]
        lats.append(helpers.fst(rows, helpers.finals_of(L + 1, {L: 0.25})))
    hl, hg = [to_device(f, gpu_ctx) for f in lats], to_device(g, gpu_ctx)
    comps = rustfst_amd.compose_batch(hl, hg, None, gpu_ctx)
    singles = [h.compose(hg) for h in hl]
    for i, (c, s) in enumerate(zip(comps, singles)):
        same(c.to_flat(), s.to_flat(), "composition %d" % i)
    cfg = ShortestPathConfig(nshortest=3)
    for i, (p, s) in enumerate(zip(rustfst_amd.shortest_path_batch(comps, cfg, gpu_ctx), singles)):
        same(p.to_flat(), s.shortest_path(cfg).to_flat(), "3 best paths of composition %d" % i)
    acyclic = [i for i, s in enumerate(singles) if s.top_sort().to_flat()["props"] & rustfst_amd.synth.ACYCLIC]
    assert len(acyclic) >= 6
    opt = rustfst_amd.optimize_batch(rustfst_amd.top_sort_batch([comps[i] for i in acyclic], gpu_ctx), gpu_ctx)
    for k, i in enumerate(acyclic):
        same(opt[k].to_flat(), singles[i].top_sort().optimize().to_flat(), "optimized composition %d" % i)


@pytest.mark.gpu
def test_counter_getter(gpu_ctx, oracle, wfst_lib):
    import rustfst_amd
    helpers.check_counter_getter(wfst_lib, "wfst_ctx_get_compose_batch_counters", COUNTERS, rustfst_amd.compose_batch_stats)
    run_list(gpu_ctx, oracle, cases.handover_list() + [cases.degenerate_list()[1]], "counters", connects=(True,), single=False)
    want = _stats(gpu_ctx)
    assert want == _c(launches=2, items_in_kernel=3, items_single=2, items_no_start=1, regrown_states=2)
    fn = wfst_lib.wfst_ctx_get_compose_batch_counters
    for k, name in enumerate(COUNTERS):  # each pointer alone receives its counter
        v = C.c_uint64(99)
        args = [None] * len(COUNTERS)
        args[k] = C.byref(v)
        assert fn(gpu_ctx._h, *args) == 0 and v.value == want[name], name
    assert fn(gpu_ctx._h, *[None] * len(COUNTERS)) == 0
    run_list(gpu_ctx, oracle, cases.random_pairs()[:3], "reset", connects=(True,), single=False)
    assert _stats(gpu_ctx) == _c(launches=1, items_in_kernel=3)  # reset when a call begins
    two, o = (C.c_void_p * 2)(), (C.c_void_p * 3)()
    assert wfst_lib.wfst_compose_batch(gpu_ctx._h, two, 2, o, 3, None, o, None) == 1
    assert _stats(gpu_ctx) == _c(launches=1, items_in_kernel=3)  # ... and left alone by a call that refuses its arguments
