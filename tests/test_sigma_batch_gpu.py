"""The fused batch with a sigma matcher on the device (compose_sigma_batch.hip through
wfst_compose_shortest_path_batch_with_matchers): every result is bit for bit the oracle's shortest path of the sequential
restatement's composition (tests/sigma_ref.py), property word included, and the counters of
wfst_ctx_get_sigma_batch_counters are read after every call.  K21's three utterances, the seeded batches of
tests/sigma_batch_cases.py, the limits of string_sigma_sp_kernel one state to either side, the routes, the errors and what
follows them, the degenerate inputs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rustfst_amd
from rustfst_amd import ComposeConfig, ComposeFilter, MatcherConfig, MatcherRewriteMode, WfstError, _lib

from oracle.model import I_LABEL_SORTED, O_LABEL_SORTED

import helpers
from helpers import dev
import sigma_batch_cases as B
import sigma_cases as S
import sigma_ref as R

pytestmark = pytest.mark.gpu
INF = np.inf
BAD_LABEL = "SigmaMatcher::Find: bad label (sigma)"
ITEM_COUNTERS = ("exact_items", "sigma_items", "sigma_arcs", "refused_items")


def matcher(m):
    return None if m is None else MatcherConfig(m[0], MatcherRewriteMode(m[1]), m[2])


def run_batch(ctx, strs, t, m2, flt=R.SEQUENCE, connect=True, m1=None, handles=None):
    """([flat results], composed arcs, counters) or (KO message, None, counters)"""
    cfg = ComposeConfig(ComposeFilter(flt), connect, matcher(m1), matcher(m2))
    accs = handles or [dev(a, ctx) for a in strs]
    try:
        outs, n_arcs = rustfst_amd.compose_shortest_path_batch(accs, dev(t, ctx), cfg, ctx=ctx)
    except WfstError as e:
        return str(e).split(": ", 1)[1], None, ctx.sigma_batch_stats()
    return [o.to_flat() for o in outs], n_arcs, ctx.sigma_batch_stats()


def check_batch(ctx, oracle, strs, t, m2, what, refs=None, flt=R.SEQUENCE, m1=None, connect=True, kernel=None):
    """one call against the restatement: results in item order, composed arcs, and every counter; `kernel`: may the kernel
    see items at all (False: another filter, a matcher on side 1, T with input epsilons); returns the counters"""
    refs = refs or [B.reference(a, t, m2, flt, m1) for a in strs]
    got, n_arcs, st = run_batch(ctx, strs, t, m2, flt, connect, m1)
    assert not isinstance(got, str), (what, got)
    assert len(got) == len(strs)
    exp = dict.fromkeys(_lib.SIGMA_BATCH_COUNTERS, 0)
    for i, (a, (c, info, widths)) in enumerate(zip(strs, refs)):
        want = B.expected_path(oracle, R.compose_sigma(a, t, flt, connect, m1, m2))
        helpers.assert_flat_identical(got[i], want, "%s item %d" % (what, i))
        string = kernel is not False and is_string(a)
        if not string:
            exp["items_loop"] += 1
        elif not B.in_kernel(info, widths):
            exp["items_handed_back"] += 1
        else:
            exp["items_in_kernel"] += 1
            for k in ITEM_COUNTERS:
                exp[k] += info[k]
            exp["max_level_width"] = max(exp["max_level_width"], max(widths))
    exp["launches"] = 1 if exp["items_in_kernel"] + exp["items_handed_back"] else 0
    assert st == exp, (what, st, exp)
    assert n_arcs == sum(info["arcs"] for _, info, _ in refs), what
    return st


def is_string(a):
    """utils::acceptor's shape: a chain from state 0, one arc per state, ilabel == olabel != 0, only the last state final"""
    rows, n = a["rows"], len(a["rows"])
    return (a["start"] == 0 and n >= 1 and not rows[n - 1] and a["finals"][n - 1] is not None and
            all(len(rows[s]) == 1 and rows[s][0][3] == s + 1 and rows[s][0][0] == rows[s][0][1] != 0 and a["finals"][s] is None
                for s in range(n - 1)))


def k21_still_works(ctx, oracle):
    strs, g, m2 = B.k21_batch()
    st = check_batch(ctx, oracle, strs, g, m2, "k21 after a KO")
    assert st["launches"] == 1 and st["items_in_kernel"] == 3


# ---------------------------------------------------------------- K21 and the seeded batches
def test_k21_three_utterances_in_one_launch(gpu_ctx, oracle):
    """fails without the feature: the parent has no such symbol and ComposeConfig._c() refuses the matcher config"""
    strs, g, m2 = B.k21_batch()
    for connect in (False, True):
        st = check_batch(gpu_ctx, oracle, strs, g, m2, "k21 connect=%s" % connect, connect=connect)
        assert (st["launches"], st["items_in_kernel"], st["items_handed_back"], st["items_loop"]) == (1, 3, 0, 0)
        assert (st["sigma_items"], st["refused_items"], st["exact_items"], st["max_level_width"]) == (2, 1, 5, 1)
    got, _, _ = run_batch(gpu_ctx, strs, g, m2)
    assert [f["n_states"] for f in got] == [0, 4, 4]  # "Bowie should NOT match"


@pytest.mark.parametrize("index", range(18))
def test_seeded_batches(gpu_ctx, oracle, index):
    name, strs, t, m2 = B.seeded_cases()[index]
    st = check_batch(gpu_ctx, oracle, strs, t, m2, name, refs=B.seeded_references()[name], connect=index % 2 == 0)
    assert st["launches"] == 1 and 4 * (st["items_loop"] + st["items_handed_back"]) <= len(strs)


def test_cpp_sigma_batch_tests_run(gpu_ctx, tmp_path):
    """examples/sigma_batch_tests.cpp: play X please for three utterances against include/wfst.hpp, end to end"""
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = tmp_path / "sigma_batch"
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(helpers.ROOT, "include"),
                    os.path.join(helpers.ROOT, "examples", "sigma_batch_tests.cpp"), "-L", libdir, "-lwfst_amd",
                    f"-Wl,-rpath,{libdir}", "-Wl,--allow-shlib-undefined", "-o", str(exe)], check=True)
    env = dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all sigma-batch tests passed" in r.stdout, r.stdout + r.stderr


# ---------------------------------------------------------------- dedup, ties and the limits
def test_tie_keeps_the_first_parent_in_emission_order(gpu_ctx, oracle):
    got, _, st = run_batch(gpu_ctx, [B.weighted_string([2, 9])], B.tie_grammar(), (B.SG, 2, None))
    check_batch(gpu_ctx, oracle, [B.weighted_string([2, 9])], B.tie_grammar(), (B.SG, 2, None), "tie")
    assert st["items_in_kernel"] == 1 and st["max_level_width"] == 2
    assert sorted(got[0]["arcs"]["olabel"].tolist()) == [2, 5]  # (through state 1, whose sigma arc says 5)


def test_level_of_64_states_and_65(gpu_ctx, oracle):
    st = check_batch(gpu_ctx, oracle, [B.weighted_string([7])], B.fan_grammar(64), (B.SG, 0, None), "64 wide")
    assert (st["items_in_kernel"], st["items_handed_back"], st["max_level_width"], st["sigma_arcs"]) == (1, 0, 64, 64)
    st = check_batch(gpu_ctx, oracle, [B.weighted_string([7])], B.fan_grammar(65), (B.SG, 0, None), "65 wide")
    assert (st["items_in_kernel"], st["items_handed_back"], st["launches"]) == (0, 1, 1)
    st = check_batch(gpu_ctx, oracle, [B.weighted_string([7])], B.fan_grammar(70, 10), (B.SG, 0, None), "70 sigma arcs, 10 states")
    assert (st["items_in_kernel"], st["max_level_width"], st["sigma_arcs"]) == (1, 10, 70)


def test_composed_states_at_the_slice_and_one_beyond(gpu_ctx, oracle):
    st = check_batch(gpu_ctx, oracle, [B.weighted_string(B.SLICE_STRING)], B.slice_grammar(57), (B.SG, 0, None), "slice")
    assert (st["items_in_kernel"], st["items_handed_back"]) == (1, 0)
    st = check_batch(gpu_ctx, oracle, [B.weighted_string(B.SLICE_STRING)], B.slice_grammar(56), (B.SG, 0, None), "slice + 1")
    assert (st["items_in_kernel"], st["items_handed_back"]) == (0, 1)


@pytest.mark.parametrize("n_arcs,sigma_first", [(65, True), (65, False), (200, True), (200, False)])
def test_arc_blocks_longer_than_a_chunk(gpu_ctx, oracle, n_arcs, sigma_first):
    t, sigma = B.long_block_grammar(n_arcs, sigma_first)
    labels = sorted({a[0] for a in t["rows"][0]} - {sigma})
    # the run across the chunk boundary, the block's first, last and 64th label, and labels only sigma answers
    strs = [B.weighted_string([l]) for l in (300, labels[0], labels[-1], t["rows"][0][64][0] if t["rows"][0][64][0] != sigma else 300, 7, 9999)]
    exact = 4 if 300 in labels else 2  # (65 arcs with sigma at the tail: the block ends before the run, sigma answers 300)
    for rw in (0, 2):
        st = check_batch(gpu_ctx, oracle, strs, t, (sigma, rw, None), "%d arcs rw=%d" % (n_arcs, rw))
        assert st["items_in_kernel"] == len(strs) and (st["exact_items"], st["sigma_items"], st["sigma_arcs"]) == (exact, 6 - exact, 3 * (6 - exact))


# ---------------------------------------------------------------- routes
def test_routes_keep_item_order(gpu_ctx, oracle):
    strs, g, m2 = B.k21_batch()
    mixed = [strs[1], B.nonlinear_acceptor(), strs[0], strs[2]]
    st = check_batch(gpu_ctx, oracle, mixed, g, m2, "a non-linear acceptor among strings")
    assert (st["items_loop"], st["items_in_kernel"], st["launches"]) == (1, 3, 1)
    st = check_batch(gpu_ctx, oracle, strs, g, m2, "m1 given", m1=(99, 0, None), kernel=False)
    assert (st["items_loop"], st["launches"]) == (3, 0)
    for flt in (R.NULL, R.TRIVIAL, R.ALT_SEQUENCE, R.MATCH, R.NO_MATCH):
        st = check_batch(gpu_ctx, oracle, strs, g, m2, "filter %d" % flt, flt=flt, kernel=False)
        assert (st["items_loop"], st["launches"]) == (3, 0)
    g_eps = S.machine([[(0, 8, 0.5, 1), (2, 2, 0.0, 1)], [(1, 1, 0.0, 2)], [(5, 5, 0.0, 3)], []], [INF, INF, INF, 0.0])
    st = check_batch(gpu_ctx, oracle, strs, g_eps, m2, "T with an input epsilon", kernel=False)
    assert (st["items_loop"], st["launches"]) == (3, 0)


def test_no_label_is_the_plain_batch(gpu_ctx, oracle):
    name, strs, t, m2 = B.seeded_cases()[1]
    handles = [dev(a, gpu_ctx) for a in strs]
    plain, plain_arcs = rustfst_amd.compose_shortest_path_batch(handles, dev(t, gpu_ctx), ComposeConfig(ComposeFilter.SEQUENCEFILTER), ctx=gpu_ctx)
    got, n_arcs, st = run_batch(gpu_ctx, strs, t, (R.NO_LABEL, 1, [3]), handles=handles)
    assert (st["items_in_kernel"], st["launches"], n_arcs) == (len(strs), 1, plain_arcs)
    assert sum(st[k] for k in ITEM_COUNTERS) == 0
    for i, p in enumerate(plain):
        helpers.assert_flat_identical(got[i], p.to_flat(), "NO_LABEL item %d" % i)
    # no matcher config at all through the new symbol: wfst_compose_shortest_path_batch, call for call
    before = gpu_ctx.sigma_batch_stats()
    arr = rustfst_amd.fst.HandleArray(handles)._arr
    outs, na = (C.c_void_p * len(strs))(), C.c_uint64()
    cfg = _lib.ComposeConfig(3, 1)
    assert _lib.lib().wfst_compose_shortest_path_batch_with_matchers(gpu_ctx._h, arr, len(strs), dev(t, gpu_ctx)._h, C.byref(cfg), None, None,
                                                                     None, outs, C.byref(na)) == 0
    for i, p in enumerate(plain):
        helpers.assert_flat_identical(rustfst_amd.DeviceFst(C.c_void_p(outs[i]), gpu_ctx).to_flat(), p.to_flat(), "forwarded item %d" % i)
    assert na.value == plain_arcs and gpu_ctx.sigma_batch_stats() == before and gpu_ctx.compose_path_stats()["string_answered"] == len(strs)


# ---------------------------------------------------------------- errors, and the context after them
def raw_call(ctx, accs, t, flt, m1, m2):
    """through the C-ABI: (status, [outs as integers or None])"""
    n = len(accs)
    arr = rustfst_amd.fst.HandleArray(accs)._arr
    outs = (C.c_void_p * n)(*[7] * n)
    cfg = _lib.ComposeConfig(flt, 1)
    c1, c2 = matcher(m1), matcher(m2)
    status = _lib.lib().wfst_compose_shortest_path_batch_with_matchers(ctx._h, arr, n, t._h, C.byref(cfg), c1._c() if c1 else None,
                                                                       c2._c() if c2 else None, None, outs, None)
    return status, [outs[i] for i in range(n)]


def test_errors_leave_every_out_null_and_the_context_working(gpu_ctx, oracle):
    strs, g, m2 = B.k21_batch()
    dg = dev(g, gpu_ctx)
    good, bad = S.chain_query([2, 3, 5]), S.chain_query([2, 1, 5])  # sigma at a position state 1 of the grammar reaches
    unreached = S.chain_query([7, 1, 5])  # ... and at one nothing reaches: "play" is the grammar's only way out of its start
    assert B.reference(bad, g, m2)[0] == BAD_LABEL and not isinstance(B.reference(unreached, g, m2)[0], str)
    status, outs = raw_call(gpu_ctx, [dev(a, gpu_ctx) for a in (good, bad, good)], dg, 3, None, m2)
    assert helpers.ko_message(status) == BAD_LABEL and outs == [None] * 3
    assert gpu_ctx.sigma_batch_stats()["launches"] == 1
    k21_still_works(gpu_ctx, oracle)
    st = check_batch(gpu_ctx, oracle, [good, unreached], g, m2, "sigma where nothing reaches")
    assert st["items_in_kernel"] == 2
    # a failing item on the loop route in front of a failing item of the kernel, and behind it: the message is the same, and
    # every out is null either way
    loop_bad = S.machine([[(2, 2, 0.0, 1), (2, 2, 0.5, 2)], [(1, 1, 0.0, 3)], [(3, 3, 0.0, 3)], [(5, 5, 0.0, 4)], []], [INF] * 4 + [0.0])
    assert B.reference(loop_bad, g, m2)[0] == BAD_LABEL
    for order in ((good, loop_bad, bad), (good, bad, loop_bad)):
        status, outs = raw_call(gpu_ctx, [dev(a, gpu_ctx) for a in order], dg, 3, None, m2)
        assert helpers.ko_message(status) == BAD_LABEL and outs == [None] * 3
    k21_still_works(gpu_ctx, oracle)
    # two failing items with different messages (both on the loop route: the other message needs a matcher on side 1)
    b = S.machine([[(1, 1, 0.0, 1), (2, 2, 0.0, 2)], [(8, 8, 0.0, 3), (9, 9, 0.0, 3)], [(9, 9, 0.0, 3)], []], [INF, INF, INF, 0.0])
    a_bad = S.machine([[(1, 1, 0.0, 1), (2, 2, 0.0, 2)], [(5, 9, 0.0, 3)], [(6, 3, 0.0, 3)], []], [INF, INF, INF, 0.0])
    a_both = S.machine([[(1, 1, 0.0, 1), (2, 2, 0.0, 2)], [(5, 8, 0.0, 3)], [(6, 3, 0.0, 3)], []], [INF, INF, INF, 0.0])
    db = dev(b, gpu_ctx)
    for order, message in (((a_bad, a_both), BAD_LABEL), ((a_both, a_bad), "Both sides can't require match")):
        assert B.reference(order[0], b, (9, 0, None), m1=(3, 0, None))[0] == message
        status, outs = raw_call(gpu_ctx, [dev(a, gpu_ctx) for a in order], db, 3, (3, 0, None), (9, 0, None))
        assert helpers.ko_message(status) == message and outs == [None] * 2
    k21_still_works(gpu_ctx, oracle)
    # set-up errors come before any launch, item by item
    status, outs = raw_call(gpu_ctx, [dev(good, gpu_ctx), dev(bad, gpu_ctx)], dg, 0, None, m2)
    assert helpers.ko_message(status) == "Custom MatcherConfig not supported with AutoFilter" and outs == [None] * 2
    assert gpu_ctx.sigma_batch_stats() == dict.fromkeys(_lib.SIGMA_BATCH_COUNTERS, 0)
    k21_still_works(gpu_ctx, oracle)
    unsorted_q = dict(good, props=(good["props"] & ~S.SORT_BITS) | (O_LABEL_SORTED << 1) | I_LABEL_SORTED)
    status, outs = raw_call(gpu_ctx, [dev(bad, gpu_ctx), dev(unsorted_q, gpu_ctx)], dg, 3, (3, 0, None), m2)
    assert helpers.ko_message(status) == "ComposeFst: 1st argument cannot perform required matching (sort?)" and outs == [None] * 2
    assert gpu_ctx.sigma_batch_stats()["launches"] == 0
    status, outs = raw_call(gpu_ctx, [dev(good, gpu_ctx)], dg, 3, None, (0, 0, None))
    assert helpers.ko_message(status) == "SigmaMatcher: 0 cannot be used as sigma_label" and outs == [None]
    sp = _lib.ShortestPathConfig(1e-6, 2, 0)
    arr = rustfst_amd.fst.HandleArray([dev(good, gpu_ctx)])._arr
    outs = (C.c_void_p * 1)(7)
    status = _lib.lib().wfst_compose_shortest_path_batch_with_matchers(gpu_ctx._h, arr, 1, dg._h, None, None, matcher(m2)._c(), C.byref(sp),
                                                                       outs, None)
    assert helpers.ko_message(status) == "unsupported: nshortest != 1 in the fused batch" and outs[0] is None
    k21_still_works(gpu_ctx, oracle)


# ---------------------------------------------------------------- degenerate inputs
def test_degenerate_inputs(gpu_ctx, oracle):
    strs, g, m2 = B.k21_batch()
    got, n_arcs, st = run_batch(gpu_ctx, [], g, m2)
    assert (got, n_arcs) == ([], 0) and st == dict.fromkeys(_lib.SIGMA_BATCH_COUNTERS, 0)
    empty_string = B.weighted_string([], final=0.25)
    no_start = dict(S.chain_query([2, 3, 5]), start=None)
    no_path = S.chain_query([2, 3])  # (ends in state 2 of the grammar, which is not final)
    final_start = S.machine([[(1, 1, 0.5, 1)], []], [0.75, 0.0])  # a grammar whose start state is final: the empty string has a path
    st = check_batch(gpu_ctx, oracle, [empty_string, no_start, no_path, strs[1]], g, m2, "degenerate acceptors")
    assert (st["items_in_kernel"], st["items_loop"]) == (3, 1)
    st = check_batch(gpu_ctx, oracle, [empty_string, strs[1]], final_start, m2, "the empty string against a final start state")
    assert st["items_in_kernel"] == 2
    st = check_batch(gpu_ctx, oracle, [strs[1], empty_string], dict(g, start=None), m2, "T without a start", kernel=False)
    assert (st["items_loop"], st["launches"]) == (2, 0)
