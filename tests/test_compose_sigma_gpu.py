"""Sigma-matcher composition on the device (compose_sigma.hip through wfst_compose_with_matchers): bit for bit the sequential
restatement tests/sigma_ref.py — states, arc order, weights, finals and the property word — with the counters of
wfst_ctx_get_compose_sigma_counters read after every call.  K21 and the reference's data files at every lane-group width, the
seeded grids of tests/sigma_cases.py, the limits of the kernel, arena growth, the errors and what follows them."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import rustfst_amd
from rustfst_amd import ComposeConfig, ComposeFilter, MatcherConfig, MatcherRewriteMode, WfstError, _lib

from oracle.model import O_LABEL_SORTED, flat_to_fst, fst_to_flat
from oracle.model.props import NOT_I_LABEL_SORTED

import helpers
from helpers import dev
import sigma_cases as S
import sigma_ref as R

pytestmark = pytest.mark.gpu
INF = np.inf
DEVICE_COUNTERS = ("require1_states", "require2_states", "exact_items", "sigma_items", "sigma_arcs", "refused_items")


def matcher(m):
    return None if m is None else MatcherConfig(m[0], MatcherRewriteMode(m[1]), m[2])


def run_device(ctx, f1, f2, flt, connect, m1, m2, d1=None, d2=None):
    """(flat result, counters) or (KO message, counters)"""
    cfg = ComposeConfig(ComposeFilter(flt), connect, matcher(m1), matcher(m2))
    try:
        out = (d1 or dev(f1, ctx)).compose(d2 or dev(f2, ctx), cfg).to_flat()
    except WfstError as e:
        return str(e).split(": ", 1)[1], ctx.compose_sigma_stats()
    return out, ctx.compose_sigma_stats()


def check_case(ctx, f1, f2, flt, m1, m2, what, connects=(False,)):
    """the device against the restatement; returns the counters of the last call (None after a KO)"""
    st = None
    for connect in connects:
        info = {}
        try:
            exp = R.compose_sigma(f1, f2, flt, connect, m1, m2, info)
        except R.SigmaError as e:
            exp = e.args[0]
        got, st = run_device(ctx, f1, f2, flt, connect, m1, m2)
        if isinstance(exp, str):
            assert got == exp, (what, got)
            assert {k: v for k, v in st.items() if k != "arena_grows"} == dict.fromkeys([k for k in st if k != "arena_grows"], 0), what
            st = None
            continue
        assert not isinstance(got, str), (what, got)
        helpers.assert_flat_identical(got, fst_to_flat(exp), "%s connect=%s" % (what, connect))
        assert (st["states"], st["arcs"], st["levels"]) == (info["states"], info["arcs"], info["levels"]), (what, st, info)
        assert st["level_launches"] >= 3 * st["levels"] and st["level_launches"] % 3 == 0, what
        for k in DEVICE_COUNTERS:  # (a level emitted again after an overflow counts its items again)
            assert st[k] == info[k] if st["arena_grows"] == 0 else st[k] >= info[k], (what, k, st, info)
        stats = ctx.stats()
        assert (stats["compose_states"], stats["compose_arcs"]) == (info["states"], info["arcs"]), what
    return st


def k21_cases(oracle):
    k = S.k21()
    g = S.from_spec(k["grammar_sigma"])
    out = [("k21-" + c["name"], S.from_spec(c["query"]), g, (1, 0, c["allowed"])) for c in k["cases"]]
    left, right = S.golden_pair(oracle)
    return out + [("sigma-matcher-2", left, right, (1, 0, None))]


def k21_still_works(ctx):
    k = S.k21()
    c = k["cases"][0]
    got, st = run_device(ctx, S.from_spec(c["query"]), S.from_spec(k["grammar_sigma"]), R.SEQUENCE, False, None, (1, 0, None))
    assert S.to_spec(flat_to_fst(got)) == c["expected_sigma"] and st["sigma_items"] == 1 and st["states"] == 4


# ---------------------------------------------------------------- K21 at every lane-group width
@pytest.mark.parametrize("group", ["2", "4", "8", "16", "64"])
def test_k21_and_golden_pair(gpu_ctx, oracle, monkeypatch, group):
    monkeypatch.setenv("WFST_WIDE_GROUP", group)
    k = S.k21()
    for name, f1, f2, m2 in k21_cases(oracle):
        st = check_case(gpu_ctx, f1, f2, R.SEQUENCE, None, m2, name + " G=" + group, connects=(False, True))
        assert st["arena_grows"] == 0
    got, st = run_device(gpu_ctx, *S.golden_pair(oracle), R.SEQUENCE, False, None, (1, 0, None))
    assert (st["states"], st["arcs"], S.count_paths(flat_to_fst(got))) == (15, 17, 4)
    assert S.to_spec(flat_to_fst(got)) == k["sigma_matcher_2"]["expected"]
    assert (st["require2_states"], st["sigma_items"], st["sigma_arcs"], st["refused_items"]) == (4, 3, 3, 0)


def test_cpp_sigma_matcher_tests_run(gpu_ctx, tmp_path):
    """examples/sigma_matcher_tests.cpp: the reference's three tests against include/wfst.hpp, end to end"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = tmp_path / "sigma_tests"
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(helpers.ROOT, "include"),
                    os.path.join(helpers.ROOT, "examples", "sigma_matcher_tests.cpp"), "-L", libdir, "-lwfst_amd",
                    f"-Wl,-rpath,{libdir}", "-Wl,--allow-shlib-undefined", "-o", str(exe)], check=True)
    env = dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([str(exe), os.path.join(helpers.ROOT, "tests", "golden")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all sigma-matcher tests passed" in r.stdout, r.stdout + r.stderr


# ---------------------------------------------------------------- seeded grids
@pytest.mark.parametrize("side,plain_unsorted", S.GRIDS, ids=["side1-both", "side1-fst2-unsorted", "side2-both",
                                                              "side2-fst1-unsorted", "both-sides"])
def test_random_grid(gpu_ctx, side, plain_unsorted):
    """six filters x three rewrite modes x acceptor / transducer sigma operand on pairs of 6-30 states, |Sigma| = 5, sigma
    inside the alphabet, epsilons on both tapes; the cases the restatement ends in an error (at most a quarter: checked on
    the CPU) are asserted as that KO"""
    kos = sigma_items = 0
    for c in S.grid(side, plain_unsorted):
        st = check_case(gpu_ctx, c["f1"], c["f2"], c["filter"], c["m1"], c["m2"], c["name"], connects=(False, True))
        kos += st is None
        sigma_items += st["sigma_items"] if st else 0
    assert 4 * kos <= 36 and sigma_items > 0


# ---------------------------------------------------------------- the limits of the kernel
SG = 50  # sigma of the hand-built grammars


def limit_cases():
    """(name, fst1, fst2, m2): fst1 a fan of arcs at its start state (iterated: state 0 of fst2 carries a sigma arc)"""
    out = []
    # 70 items (69 arcs and the loop item), some answered exactly (100..119 are explicit) and some by sigma
    out.append(("70-items", S.fan_query(range(100, 169)), S.sigma_state(range(100, 120), [(SG, SG)]), None))
    for n_sig in (1, 2, 3):  # more than one sigma arc in a state: eval_item's `write` path
        out.append(("%d-sigma-arcs" % n_sig, S.fan_query([3, 4, 60]), S.sigma_state([3], [(SG, SG), (SG, 7), (SG, 0)][:n_sig]), None))
    for n_se in (16, 17):  # searched side staged in LDS / read from memory
        out.append(("searched-%d" % n_se, S.fan_query([1, 8, 40, 60, 99]), S.sigma_state(range(1, n_se), [(SG, SG)]), None))
        out.append(("searched-%d-sigma-first" % n_se, S.fan_query([1, 8, 40, 60, 99]), S.sigma_state(range(60, 59 + n_se), [(SG, 9)]), None))
    out.append(("sigma-smallest", S.fan_query([60, 61, 70]), S.sigma_state([60, 61, 62], [(SG, SG)]), None))
    out.append(("sigma-largest", S.fan_query([1, 2, 70]), S.sigma_state([1, 2, 3], [(SG, SG)]), None))
    out.append(("sigma-above-every-label", S.fan_query([1, 2, 3]), S.sigma_state([1, 2], [(1000000, 1000000)]), (1000000, None)))
    # forms of the sigma arc; 7:SG is NOT a sigma arc under MatchInput (its ilabel is 7)
    g = S.machine([sorted([(7, SG, 0.5, 1), (SG, SG, 1.0, 1), (SG, 8, 1.25, 1), (SG, 0, 1.5, 1)], key=lambda t: t[0]), []], [INF, 0.0])
    out.append(("sigma-forms", S.fan_query([7, 9, 11]), g, None))
    g = S.machine([[(7, SG, 0.5, 1)], []], [INF, 0.0])
    out.append(("olabel-sigma-only", S.fan_query([7, 9]), g, None))
    # allowed sets: one entry, a thousand, duplicates; labels at both ends of the set and just outside it
    grammar = S.sigma_state([5], [(SG, SG)])
    out.append(("allowed-1", S.fan_query([5, 9, 10, 11]), grammar, (SG, [10])))
    big = [2 * x for x in range(100, 1100)]
    out.append(("allowed-1000", S.fan_query([199, 200, 201, 1000, 2198, 2199, 2200]), grammar, (SG, big)))
    out.append(("allowed-duplicates", S.fan_query([9, 10, 11, 12]), grammar, (SG, [12, 10, 12, 10, 10])))
    return out


def test_kernel_limits(gpu_ctx, monkeypatch):
    seen = dict.fromkeys(("sigma_items", "refused_items", "exact_items"), 0)
    for name, f1, f2, m in limit_cases():
        sigma, allowed = m if m else (SG, None)
        for rw in (0, 1, 2):
            st = check_case(gpu_ctx, f1, f2, R.SEQUENCE, None, (sigma, rw, allowed), "%s rw=%d" % (name, rw))
            for k in seen:
                seen[k] += st[k]
            if name == "70-items":
                assert (st["exact_items"], st["sigma_items"]) == (20, 69 - 20)  # (the loop item asks for NO_LABEL: nothing)
            if name == "3-sigma-arcs":
                assert (st["sigma_items"], st["sigma_arcs"]) == (2, 6)
            if name == "olabel-sigma-only":
                assert (st["require2_states"], st["sigma_items"]) == (0, 0)
            if name == "allowed-1000":
                assert (st["sigma_items"], st["refused_items"]) == (3, 4)
    assert all(seen.values())
    for group in ("2", "64"):  # 70 items are 35 chunks of two lanes, two of 64
        monkeypatch.setenv("WFST_WIDE_GROUP", group)
        name, f1, f2, _ = limit_cases()[0]
        check_case(gpu_ctx, f1, f2, R.MATCH, None, (SG, 0, None), name + " G=" + group)


def test_sigma_on_side_one_limits(gpu_ctx):
    """the mirror image: fst1 carries sigma on its OUTPUT tape and is searched, fst2 is iterated (MatchOutput rewriting)"""
    f1 = S.machine([sorted([(7, 3, 0.5, 1), (SG, SG, 1.0, 1), (8, SG, 1.25, 1), (0, SG, 1.5, 1), (SG, 9, 0.25, 1)], key=lambda t: t[1]), []],
                   [INF, 0.0])
    f2 = S.machine([[(3, 3, 0.0, 1), (4, 40, 0.25, 1), (9, 90, 0.5, 1)], []], [INF, 0.25])
    for rw in (0, 1, 2):
        st = check_case(gpu_ctx, f1, f2, R.SEQUENCE, (SG, rw, [4, 9]), None, "side1 rw=%d" % rw, connects=(False, True))
        assert (st["require1_states"], st["sigma_items"], st["sigma_arcs"], st["exact_items"]) == (1, 1, 3, 2)


# ---------------------------------------------------------------- arena growth
def big_pair():
    """a result of a few thousand states"""
    rng = np.random.default_rng(79)
    f1 = flat_to_fst(helpers.random_fst_flat(rng, 90, 3, 6, p_eps_o=0.1, p_final=0.1, sort="olabel", min_fanout=2))
    f2 = flat_to_fst(helpers.random_fst_flat(rng, 90, 3, 6, p_eps_i=0.1, p_final=0.1, sort="ilabel", min_fanout=2))
    for r in f1["rows"]:
        for t in r:
            if t[1] == 4:
                t[1] = 6
    f1 = S._sorted_rows(f1, 1)
    return S.with_sort_word(f1), S.with_sort_word(f2)


@pytest.mark.parametrize("foresight", [True, False])
@pytest.mark.parametrize("batch", ["1", "8"])
def test_arena_growth(gpu_ctx, monkeypatch, foresight, batch):
    monkeypatch.setenv("WFST_WIDE_EST_STATES", "64")
    monkeypatch.setenv("WFST_WIDE_BATCH", batch)
    if not foresight:
        monkeypatch.setenv("WFST_WIDE_NO_FORESIGHT", "1")
    f1, f2 = big_pair()
    retries = gpu_ctx.stats()["compose_retries"]
    st = check_case(gpu_ctx, f1, f2, R.SEQUENCE, None, (4, 2, None), "growth", connects=(False, True))
    assert 2000 <= st["states"] <= 20000 and st["sigma_items"] > 0
    assert st["arena_grows"] >= 2 and gpu_ctx.stats()["compose_retries"] >= retries + st["arena_grows"]


# ---------------------------------------------------------------- errors, and the context after them
def test_ko_cases_leave_the_context_working(gpu_ctx):
    k = S.k21()
    q, g = S.chain_query([2, 3, 5]), S.from_spec(k["grammar_sigma"])
    unsorted_g = dict(g, props=(g["props"] & ~S.SORT_BITS) | NOT_I_LABEL_SORTED | O_LABEL_SORTED)
    # bad label with a sigma arc in the searched state (fst2's state 1) and without one (state 0), fst1 iterated
    bad_with = S.chain_query([2, 1, 5])
    bad_without = S.chain_query([1, 3, 5])
    both_a = S.machine([[(4, 3, 0.0, 1), (9, 9, 0.0, 1)], []], [INF, 0.0])
    both_b = S.machine([[(3, 3, 0.0, 1), (9, 9, 0.0, 1)], []], [INF, 0.0])
    cases = [
        ("bad label, sigma arc in the state", bad_with, g, R.SEQUENCE, None, (1, 0, None), "SigmaMatcher::Find: bad label (sigma)"),
        ("bad label, no sigma arc in the state", bad_without, g, R.SEQUENCE, None, (1, 0, None), "SigmaMatcher::Find: bad label (sigma)"),
        ("both sides require", both_a, both_b, R.SEQUENCE, (3, 0, None), (9, 0, None), "Both sides can't require match"),
        ("unsorted sigma side", q, unsorted_g, R.SEQUENCE, None, (1, 0, None), "ComposeFst: 2nd argument cannot perform required matching (sort?)"),
        ("AutoFilter", q, g, R.AUTO, None, (1, 0, None), "Custom MatcherConfig not supported with AutoFilter"),
        ("sigma 0", q, unsorted_g, R.AUTO, None, (0, 0, None), "SigmaMatcher: 0 cannot be used as sigma_label"),
    ]
    for what, f1, f2, flt, m1, m2, message in cases:
        assert _ref_message(f1, f2, flt, m1, m2) == message, what
        got, st = run_device(gpu_ctx, f1, f2, flt, False, m1, m2)
        assert got == message, what
        assert all(v == 0 for k, v in st.items() if k != "arena_grows"), what
        k21_still_works(gpu_ctx)
    # rewrite_mode 3 has no Python spelling: through the C-ABI
    d1, d2 = dev(q, gpu_ctx), dev(g, gpu_ctx)
    out = C.c_void_p()
    cfg = _lib.ComposeConfig(3, 0)
    m = _lib.MatcherConfig(1, 3, None, 0)
    status = _lib.lib().wfst_compose_with_matchers(gpu_ctx._h, d1._h, d2._h, C.byref(cfg), None, C.byref(m), C.byref(out))
    assert helpers.ko_message(status) == "unknown rewrite_mode 3" and out.value is None
    k21_still_works(gpu_ctx)


def _ref_message(f1, f2, flt, m1, m2):
    try:
        R.compose_sigma(f1, f2, flt, False, m1, m2)
    except R.SigmaError as e:
        return e.args[0]
    return None


def test_error_order_across_states(gpu_ctx, monkeypatch):
    """rule 7 on the device: an earlier state's bad label beats a later state's "both sides", and the other way round"""
    b = S.machine([[(1, 1, 0.0, 1), (2, 2, 0.0, 2)], [(8, 8, 0.0, 3), (9, 9, 0.0, 3)], [(9, 9, 0.0, 3)], []], [INF, INF, INF, 0.0])
    a = S.machine([[(1, 1, 0.0, 1), (2, 2, 0.0, 2)], [(5, 9, 0.0, 3)], [(6, 3, 0.0, 3)], []], [INF, INF, INF, 0.0])
    a2 = S.machine([[(1, 1, 0.0, 1), (2, 2, 0.0, 2)], [(5, 8, 0.0, 3)], [(6, 3, 0.0, 3)], []], [INF, INF, INF, 0.0])
    for f1, message in ((a, "SigmaMatcher::Find: bad label (sigma)"), (a2, "Both sides can't require match")):
        assert _ref_message(f1, b, R.SEQUENCE, (3, 0, None), (9, 0, None)) == message
        for group in ("2", "64"):
            monkeypatch.setenv("WFST_WIDE_GROUP", group)
            got, _ = run_device(gpu_ctx, f1, b, R.SEQUENCE, False, (3, 0, None), (9, 0, None))
            assert got == message, group
    monkeypatch.delenv("WFST_WIDE_GROUP")
    k21_still_works(gpu_ctx)


# ---------------------------------------------------------------- what the call is equal to, and what it leaves alone
def test_no_label_and_no_config_are_the_plain_composition(gpu_ctx, oracle):
    cases = [c for c in S.grid(2, False)][:12]
    for c in cases:
        d1, d2 = dev(c["f1"], gpu_ctx), dev(c["f2"], gpu_ctx)
        before = (d1.to_flat(), d2.to_flat())
        for connect in (False, True):
            flt = ComposeFilter(c["filter"])
            plain = d1.compose(d2, ComposeConfig(flt, connect)).to_flat()
            path_stats = gpu_ctx.compose_path_stats()
            # sigma = NO_LABEL: no state has a sigma arc, on either side or on both (the wide driver all the same)
            for m1, m2 in ((None, (R.NO_LABEL, 1, [3])), ((R.NO_LABEL, 0, None), None), ((R.NO_LABEL, 2, None), (R.NO_LABEL, 0, None))):
                got, st = run_device(gpu_ctx, None, None, c["filter"], connect, m1, m2, d1, d2)
                helpers.assert_flat_identical(got, plain, c["name"])
                assert st["levels"] > 0 and sum(st[k] for k in DEVICE_COUNTERS) == 0
            # both configs NULL through the new entry point: wfst_compose, call for call (its route counters move, sigma's do not)
            sigma_before = gpu_ctx.compose_sigma_stats()
            out = C.c_void_p()
            cfg = _lib.ComposeConfig(c["filter"], 1 if connect else 0)
            assert _lib.lib().wfst_compose_with_matchers(gpu_ctx._h, d1._h, d2._h, C.byref(cfg), None, None, C.byref(out)) == 0
            helpers.assert_flat_identical(rustfst_amd.DeviceFst(out, gpu_ctx).to_flat(), plain, c["name"])
            assert gpu_ctx.compose_sigma_stats() == sigma_before and gpu_ctx.compose_path_stats() == path_stats
        for b, d in zip(before, (d1, d2)):  # the input handles are left as they were
            helpers.assert_flat_identical(d.to_flat(), b, c["name"] + " input")


def test_inputs_untouched_and_shortest_path_on_the_result(gpu_ctx, oracle):
    left, right = S.golden_pair(oracle)
    d1, d2 = dev(left, gpu_ctx), dev(right, gpu_ctx)
    before = (d1.to_flat(), d2.to_flat())
    cfg = ComposeConfig(ComposeFilter.SEQUENCEFILTER, True, None, MatcherConfig(1))
    composed = d1.compose(d2, cfg)
    exp = fst_to_flat(R.compose_sigma(left, right, R.SEQUENCE, True, None, (1, 0, None)))
    helpers.assert_flat_identical(composed.to_flat(), exp, "sigma-matcher-2 connected")
    for b, d in zip(before, (d1, d2)):
        helpers.assert_flat_identical(d.to_flat(), b, "input")
    sp = composed.shortest_path().to_flat()
    want = helpers.to_oracle(oracle, exp).shortest_path_canonical().to_flat()
    helpers.assert_flat_identical(sp, want, "shortest path of the sigma composition", check_props=False)
    # the host mirror and the free function route the same way
    v1, v2 = d1.to_vector_fst(), d2.to_vector_fst()
    helpers.assert_flat_identical(rustfst_amd.compose_with_config(v1, v2, cfg).to_device(gpu_ctx).to_flat(), exp, "VectorFst")


def test_counter_getter_pointer_by_pointer(gpu_ctx, oracle, wfst_lib):
    """wfst_ctx_get_compose_sigma_counters: any out-pointer may be NULL, each one alone receives the counter of its position"""
    left, right = S.golden_pair(oracle)
    _, full = run_device(gpu_ctx, left, right, R.SEQUENCE, False, None, (1, 0, None))
    names, fn, sentinel = _lib.COMPOSE_SIGMA_COUNTERS, wfst_lib.wfst_ctx_get_compose_sigma_counters, 0xA5A5A5A5A5A5A5A5
    assert tuple(full) == names and full["states"] == 15 and fn(gpu_ctx._h, *[None] * len(names)) == 0
    for i, name in enumerate(names):
        vals = [C.c_uint64(sentinel) for _ in names]
        assert fn(gpu_ctx._h, *[C.byref(v) if k == i else None for k, v in enumerate(vals)]) == 0
        assert [v.value for v in vals] == [full[name] if k == i else sentinel for k in range(len(names))], name
