"""Sigma-matcher composition without a GPU: the sequential restatement (tests/sigma_ref.py) reproduces the reference's own
tests (K21) and its errors in their order, agrees bit for bit with the C++ oracle's PLAIN composition of the explicitly
expanded grammar (the expansion identity), and the C-ABI / Python / C++ surfaces are declared, bound and validated."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import rustfst_amd
from rustfst_amd import ComposeConfig, ComposeFilter, MatcherConfig, MatcherRewriteMode, _lib

from oracle.model import ACCEPTOR, I_LABEL_SORTED, O_LABEL_SORTED, flat_to_fst, fst_to_flat
from oracle.model.props import NOT_I_LABEL_SORTED, NOT_O_LABEL_SORTED

import helpers
import sigma_cases as S
import sigma_ref as R

ROOT = helpers.ROOT
INF = np.inf
NEW_SYMBOLS = ("wfst_compose_with_matchers", "wfst_ctx_get_compose_sigma_counters")
COUNTERS = ("levels", "states", "arcs", "require1_states", "require2_states", "exact_items", "sigma_items", "sigma_arcs",
            "refused_items", "arena_grows", "level_launches")


# ---------------------------------------------------------------- K21: the reference's own tests
def test_k21_play_sigma_please():
    """sigma_matcher.rs:486-546: the sigma grammar answers like the loop grammar, except for "bowie" under {radiohead, queen}"""
    k = S.k21()
    assert k["sigma_label"] == 1 and k["compose_filter"] == R.SEQUENCE and not k["connect"]
    g_sigma = S.from_spec(k["grammar_sigma"])
    assert g_sigma["props"] & ACCEPTOR
    for case in k["cases"]:
        q = S.from_spec(case["query"])
        info = {}
        got = R.compose_sigma(q, g_sigma, R.SEQUENCE, False, None, (1, k["rewrite_mode"], case["allowed"]), info)
        assert S.to_spec(got) == case["expected_sigma"], case["name"]
        assert (case["expected_sigma"] == case["expected_loop"]) == case["equal"] == (case["name"] != "bowie_refused")
        assert info["refused_items"] == (0 if case["equal"] else 1) and info["sigma_items"] == (1 if case["equal"] else 0)


def test_k21_loop_grammar_is_the_plain_composition(oracle):
    k = S.k21()
    g_loop = fst_to_flat(S.from_spec(k["grammar_loop"]))
    for case in k["cases"]:
        q = fst_to_flat(S.from_spec(case["query"]))
        got = helpers.to_oracle(oracle, q).compose(helpers.to_oracle(oracle, g_loop), connect=False, compose_filter=3).to_flat()
        assert S.to_spec(flat_to_fst(got)) == case["expected_loop"], case["name"]


def test_k21_sigma_matcher_2(oracle):
    """sigma_matcher.rs:548-596 on its own data files: 15 states and 17 arcs before connect, 4 complete paths; state 4 of
    right carries an input-epsilon arc AND a sigma arc, so a fall-through from the epsilons to sigma would show (K21_DERIVATION.md)"""
    k = S.k21()["sigma_matcher_2"]
    left, right = S.golden_pair(oracle)
    assert left["props"] & O_LABEL_SORTED and right["props"] & I_LABEL_SORTED and not right["props"] & ACCEPTOR
    assert S.has_sigma_state_with_ieps(right, 1)
    info = {}
    got = R.compose_sigma(left, right, R.SEQUENCE, False, None, (k["sigma_label"], 0, None), info)
    assert (info["states"], info["arcs"], S.count_paths(got)) == (k["states"], k["arcs"], k["paths"]) == (15, 17, 4)
    assert S.to_spec(got) == k["expected"]
    connected = R.compose_sigma(left, right, R.SEQUENCE, True, None, (k["sigma_label"], 0, None))
    assert S.count_paths(connected) == 4


# ---------------------------------------------------------------- errors and their order
def _pair():
    q = S.chain_query([2, 3, 5])
    g = S.from_spec(S.k21()["grammar_sigma"])
    return q, g


def _ko(f1, f2, flt, m1, m2):
    with pytest.raises(R.SigmaError) as e:
        R.compose_sigma(f1, f2, flt, False, m1, m2)
    return e.value.args[0]


def test_ref_setup_errors_in_order():
    q, g = _pair()
    unsorted_g = dict(g, props=(g["props"] & ~S.SORT_BITS) | NOT_I_LABEL_SORTED | O_LABEL_SORTED)
    unknown_g = dict(g, props=g["props"] & ~S.SORT_BITS)
    # sigma 0 comes before the filter, the filter before sortedness (compose_static.rs:178-192)
    assert _ko(q, unsorted_g, R.AUTO, None, (0, 0, None)) == "SigmaMatcher: 0 cannot be used as sigma_label"
    assert _ko(q, unsorted_g, R.AUTO, (0, 0, None), (1, 0, None)) == "SigmaMatcher: 0 cannot be used as sigma_label"
    assert _ko(q, unsorted_g, R.AUTO, None, (1, 0, None)) == "Custom MatcherConfig not supported with AutoFilter"
    assert _ko(q, g, R.AUTO, None, (R.NO_LABEL, 0, None)) == "Custom MatcherConfig not supported with AutoFilter"
    assert _ko(q, unsorted_g, R.SEQUENCE, None, (1, 0, None)) == "ComposeFst: 2nd argument cannot perform required matching (sort?)"
    assert "2nd argument: label-sortedness properties are not known" in _ko(q, unknown_g, R.SEQUENCE, None, (1, 0, None))
    unsorted_q = dict(q, props=(q["props"] & ~S.SORT_BITS) | NOT_O_LABEL_SORTED | I_LABEL_SORTED)
    assert _ko(unsorted_q, unsorted_g, R.SEQUENCE, (1, 0, None), (1, 0, None)) == \
        "ComposeFst: 1st argument cannot perform required matching (sort?)"
    # sigma = NO_LABEL requires nothing: the unsorted grammar is fine while fst1 is sorted, and the result is the plain one
    plain = R.compose_sigma(q, unsorted_g, R.SEQUENCE, False, None, None)
    assert R.compose_sigma(q, unsorted_g, R.SEQUENCE, False, None, (R.NO_LABEL, 1, [7])) == plain


def test_ref_run_errors_first_state_first_item():
    """rule 7: the first offending composed state in id order; within it "both sides" before the items, the items in order"""
    # state 0 x 0: fst1's second arc carries label 1 = sigma of side 2 -> bad label, though state 0 of g has no sigma arc
    g = S.machine([[(2, 2, 0.0, 1)], [(1, 1, 0.0, 1)]], [INF, 0.0])
    q = S.machine([[(2, 2, 0.0, 1), (7, 1, 0.0, 1)], []], [INF, 0.0], sort_bits=I_LABEL_SORTED | NOT_O_LABEL_SORTED)
    assert _ko(q, g, R.SEQUENCE, None, (1, 0, None)) == "SigmaMatcher::Find: bad label (sigma)"
    # both sides sorted, both start states carry their sigma: "both" wins over the bad label of the same state
    a = S.machine([[(4, 3, 0.0, 1), (9, 9, 0.0, 1)], []], [INF, 0.0])  # olabels 3 (sigma of side 1) and 9 (sigma of side 2)
    b = S.machine([[(3, 3, 0.0, 1), (9, 9, 0.0, 1)], []], [INF, 0.0])
    assert _ko(a, b, R.SEQUENCE, (3, 0, None), (9, 0, None)) == "Both sides can't require match"
    # the same pair with only side 2 configured: fst1 is iterated, its arc 9 is the bad label
    assert _ko(a, b, R.SEQUENCE, None, (9, 0, None)) == "SigmaMatcher::Find: bad label (sigma)"
    # a later state's "both" loses against an earlier state's bad label: state 1 = (1, 1) is bad, state 2 = (2, 2) is both
    a = S.machine([[(1, 1, 0.0, 1), (2, 2, 0.0, 2)], [(5, 9, 0.0, 3)], [(6, 3, 0.0, 3)], []], [INF, INF, INF, 0.0])
    b = S.machine([[(1, 1, 0.0, 1), (2, 2, 0.0, 2)], [(8, 8, 0.0, 3), (9, 9, 0.0, 3)], [(9, 9, 0.0, 3)], []], [INF, INF, INF, 0.0])
    assert _ko(a, b, R.SEQUENCE, (3, 0, None), (9, 0, None)) == "SigmaMatcher::Find: bad label (sigma)"
    # ... and wins once state 1 is clean (its label 8 is matched exactly)
    a2 = S.machine([[(1, 1, 0.0, 1), (2, 2, 0.0, 2)], [(5, 8, 0.0, 3)], [(6, 3, 0.0, 3)], []], [INF, INF, INF, 0.0])
    assert _ko(a2, b, R.SEQUENCE, (3, 0, None), (9, 0, None)) == "Both sides can't require match"


# ---------------------------------------------------------------- the expansion identity against the C++ oracle
def _identity_pair(seed, acceptor):
    """q (fst1, says NOT_O_LABEL_SORTED so that both runs iterate it) and g (fst2, sigma = 3 on the input tape).  Label 6 is
    on q's output tape only, so every sigma state keeps a non-epsilon arc after the expansion (alleps2 stays what it was)."""
    rng = np.random.default_rng(seed)
    q = flat_to_fst(helpers.random_fst_flat(rng, int(rng.integers(6, 20)), 4, 5, p_eps_i=0.1, p_eps_o=0.2, p_final=0.3,
                                            sort="none", min_fanout=1))
    for r in q["rows"]:
        for t in r:
            if t[1] == 3:
                t[1] = 6
    q["rows"][0].append([1, 6, q["rows"][0][0][2], 0])
    g = flat_to_fst(helpers.random_fst_flat(rng, int(rng.integers(6, 20)), 4, 5, p_eps_i=0.2, p_eps_o=0.1, p_final=0.3,
                                            sort="ilabel", min_fanout=1))
    if acceptor:
        g["rows"] = [[[t[0], t[0], t[2], t[3]] for t in r] for r in g["rows"]]
    q = S.with_sort_word(q)
    q["props"] = (q["props"] & ~(O_LABEL_SORTED | NOT_O_LABEL_SORTED)) | NOT_O_LABEL_SORTED
    return q, S.with_sort_word(g, acceptor)


@pytest.mark.parametrize("acceptor", [False, True])
def test_expansion_identity(oracle, acceptor):
    """sigma(q, g) == plain(q, expand(g)) bit for bit, six filters x three rewrite modes, with and without an allowed set"""
    seen_ieps = False
    for seed in range(4):
        q, g = _identity_pair(40 + seed, acceptor)
        seen_ieps |= S.has_sigma_state_with_ieps(g, 3)
        labels = sorted({t[1] for r in q["rows"] for t in r})
        assert 6 in labels and all(t[0] != 6 for r in g["rows"] for t in r)
        oq = helpers.to_oracle(oracle, fst_to_flat(q))
        for allowed in (None, [6, 1, 2, 6, 5]):
            for rw in (0, 1, 2):
                e = R.expand_sigma(g, 3, rw, allowed, labels)
                assert S.sortedness(e) & I_LABEL_SORTED
                oe = helpers.to_oracle(oracle, fst_to_flat(e))
                for flt in S.FILTERS:
                    for connect in (False, True):
                        got = fst_to_flat(R.compose_sigma(q, g, flt, connect, None, (3, rw, allowed)))
                        exp = oq.compose(oe, connect=connect, compose_filter=flt).to_flat()
                        helpers.assert_flat_identical(got, exp, "seed %d rw %d filter %d allowed %s" % (seed, rw, flt, allowed))
    assert seen_ieps


def test_random_grids_stay_within_the_ko_cap():
    """what the GPU tests run: at most a quarter of each grid ends in an error, sigma states with input epsilons occur"""
    ieps = False
    for side, plain_unsorted in S.GRIDS:
        cases = list(S.grid(side, plain_unsorted))
        kos = [c["name"] for c in cases if isinstance(S.run_ref(c)[0], str)]
        assert len(cases) == 36 and 4 * len(kos) <= len(cases), (side, plain_unsorted, kos)
        ieps |= any(c["m2"] and S.has_sigma_state_with_ieps(c["f2"], c["m2"][0]) for c in cases)
        if side == 3:
            assert kos, "the grid with both sides configured is there for its errors too"
    assert ieps


# ---------------------------------------------------------------- the surfaces
def test_symbols_declared_bound_and_versioned(wfst_lib):
    with open(os.path.join(ROOT, "include", "wfst.h")) as f:
        header = f.read()
    bound = {n: a for n, _, a in _lib.SYMBOLS}
    m = re.search(r"#define\s+WFST_ABI_VERSION\s+7\b(.*)", header)
    for name in NEW_SYMBOLS:
        assert hasattr(wfst_lib, name) and name in bound and name in m.group(1).split("; 6:")[0]
    assert wfst_lib.wfst_abi_version() == 7
    assert helpers.header_params(header, "wfst_compose_with_matchers") == (
        "wfst_ctx* ctx, const wfst_fst* fst1, const wfst_fst* fst2, const wfst_compose_config* cfg, "
        "const wfst_matcher_config* m1, const wfst_matcher_config* m2, wfst_fst** out")
    assert re.search(r"typedef struct \{\s*uint32_t sigma_label;\s*uint32_t rewrite_mode;[^}]*const uint32_t\* sigma_allowed_matches;"
                     r"\s*size_t n_allowed;[^}]*\} wfst_matcher_config;", header)
    assert re.search(r"typedef struct \{\s*uint32_t compose_filter;\s*uint32_t connect;[^}]*\} wfst_compose_config;", header)
    assert C.sizeof(_lib.MatcherConfig) == 24 and C.sizeof(_lib.ComposeConfig) == 8
    helpers.check_counter_getter(wfst_lib, "wfst_ctx_get_compose_sigma_counters", COUNTERS, rustfst_amd.Context.compose_sigma_stats)
    assert _lib.COMPOSE_SIGMA_COUNTERS == COUNTERS


def test_null_arguments_are_ko_without_a_gpu(wfst_lib):
    m = _lib.MatcherConfig(1, 0, None, 0)
    out = C.c_void_p(5)
    assert "null" in helpers.ko_message(wfst_lib.wfst_compose_with_matchers(None, None, None, None, C.byref(m), None, C.byref(out)))
    assert out.value is None  # (zeroed before anything is looked at)
    assert "null" in helpers.ko_message(wfst_lib.wfst_compose_with_matchers(None, None, None, None, None, None, C.byref(out)))


def test_python_surface():
    assert [m.value for m in MatcherRewriteMode] == [0, 1, 2] and MatcherRewriteMode.AUTO.value == 0
    m = MatcherConfig(7)
    assert (m.sigma_label, m.rewrite_mode, m.sigma_allowed_matches) == (7, MatcherRewriteMode.AUTO, [])
    c = m._c().contents
    assert (c.sigma_label, c.rewrite_mode, c.n_allowed, bool(c.sigma_allowed_matches)) == (7, 0, 0, False)
    m = MatcherConfig(0xFFFFFFFF, MatcherRewriteMode.NEVER, [6, 4, 6])
    c = m._c().contents
    assert (c.sigma_label, c.rewrite_mode, c.n_allowed) == (0xFFFFFFFF, 2, 3) and c.sigma_allowed_matches[:3] == [6, 4, 6]
    with pytest.raises(ValueError):
        MatcherConfig(1 << 32)
    with pytest.raises(TypeError):
        MatcherConfig(1, 2)
    with pytest.raises(TypeError):
        ComposeConfig(matcher2_config=(1, 0, None))
    cfg = ComposeConfig(ComposeFilter.SEQUENCEFILTER, False, None, m)
    assert cfg.matcher1_config is None and cfg.matcher2_config is m and cfg._c(matchers=True).contents.compose_filter == 3
    with pytest.raises(rustfst_amd.WfstError):  # the fused batch has no matcher configs
        cfg._c()
    assert ComposeConfig().matcher1_config is None and ComposeConfig()._c().contents.connect == 1
    assert "MatcherConfig" in rustfst_amd.__all__ and "MatcherRewriteMode" in rustfst_amd.__all__


def test_cpp_mirror_example_compiles(tmp_path):
    """include/wfst.hpp carries the matcher configs at the END of ComposeConfig (positional initialisers of the two leading
    members still compile) and examples/sigma_matcher_tests.cpp restates the reference's three tests against it"""
    src = tmp_path / "positional.cpp"
    src.write_text('#include "wfst.hpp"\nint main() { wfst_amd::ComposeConfig a{wfst_amd::ComposeFilterEnum::SequenceFilter, false};\n'
                   '  wfst_amd::ComposeConfig b; b.matcher2_config.sigma_matcher_config = wfst_amd::SigmaMatcherConfig{1};\n'
                   '  return a.matcher1_config.empty() && !b.matcher2_config.empty() ? 0 : 1; }\n')
    for path in (str(src), os.path.join(ROOT, "examples", "sigma_matcher_tests.cpp")):
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), path],
                       check=True, capture_output=True)
