"""The fused batch with a sigma matcher, without a GPU: the new symbols are declared, bound and versioned, the arguments are
validated before a GPU is touched, the C++ example compiles, and the restatement (tests/sigma_ref.py) says what the GPU tests
(tests/test_sigma_batch_gpu.py) may expect of the kernel: which of their items fit its limits."""
import ctypes as C
import os
import re
import subprocess

import pytest

import rustfst_amd
from rustfst_amd import ComposeConfig, ComposeFilter, MatcherConfig, _lib

import helpers
import sigma_batch_cases as B
import sigma_ref as R

ROOT = helpers.ROOT
NEW_SYMBOLS = ("wfst_compose_shortest_path_batch_with_matchers", "wfst_ctx_get_sigma_batch_counters")
COUNTERS = ("launches", "items_in_kernel", "items_handed_back", "items_loop", "exact_items", "sigma_items", "sigma_arcs",
            "refused_items", "max_level_width")


def test_symbols_declared_bound_and_versioned(wfst_lib):
    with open(os.path.join(ROOT, "include", "wfst.h")) as f:
        header = f.read()
    bound = {n: a for n, _, a in _lib.SYMBOLS}
    m = re.search(r"#define\s+WFST_ABI_VERSION\s+7\b(.*)", header)
    for name in NEW_SYMBOLS:
        assert hasattr(wfst_lib, name) and name in bound and name in m.group(1).split("; 6:")[0]
    assert wfst_lib.wfst_abi_version() == 7
    assert helpers.header_params(header, "wfst_compose_shortest_path_batch_with_matchers") == (
        "wfst_ctx* ctx, const wfst_fst* const* acceptors, size_t n, const wfst_fst* t, const wfst_compose_config* ccfg, "
        "const wfst_matcher_config* m1, const wfst_matcher_config* m2, const wfst_shortest_path_config* scfg, wfst_fst** outs, "
        "uint64_t* composed_arcs")
    assert len(bound["wfst_compose_shortest_path_batch_with_matchers"]) == 10
    helpers.check_counter_getter(wfst_lib, "wfst_ctx_get_sigma_batch_counters", COUNTERS, rustfst_amd.Context.sigma_batch_stats)
    assert _lib.SIGMA_BATCH_COUNTERS == COUNTERS
    # outside the table of the *_stats families, and its struct is not one of theirs
    assert all(symbol != "wfst_ctx_get_sigma_batch_counters" for symbol, _ in _lib.COUNTERS.values())
    with open(os.path.join(ROOT, "rustfst_amd", "csrc", "common.h")) as f:
        assert re.search(r"struct SigmaBatchCounters \{[^}]*\} sigma_batch;", f.read())


def test_null_arguments_are_ko_without_a_gpu(wfst_lib):
    fn = wfst_lib.wfst_compose_shortest_path_batch_with_matchers
    m = _lib.MatcherConfig(1, 0, None, 0)
    outs = (C.c_void_p * 2)(5, 6)
    assert "null pointer" in helpers.ko_message(fn(None, None, 2, None, None, None, C.byref(m), None, outs, None))
    assert outs[0] is None and outs[1] is None  # (zeroed before anything is looked at)
    assert "null pointer" in helpers.ko_message(fn(None, None, 0, None, None, C.byref(m), None, None, None, None))
    # without matcher configs the call is wfst_compose_shortest_path_batch, its null check included
    assert "null pointer" in helpers.ko_message(fn(None, None, 0, None, None, None, None, None, outs, None))


def test_python_surface_still_refuses_outside_the_batch_call():
    cfg = ComposeConfig(ComposeFilter.SEQUENCEFILTER, True, None, MatcherConfig(1))
    with pytest.raises(rustfst_amd.WfstError):
        cfg._c()
    assert cfg._c(matchers=True).contents.compose_filter == 3
    assert callable(rustfst_amd.Context.sigma_batch_stats)


def test_cpp_example_compiles():
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "sigma_batch_tests.cpp")], check=True, capture_output=True)


# ---------------------------------------------------------------- what the GPU tests may expect
def test_seeded_batches_fit_the_kernel():
    """every BFS level of R.compose_sigma is at most 64 wide for the items the GPU test expects in the kernel, at most a
    quarter of each seeded batch is expected on the loop route, no seeded item ends in an error, and the batches exercise
    what they are there for: exact answers, sigma answers, refusals, two sigma arcs in a state, rewritten olabels"""
    refs = B.seeded_references()
    seen = dict.fromkeys(("exact_items", "sigma_items", "refused_items"), 0)
    multi = 0
    assert [len(s) for _, s, _, _ in B.seeded_cases()] == list(B.SIZES) * 6
    for name, strs, t, m2 in B.seeded_cases():
        assert t["props"] & R.I_LABEL_SORTED and all(a[0] != 0 for r in t["rows"] for a in r) and 6 <= len(t["rows"]) <= 20
        assert all(len(s["rows"]) - 1 <= 12 for s in strs)
        loop = 0
        for c, info, widths in refs[name]:
            assert not isinstance(c, str), (name, c)
            if B.in_kernel(info, widths):
                assert max(widths) <= B.WIDTH and info["states"] <= B.SLICE
            else:
                loop += 1
            for k in seen:
                seen[k] += info[k]
            multi += info["sigma_arcs"] > info["sigma_items"]
        assert 4 * loop <= len(strs), name
    assert all(seen.values()) and multi


def test_limit_machines_sit_where_the_tests_say():
    # a level of exactly 64 states, and of 65
    for n, fits in ((64, True), (65, False)):
        c, info, widths = B.reference(B.weighted_string([7]), B.fan_grammar(n), (B.SG, 0, None))
        assert widths == [1, n] and B.in_kernel(info, widths) == fits
    # 70 sigma arcs into 10 states: a sigma range longer than a chunk, a level of 10
    c, info, widths = B.reference(B.weighted_string([7]), B.fan_grammar(70, 10), (B.SG, 0, None))
    assert widths == [1, 10] and info["sigma_arcs"] == 70
    # composed states exactly at the slice, and one beyond
    for m, states in ((57, B.SLICE), (56, B.SLICE + 1)):
        c, info, widths = B.reference(B.weighted_string(B.SLICE_STRING), B.slice_grammar(m), (B.SG, 0, None))
        assert info["states"] == states and max(widths) <= B.WIDTH and B.in_kernel(info, widths) == (states <= B.SLICE)
    # the run of label 300 crosses the first 64-arc chunk of the block
    for n_arcs, sigma_first in ((65, True), (200, True), (200, False)):
        t, sigma = B.long_block_grammar(n_arcs, sigma_first)
        pos = [k for k, a in enumerate(t["rows"][0]) if a[0] == 300]
        assert len(t["rows"][0]) == n_arcs and pos[0] < 64 <= pos[-1] and pos == list(range(pos[0], pos[-1] + 1))
    t, sigma = B.long_block_grammar(65, False)  # ... and here the sigma range does
    pos = [k for k, a in enumerate(t["rows"][0]) if a[0] == sigma]
    assert pos == [62, 63, 64]
    # the tie: both ways into state 3 weigh the same, the first in emission order carries olabel 5
    c, info, widths = B.reference(B.weighted_string([2, 9]), B.tie_grammar(), (B.SG, 2, None))
    assert widths == [1, 2, 1] and [a[1] for r in c["rows"][1:3] for a in r] == [5, 6]
    assert c["rows"][1][0][2] == c["rows"][2][0][2] and c["rows"][0][0][2] == c["rows"][0][1][2]


def test_k21_batch_counts():
    strs, g, m2 = B.k21_batch()
    infos = [B.reference(a, g, m2)[1] for a in strs]
    assert [i["sigma_items"] for i in infos] == [0, 1, 1] and [i["refused_items"] for i in infos] == [1, 0, 0]
    assert all(B.in_kernel(i, B.reference(a, g, m2)[2]) for a, i in zip(strs, infos))
