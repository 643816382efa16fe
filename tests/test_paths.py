"""paths_iter without a GPU: the line-by-line restatement tests/paths_ref.py against the hand-worked answers of K23 and against
a second, independent enumerator (depth-first listing, then a stable sort by arc count) on seeded random DAGs — the order
argument of DESIGN.md 3.18 — and the plumbing of the new symbols: declared, exported, bound, named in the version-7 note,
KO on null arguments with the out-pointers untouched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import helpers
import paths_cases as K
import paths_ref
import rustfst_amd
from rustfst_amd import _lib

F32 = np.float32
PATHS_SYMBOLS = ["wfst_fst_count_paths", "wfst_fst_paths", "wfst_fst_paths_batch", "wfst_paths_info", "wfst_paths_download",
                 "wfst_paths_destroy", "wfst_ctx_get_paths_counters"]
PATHS_COUNTERS = ("launches", "items_in_kernel", "items_single", "levels", "paths", "max_path_arcs", "saturated")


def depth_first_then_stable_sort(flat):
    """the second enumerator: every successful path in depth-first order — "end here" before the arcs, the arcs in order —
    then a stable sort by the number of arcs.  Weights: the same left-to-right f32 sum, computed on the way down."""
    if flat["start"] is None or flat["n_states"] == 0:
        return []
    off, arcs, fin = flat["offsets"], flat["arcs"], flat["finals"]
    listed = []

    def rec(s, n_arcs, il, ol, w):
        if not (np.isinf(fin[s]) and fin[s] > 0):
            listed.append((n_arcs, il, ol, paths_ref.times(w, F32(fin[s]))))
        for a in arcs[int(off[s]):int(off[s + 1])]:
            rec(int(a["nextstate"]), n_arcs + 1, il + ((int(a["ilabel"]),) if a["ilabel"] else ()),
                ol + ((int(a["olabel"]),) if a["olabel"] else ()), paths_ref.times(w, F32(a["weight"])))

    rec(int(flat["start"]), 0, (), (), F32(0.0))
    listed.sort(key=lambda p: p[0])  # (list.sort is stable)
    return [p[1:] for p in listed]


@pytest.mark.parametrize("case", K.golden_cases(), ids=lambda c: c["name"])
def test_restatement_reproduces_k23(case):
    paths_ref.assert_rows_equal(paths_ref.paths_iter(K.golden_flat(case)), K.golden_rows(case), case["name"])


def test_k23_covers_the_reference_unit_tests_and_epsilons():
    cases = {c["name"]: c for c in K.golden_cases()}
    assert set(cases) == {"empty_fst", "single_state_start_and_final", "linear_fst", "small_fst_one_final_state",
                          "small_fst_multiple_final_states", "epsilon_transducer"}
    assert [len(cases[n]["paths"]) for n in ("empty_fst", "single_state_start_and_final", "linear_fst",
                                             "small_fst_one_final_state", "small_fst_multiple_final_states")] == [0, 1, 1, 3, 6]
    eps = cases["epsilon_transducer"]["paths"]
    assert any(len(p["ilabels"]) != len(p["olabels"]) for p in eps)
    assert [p["weight"] for p in eps] != sorted(p["weight"] for p in eps)  # the order is not by weight


@pytest.mark.parametrize("block", range(6))
def test_two_enumerators_agree_on_random_dags(block):
    """300 seeded DAGs with epsilons on either tape, parallel arcs, dead ends and several final states: the FIFO and the
    sorted depth-first listing give the same rows in the same order, weight bits included"""
    shapes = set()
    for seed in range(50 * block, 50 * block + 50):
        f = K.random_dag(seed)
        a, b = paths_ref.paths_iter(f), depth_first_then_stable_sort(f)
        paths_ref.assert_rows_equal(b, a, "seed %d" % seed)
        shapes.add(min(len(a), 3))
    assert shapes >= {0, 1, 3}  # machines without a path, with one and with several are all among them


def test_random_dags_have_what_the_order_argument_needs():
    eps_i = eps_o = parallel = dead = multi_final = unequal = 0
    for seed in range(300):
        f = K.random_dag(seed)
        arcs, off = f["arcs"], f["offsets"]
        eps_i += bool(np.any(arcs["ilabel"] == 0))
        eps_o += bool(np.any(arcs["olabel"] == 0))
        parallel += any(len(set(arcs["nextstate"][off[s]:off[s + 1]])) < off[s + 1] - off[s] for s in range(f["n_states"]))
        dead += any(off[s] == off[s + 1] and np.isinf(f["finals"][s]) for s in range(f["n_states"]))
        multi_final += int(np.sum(np.isfinite(f["finals"])) >= 2)
        unequal += any(len(r[0]) != len(r[1]) for r in paths_ref.paths_iter(f))
    assert min(eps_i, eps_o, parallel, dead, multi_final, unequal) >= 30


def test_small_machines_both_enumerators():
    for name, f in K.small_machines().items():
        paths_ref.assert_rows_equal(depth_first_then_stable_sort(f), paths_ref.paths_iter(f), name)
    rows = paths_ref.paths_iter(K.small_machines()["order_of_sum"])
    assert len(rows) == 1 and rows[0][2] == F32(1.0)  # ((1e8 + 1) - 1e8) + 1 in f32; 2.0 or 0.0 in another association
    rows = paths_ref.paths_iter(K.small_machines()["lex_not_state"])
    assert [r[0] for r in rows] == [(1, 7), (2, 4), (2, 5), (3, 6), (1, 8, 6)]
    assert np.isinf(paths_ref.paths_iter(K.small_machines()["inf_arc"])[0][2])
    for name, f in K.cyclic_machines().items():
        with pytest.raises(RuntimeError, match="does not drain"):
            paths_ref.paths_iter(f, max_steps=5000)


def test_restatement_agrees_with_the_brute_force_of_the_nbest_tests():
    """helpers.enumerate_paths — the depth-first brute force the n-best tests use, which keeps epsilons — lists the same
    paths once its labels are stripped"""
    for seed in range(40):
        f = K.random_dag(seed)
        brute = sorted((tuple(x for x in il if x), tuple(x for x in ol if x), float(w)) for w, il, ol in helpers.enumerate_paths(f))
        mine = sorted((il, ol, float(w)) for il, ol, w in paths_ref.paths_iter(f))
        assert brute == mine, seed


# ---------------------------------------------------------------- plumbing
def _header():
    with open(os.path.join(helpers.ROOT, "include", "wfst.h")) as f:
        return f.read()


def test_symbols_declared_exported_bound_and_in_the_version_note(wfst_lib):
    header = _header()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    bound = {n for n, _, _ in _lib.SYMBOLS}
    note = re.search(r"#define\s+WFST_ABI_VERSION\s+7\b(.*)", header).group(1).split("; 6:")[0]
    for name in PATHS_SYMBOLS:
        assert re.search(r"\bwfst_status\s+%s\s*\(" % name, code), name
        assert hasattr(wfst_lib, name), name
        assert name in bound, name
        assert re.search(r"\b%s\b" % name, note), name
    assert wfst_lib.wfst_abi_version() == 7
    assert "typedef struct wfst_paths wfst_paths;" in code
    assert helpers.header_params(header, "wfst_fst_paths_batch") == \
        "wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, uint64_t max_paths, wfst_paths** out, uint8_t* in_kernel"
    assert re.search(r"#define\s+WFST_PATHS_BATCH_MAX_STATES\s+%d\b" % K.BATCH_MAX_STATES, code)
    assert re.search(r"#define\s+WFST_PATHS_BATCH_MAX_ARCS\s+%d\b" % K.BATCH_MAX_ARCS, code)


def test_python_surface():
    for name in ("FstPath", "PathTable", "paths_batch"):
        assert hasattr(rustfst_amd, name) and name in rustfst_amd.__all__
    for cls, name in ((rustfst_amd.DeviceFst, "paths"), (rustfst_amd.DeviceFst, "count_paths"), (rustfst_amd.VectorFst, "paths_iter"),
                      (rustfst_amd.Context, "paths_counters")):
        assert callable(getattr(cls, name))
    assert rustfst_amd.FstPath([1], [2], 0.5) == rustfst_amd.FstPath([1], [2], 0.5)
    assert rustfst_amd.FstPath([1], [2], 0.0) != rustfst_amd.FstPath([1], [2], -0.0)  # weights by their bits
    from rustfst_amd import build
    assert "paths.hip" in build.SOURCES


def test_path_table_views():
    """PathTable over hand-made arrays: rows, item(i) with rebased offsets, no copy of the label arrays"""
    t = rustfst_amd.PathTable(np.array([0, 2, 2, 3], np.uint64), np.array([0.5, 1.5, 2.5], np.float32),
                              np.array([0, 1, 3, 3], np.uint64), np.array([7, 8, 9], np.uint32),
                              np.array([0, 0, 1, 3], np.uint64), np.array([4, 5, 6], np.uint32))
    assert len(t) == 3 and t.num_items == 3
    assert list(t) == [rustfst_amd.FstPath([7], [], 0.5), rustfst_amd.FstPath([8, 9], [4], 1.5), rustfst_amd.FstPath([], [5, 6], 2.5)]
    assert t[-1] == t[2] and t[0:2] == [t[0], t[1]]
    assert [len(t.item(i)) for i in range(3)] == [2, 0, 1]
    last = t.item(2)
    assert list(last) == [t[2]] and list(last.ilabel_off) == [0, 0] and list(last.olabel_off) == [0, 2]
    assert np.shares_memory(last.olabels, t.olabels)
    assert paths_ref.table_rows(t) == [((7,), (), F32(0.5)), ((8, 9), (4,), F32(1.5)), ((), (5, 6), F32(2.5))]
    with pytest.raises(IndexError):
        t.item(3)
    with pytest.raises(IndexError):
        t[3]


def test_counter_getter(wfst_lib):
    header = helpers.check_counter_getter(wfst_lib, "wfst_ctx_get_paths_counters", PATHS_COUNTERS, rustfst_amd.Context.paths_counters)
    assert _lib.PATHS_COUNTERS == PATHS_COUNTERS
    assert "wfst_ctx_get_paths_counters" not in {symbol for symbol, _ in _lib.COUNTERS.values()}
    # the struct behind it: uint64_t fields only, in the getter's order
    with open(os.path.join(helpers.ROOT, "rustfst_amd", "csrc", "common.h")) as f:
        body = re.search(r"struct PathsCounters \{(.*?)\};", f.read(), re.S).group(1)
    fields = [d.split("=")[0].strip() for stmt in re.findall(r"\buint64_t\s+([^;]*);", body) for d in stmt.split(",")]
    assert tuple(fields) == PATHS_COUNTERS and re.sub(r"\buint64_t\s+[^;]*;", "", body).strip() == ""
    assert "wfst_ctx_get_paths_stats" not in header  # (the table of the *_stats getters has a fixed size: tests/test_host.py)


def test_null_arguments_are_ko_and_leave_the_out_pointers(wfst_lib):
    L = wfst_lib
    count, out, dummy = C.c_uint64(5), C.c_void_p(0x1234), C.c_void_p(1)
    arr = (C.c_void_p * 1)(None)
    flags = (C.c_uint8 * 1)(9)
    assert "null" in helpers.ko_message(L.wfst_fst_count_paths(None, None, C.byref(count)))
    assert count.value == 5
    assert "null" in helpers.ko_message(L.wfst_fst_paths(None, None, 10, C.byref(out)))
    assert "null" in helpers.ko_message(L.wfst_fst_paths(None, dummy, 10, None))
    assert "null" in helpers.ko_message(L.wfst_fst_paths_batch(None, arr, 1, 10, C.byref(out), flags))
    assert "null" in helpers.ko_message(L.wfst_fst_paths_batch(None, None, 0, 10, C.byref(out), None))  # n == 0 needs a context too
    assert out.value == 0x1234 and flags[0] == 9
    assert "null" in helpers.ko_message(L.wfst_paths_info(None, C.byref(count), None, None, None))
    assert count.value == 5
    assert "null" in helpers.ko_message(L.wfst_paths_download(None, None, None, None, None, None, None, None))
    assert L.wfst_paths_destroy(None) == 0  # like free(NULL)
