"""paths_iter on the device (wfst_fst_paths, wfst_fst_count_paths, wfst_fst_paths_batch) against the line-by-line restatement
tests/paths_ref.py, bit for bit: labels, offsets, order and weight bits.  The edge machines, K23, the weights whose sum
depends on the order, cycles, the count bound, the list form against the loop of single calls, and the n-best results of a
decoding batch handed over without a download."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import helpers
import paths_cases as K
import paths_ref
import rustfst_amd
from helpers import to_device
from rustfst_amd import _lib

pytestmark = pytest.mark.gpu

MSG_CYCLE = "paths: a cycle is accessible from the start state: the reference's paths_iter never returns"


def check_table_shape(t):
    """what every table satisfies, whatever it holds"""
    P = len(t.weights)
    assert len(t.ilabel_off) == len(t.olabel_off) == P + 1
    assert t.ilabel_off[0] == 0 and t.olabel_off[0] == 0
    assert np.all(np.diff(t.ilabel_off.astype(np.int64)) >= 0) and np.all(np.diff(t.olabel_off.astype(np.int64)) >= 0)
    assert t.ilabel_off[-1] == len(t.ilabels) and t.olabel_off[-1] == len(t.olabels)
    assert t.item_off[0] == 0 and t.item_off[-1] == P and np.all(np.diff(t.item_off.astype(np.int64)) >= 0)
    assert not np.any(t.ilabels == 0) and not np.any(t.olabels == 0)


def check_single(ctx, flat, what):
    d = to_device(flat, ctx)
    exp = paths_ref.paths_iter(flat)
    t = d.paths()
    check_table_shape(t)
    paths_ref.assert_rows_equal(paths_ref.table_rows(t), exp, what)
    c = ctx.paths_counters()
    assert c["items_single"] == 1 and c["items_in_kernel"] == 0 and c["paths"] == len(exp) and c["saturated"] == 0, (what, c)
    assert d.count_paths() == len(exp), what
    assert ctx.paths_counters()["paths"] == len(exp) and ctx.paths_counters()["max_path_arcs"] == 0  # (the count walks no path)
    helpers.assert_flat_identical(d.to_flat(), flat, what + ": the operand")  # left as it is
    return t, c


@pytest.mark.parametrize("name", sorted(K.small_machines()))
def test_small_machines(gpu_ctx, name):
    flat = K.small_machines()[name]
    t, c = check_single(gpu_ctx, flat, name)
    if name in ("empty", "no_start", "lone_nonfinal_start"):
        assert len(t) == 0 and c["max_path_arcs"] == 0
    if name == "lone_final_start":
        assert list(t) == [rustfst_amd.FstPath([], [], 2.5)]
    if name == "order_of_sum":
        assert t.weights[0] == np.float32(1.0)
    if name == "inf_arc":
        assert np.isposinf(t.weights[0]) and np.isfinite(t.weights[1])
    if name == "unequal_tapes":
        assert any(len(p.ilabels) != len(p.olabels) for p in t)
    if name == "linear":
        assert c["max_path_arcs"] == 3 and c["levels"] == 4


@pytest.mark.parametrize("case", K.golden_cases(), ids=lambda c: c["name"])
def test_k23(gpu_ctx, case):
    t = to_device(K.golden_flat(case), gpu_ctx).paths()
    paths_ref.assert_rows_equal(paths_ref.table_rows(t), K.golden_rows(case), case["name"])


def test_random_dags(gpu_ctx):
    for seed in range(60):
        check_single(gpu_ctx, K.random_dag(seed), "seed %d" % seed)


@pytest.mark.parametrize("word", [0, K.ACYCLIC, K.CYCLIC], ids=["unknown", "acyclic", "cyclic"])
def test_cycles(gpu_ctx, word):
    """the verdict comes from the content, whatever the stored word says about cycles"""
    for name, flat in K.cyclic_machines().items():
        if word == K.ACYCLIC:
            continue  # (a word that states ACYCLIC of a cyclic machine is a lie, not an input)
        d = to_device(K.with_word(flat, word), gpu_ctx)
        with pytest.raises(rustfst_amd.WfstError) as e:
            d.paths()
        assert MSG_CYCLE in str(e.value), name
        with pytest.raises(rustfst_amd.WfstError) as e:
            d.count_paths()
        assert MSG_CYCLE in str(e.value), name
    for name in ("inaccessible_cycle", "two_depths", "parallel"):
        flat = K.small_machines()[name]
        if word == K.CYCLIC and name != "inaccessible_cycle":
            continue
        check_single(gpu_ctx, K.with_word(flat, word), name)
    # the context works after a KO
    check_single(gpu_ctx, K.small_machines()["linear"], "after a KO")


def test_max_paths_bound(gpu_ctx):
    flat = K.small_machines()["lex_not_state"]
    P = len(paths_ref.paths_iter(flat))
    d = to_device(flat, gpu_ctx)
    assert len(d.paths(max_paths=P)) == P
    with pytest.raises(rustfst_amd.WfstError, match=r"paths: the FST has %d paths, more than max_paths \(%d\)" % (P, P - 1)):
        d.paths(max_paths=P - 1)
    c = gpu_ctx.paths_counters()
    assert c["paths"] == P and c["max_path_arcs"] == 0  # refused before any path was walked
    with pytest.raises(rustfst_amd.WfstError, match="more than max_paths"):
        d.paths(max_paths=0)


def test_seventy_diamonds_saturate(gpu_ctx):
    d = to_device(K.diamonds(70), gpu_ctx)
    assert d.count_paths() == (1 << 64) - 1
    assert gpu_ctx.paths_counters()["saturated"] == 1
    for bound in (1 << 20, (1 << 64) - 1):
        with pytest.raises(rustfst_amd.WfstError, match=r"paths: the FST has 18446744073709551615 paths, more than max_paths \(%d\): the count is saturated" % bound):
            d.paths(max_paths=bound)
        assert gpu_ctx.paths_counters()["saturated"] == 1
    with pytest.raises(rustfst_amd.WfstError, match=r"item 1: paths: the FST has 18446744073709551615 paths, more than max_paths"):
        rustfst_amd.paths_batch([to_device(K.small_machines()["linear"], gpu_ctx), d], ctx=gpu_ctx)
    assert gpu_ctx.paths_counters()["saturated"] == 1
    # 63 diamonds still count exactly
    assert to_device(K.diamonds(63), gpu_ctx).count_paths() == 1 << 63
    assert gpu_ctx.paths_counters()["saturated"] == 0


def test_vector_fst_paths_iter(gpu_ctx):
    f = rustfst_amd.VectorFst()
    s1, s2, s3, s4 = (f.add_state() for _ in range(4))
    f.set_start(s1)
    f.set_final(s4, 18.0)
    for s, (l, w, ns) in ((s1, (1, 1.0, s2)), (s1, (2, 2.0, s3)), (s1, (3, 3.0, s4)), (s2, (4, 4.0, s4)), (s3, (5, 5.0, s4))):
        f.add_tr(s, rustfst_amd.Tr(l, l, w, ns))
    assert list(f.paths_iter()) == [rustfst_amd.FstPath([3], [3], 21.0), rustfst_amd.FstPath([1, 4], [1, 4], 23.0),
                                    rustfst_amd.FstPath([2, 5], [2, 5], 25.0)]


# ---------------------------------------------------------------- the list form
def check_batch(ctx, flats, what, max_paths=1 << 20):
    ds = [to_device(f, ctx) for f in flats]
    t, flags = rustfst_amd.paths_batch(ds, max_paths, ctx, return_in_kernel=True)
    c = ctx.paths_counters()
    check_table_shape(t)
    assert t.num_items == len(flats)
    for i, f in enumerate(flats):
        paths_ref.assert_rows_equal(paths_ref.table_rows(t.item(i)), paths_ref.paths_iter(f), "%s item %d" % (what, i))
    assert c["items_in_kernel"] == int(flags.sum()) and c["items_single"] == len(flats) - int(flags.sum())
    assert c["paths"] == len(t)
    return t, flags, c, ds


def test_batch_equals_loop_of_single_calls(gpu_ctx):
    m = K.small_machines()
    flats = [m["empty"], m["no_start"], m["linear"], m["lex_not_state"], m["lone_final_start"], m["unequal_tapes"], m["order_of_sum"],
             m["inaccessible_cycle"], m["negative_zero"], m["non_coaccessible"]] + [K.random_dag(s) for s in range(30)]
    t, flags, c, ds = check_batch(gpu_ctx, flats, "mixed")
    assert flags.all() and c["items_single"] == 0
    # against the single calls' tables, array for array
    for i, d in enumerate(ds):
        one, part = d.paths(), t.item(i)
        for k in ("weights", "ilabel_off", "ilabels", "olabel_off", "olabels"):
            a, b = getattr(one, k), getattr(part, k)
            assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b), (i, k)


def test_batch_launches_do_not_depend_on_length_or_depth(gpu_ctx):
    shallow = [K.random_dag(s) for s in range(3)]
    c3 = check_batch(gpu_ctx, shallow, "3 items")[2]
    c300 = check_batch(gpu_ctx, [K.random_dag(s) for s in range(300)], "300 items")[2]
    deep = [K.chain(700), K.fan(65), K.chain(1500)]
    cdeep = check_batch(gpu_ctx, deep, "deep items")[2]
    assert c3["launches"] == c300["launches"] == cdeep["launches"] == 7
    assert cdeep["levels"] == 1501 and cdeep["max_path_arcs"] == 1500 and c3["levels"] <= 9
    # a list without any path stops behind the count
    none = check_batch(gpu_ctx, [K.small_machines()["lone_nonfinal_start"]] * 2, "no paths")[2]
    assert none["launches"] == 1 and none["paths"] == 0
    # and a list whose items need no launch at all
    assert check_batch(gpu_ctx, [K.small_machines()["empty"], K.small_machines()["no_start"]], "nothing to count")[2]["launches"] == 0


def test_batch_first_ko_is_the_lowest_index(gpu_ctx):
    m, cyc = K.small_machines(), K.cyclic_machines()
    flats = [m["linear"], m["parallel"], cyc["cycle_without_final"], m["linear"], m["two_depths"], cyc["self_loop_on_start"]]
    ds = [to_device(f, gpu_ctx) for f in flats]
    with pytest.raises(rustfst_amd.WfstError) as e:
        rustfst_amd.paths_batch(ds, ctx=gpu_ctx)
    assert "item 2: " + MSG_CYCLE in str(e.value) and "item 5" not in str(e.value)
    # the count bound applies per item: item 1 has six paths, the list seven
    with pytest.raises(rustfst_amd.WfstError, match=r"item 1: paths: the FST has 6 paths, more than max_paths \(5\)"):
        rustfst_amd.paths_batch(ds[:2], 5, gpu_ctx)
    assert len(rustfst_amd.paths_batch(ds[:2], 6, gpu_ctx)) == 7
    # the context works on
    check_batch(gpu_ctx, flats[:2], "after a KO")


def test_batch_refuses_foreign_handles_and_null_entries(gpu_ctx):
    import ctypes as C
    other = rustfst_amd.Context(0)
    mine, theirs = to_device(K.small_machines()["linear"], gpu_ctx), to_device(K.small_machines()["linear"], other)
    with pytest.raises(rustfst_amd.WfstError, match="item 1: paths_batch: the FST belongs to another context"):
        rustfst_amd.paths_batch([mine, theirs], ctx=gpu_ctx)
    assert gpu_ctx.paths_counters() == dict.fromkeys(_lib.PATHS_COUNTERS, 0)
    with pytest.raises(rustfst_amd.WfstError, match="paths: the FST belongs to another context"):
        rustfst_amd.DeviceFst(theirs._h, gpu_ctx, owner=theirs).paths()
    out = C.c_void_p(0x1234)
    arr = (C.c_void_p * 2)(mine._h.value if isinstance(mine._h, C.c_void_p) else mine._h, None)
    assert "item 1: null FST in batch" in helpers.ko_message(_lib.lib().wfst_fst_paths_batch(gpu_ctx._h, arr, 2, 10, C.byref(out), None))
    assert out.value == 0x1234
    # n == 0: a table of no items
    t = rustfst_amd.paths_batch([], ctx=gpu_ctx)
    assert len(t) == 0 and t.num_items == 0 and list(t.item_off) == [0] and list(t.ilabel_off) == [0]


def test_nbest_of_a_decoding_batch(gpu_ctx):
    """compose_batch -> shortest_path_batch(nshortest = 10) -> paths_batch, handles only: every table item equals the
    restatement on the downloaded n-best FST"""
    import compose_batch_cases as cb
    pairs = cb.random_pairs()[:36]
    d1 = [to_device(a, gpu_ctx) for a, _ in pairs]
    d2 = [to_device(b, gpu_ctx) for _, b in pairs]
    lattices = rustfst_amd.compose_batch(d1, d2, None, gpu_ctx)
    nbest = rustfst_amd.shortest_path_batch(lattices, rustfst_amd.ShortestPathConfig(nshortest=10), gpu_ctx)
    t, flags = rustfst_amd.paths_batch(nbest, ctx=gpu_ctx, return_in_kernel=True)
    c = gpu_ctx.paths_counters()
    assert flags.all() and c["launches"] <= 7 and t.num_items == len(pairs)
    sizes = []
    for i, d in enumerate(nbest):
        rows = paths_ref.table_rows(t.item(i))
        paths_ref.assert_rows_equal(rows, paths_ref.paths_iter(d.to_flat()), "item %d" % i)
        assert len(rows) <= 10
        sizes.append(len(rows))
    assert max(sizes) == 10 and sum(1 for s in sizes if s > 1) >= 10  # the batch does hold n-best results


def test_cpp_paths_iterator_tests_run(gpu_ctx, tmp_path):
    """examples/paths_iterator_tests.cpp: the reference's five tests of paths_iter against include/wfst.hpp, end to end"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = tmp_path / "paths_iterator_tests"
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(helpers.ROOT, "include"),
                    os.path.join(helpers.ROOT, "examples", "paths_iterator_tests.cpp"), "-L", libdir, "-lwfst_amd",
                    f"-Wl,-rpath,{libdir}", "-Wl,--allow-shlib-undefined", "-o", str(exe)], check=True)
    env = dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all paths_iterator tests passed" in r.stdout, r.stdout + r.stderr
