"""paths at the limits of its routes and of its walk.  The batch kernel counts items of at most 4096 states and 16384 arcs
(WFST_PATHS_BATCH_MAX_STATES / _ARCS); an item beyond either is counted by the device-wide launches and lands in the same
table, so only in_kernel and the counters of wfst_ctx_get_paths_counters show which route ran.  For each limit an item
exactly on it and one past it; and the shapes where the walk can go wrong: a start state with 63, 64, 65 and 4097 arcs
(the wave boundary and the binary search over the arc prefixes), a chain of 5000 states (depth >> width), a state reached
at two depths.  Everything is compared with tests/paths_ref.py bit for bit.  Without a GPU: every input is on the limit it is
built for."""
import numpy as np
import pytest

import paths_cases as K
import paths_ref
import rustfst_amd
from helpers import to_device

S, A = K.BATCH_MAX_STATES, K.BATCH_MAX_ARCS
LIMIT_ITEMS = {  # name -> (n_states, n_arcs, in_kernel)
    "on_states": (S, S + 10, 1), "past_states": (S + 1, S + 10, 0),
    "on_arcs": (64, A, 1), "past_arcs": (64, A + 1, 0),
    "on_both": (S, A, 1), "past_both": (S + 1, A + 1, 0),
}


def test_inputs_are_on_their_limits():
    for name, (n, e, in_kernel) in LIMIT_ITEMS.items():
        f = K.sized(n, e)
        assert f["n_states"] == n and len(f["arcs"]) == e and f["offsets"][-1] == e
        assert in_kernel == (n <= S and e <= A), name
        assert len(paths_ref.paths_iter(f)) == 6
    for k in (63, 64, 65, 4097):
        f = K.fan(k)
        assert f["offsets"][1] - f["offsets"][0] == k
    assert K.chain(5000)["n_states"] == 5001
    assert len(paths_ref.paths_iter(K.diamonds(4))) == 16


@pytest.fixture(scope="module")
def limit_refs():
    """the restatement's rows of every limit item, computed once"""
    return {name: paths_ref.paths_iter(K.sized(n, e)) for name, (n, e, _) in LIMIT_ITEMS.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("k", [63, 64, 65, 4097])
def test_wide_start_state(gpu_ctx, k):
    """paths of one and of two arcs alternate along the start state's arcs: the ranks of the two-arc paths lie between
    those of the one-arc paths, and the final order pulls them apart"""
    f = K.fan(k, tail=3)
    exp = paths_ref.paths_iter(f)
    assert len(exp) == (k + 1) // 2 + 3 * (k // 2)
    d = to_device(f, gpu_ctx)
    paths_ref.assert_rows_equal(paths_ref.table_rows(d.paths()), exp, "fan %d" % k)
    assert gpu_ctx.paths_counters()["max_path_arcs"] == (2 if k > 1 else 1)
    t = rustfst_amd.paths_batch([d, d], ctx=gpu_ctx)
    for i in range(2):
        paths_ref.assert_rows_equal(paths_ref.table_rows(t.item(i)), exp, "fan %d in a list, item %d" % (k, i))


@pytest.mark.gpu
def test_deep_chain(gpu_ctx):
    f = K.chain(5000)
    exp = paths_ref.paths_iter(f)
    assert len(exp) == 6  # the states 0, 1000, .. 5000 are final
    d = to_device(f, gpu_ctx)
    paths_ref.assert_rows_equal(paths_ref.table_rows(d.paths()), exp, "chain")
    c = gpu_ctx.paths_counters()
    assert c["levels"] == 5001 and c["max_path_arcs"] == 5000 and c["items_single"] == 1
    t, flags = rustfst_amd.paths_batch([d], ctx=gpu_ctx, return_in_kernel=True)  # 5001 states: past the batch limit
    assert list(flags) == [0]
    paths_ref.assert_rows_equal(paths_ref.table_rows(t), exp, "chain in a list")


@pytest.mark.gpu
def test_state_reached_at_two_depths(gpu_ctx):
    # state 3 is reached over one arc and over a chain of three; its subtree is walked at both depths
    rows = [[(1, 1, 0.5, 1), (2, 2, 0.25, 3)], [(3, 3, 0.5, 2)], [(4, 0, 0.125, 3)], [(5, 5, 1.0, 4), (6, 6, 2.0, 5)], [(7, 7, 0.0, 5)], []]
    f = K.fst(rows, K.finals_of(6, {3: 0.75, 5: 0.0}))
    exp = paths_ref.paths_iter(f)
    assert len(exp) == 6  # three ways on from state 3 (end there, 3 -> 5, 3 -> 4 -> 5), for each of the two ways into it
    for route in ("single", "batch"):
        d = to_device(f, gpu_ctx)
        t = d.paths() if route == "single" else rustfst_amd.paths_batch([d], ctx=gpu_ctx)
        paths_ref.assert_rows_equal(paths_ref.table_rows(t), exp, route)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(LIMIT_ITEMS))
def test_batch_limit(gpu_ctx, limit_refs, name):
    n, e, in_kernel = LIMIT_ITEMS[name]
    small = K.small_machines()["lex_not_state"]
    flats = [small, K.sized(n, e), small]
    t, flags = rustfst_amd.paths_batch([to_device(f, gpu_ctx) for f in flats], ctx=gpu_ctx, return_in_kernel=True)
    c = gpu_ctx.paths_counters()
    assert list(flags) == [1, in_kernel, 1]
    assert c["items_in_kernel"] == 2 + in_kernel and c["items_single"] == 1 - in_kernel
    assert c["levels"] == n - 1 and c["max_path_arcs"] == n - 2 and c["paths"] == 6 + 2 * 5
    if in_kernel:
        assert c["launches"] == 7
    else:
        assert c["launches"] > 7 + 2 * (n - 2)  # a launch per level of the search and of the peel
    paths_ref.assert_rows_equal(paths_ref.table_rows(t.item(1)), limit_refs[name], name)
    for i in (0, 2):
        paths_ref.assert_rows_equal(paths_ref.table_rows(t.item(i)), paths_ref.paths_iter(small), "%s neighbour %d" % (name, i))


@pytest.mark.gpu
def test_mixed_list_with_items_beyond_each_limit(gpu_ctx, limit_refs):
    m = K.small_machines()
    names = ["past_states", "on_arcs", "past_arcs"]
    flats = [m["empty"], m["no_start"], m["linear"], K.sized(*LIMIT_ITEMS["past_states"][:2]), m["lex_not_state"],
             K.sized(*LIMIT_ITEMS["on_arcs"][:2]), K.sized(*LIMIT_ITEMS["past_arcs"][:2]), m["parallel"]]
    ds = [to_device(f, gpu_ctx) for f in flats]
    t, flags = rustfst_amd.paths_batch(ds, ctx=gpu_ctx, return_in_kernel=True)
    assert list(flags) == [1, 1, 1, 0, 1, 1, 0, 1]
    c = gpu_ctx.paths_counters()
    assert c["items_in_kernel"] == 6 and c["items_single"] == 2
    for i, f in enumerate(flats):
        exp = limit_refs[names[(3, 5, 6).index(i)]] if i in (3, 5, 6) else paths_ref.paths_iter(f)
        paths_ref.assert_rows_equal(paths_ref.table_rows(t.item(i)), exp, "item %d" % i)
    # a cyclic item beyond the limit, behind a cyclic item within it: the lower index is reported
    big_cycle = K.sized(S + 1, S + 10)
    big_cycle["arcs"]["nextstate"][-1] = 0
    cyc = [ds[2], to_device(K.cyclic_machines()["cycle_behind_final"], gpu_ctx), to_device(big_cycle, gpu_ctx)]
    with pytest.raises(rustfst_amd.WfstError, match="item 1: paths: a cycle is accessible"):
        rustfst_amd.paths_batch(cyc, ctx=gpu_ctx)
    with pytest.raises(rustfst_amd.WfstError, match="item 1: paths: a cycle is accessible"):
        rustfst_amd.paths_batch([cyc[0], cyc[2]], ctx=gpu_ctx)
