"""The per-pointer contract of the 17 wfst_ctx_get_*_stats getters: any out-pointer behind ctx may be NULL, and each one
alone receives the counter of its position.  What the counters COUNT is pinned by the limit tests of each family through the
Python dicts; here one context runs one smallest-possible call per family, so that most counters hold something, and every
getter is then read pointer by pointer against the dict its Python accessor returns."""
import ctypes as C

import numpy as np
import pytest

import rustfst_amd
from rustfst_amd import _lib, synth

from oracle.model import content_word_of_flat, rows_flat

from helpers import to_device

INF = np.inf
SENTINEL = 0xA5A5A5A5A5A5A5A5


def flat(rows, finals):
    """rows[s] = [(ilabel, olabel, weight, nextstate)], start state 0, acyclic, under the word computed from the content"""
    f = rows_flat(rows, finals)
    return dict(f, props=int(content_word_of_flat(f)))


def acceptor():
    """4 states, acyclic: two arcs with label 1 leave the start state, an eps:eps arc leaves state 1"""
    rows = [[(1, 1, 0.5, 1), (1, 1, 1.0, 2)], [(0, 0, 0.25, 3)], [(2, 2, 0.5, 3)], []]
    return flat(rows, [INF, INF, INF, 0.0])


def transducer():
    """3 states over the input labels 1 and 2, the last one final with a loop"""
    rows = [[(1, 7, 0.25, 1), (2, 8, 0.25, 1)], [(1, 7, 0.5, 2), (2, 8, 0.5, 2)], [(1, 7, 0.0, 2)]]
    return rows_flat(rows, [INF, INF, 0.0], props=int(synth.I_LABEL_SORTED | synth.O_LABEL_SORTED))


def run_every_family(ctx):
    a, t = to_device(acceptor(), ctx), to_device(transducer(), ctx)
    r = a.rm_epsilon()
    d = r.determinize()
    d.minimize()
    d.push_weights(rustfst_amd.ReweightType.REWEIGHT_TO_INITIAL)
    a.top_sort()
    a.shortest_path()
    a.shortest_path(rustfst_amd.ShortestPathConfig(nshortest=2))
    rustfst_amd.shortest_path_batch([a], rustfst_amd.ShortestPathConfig(nshortest=2), ctx)
    a.compose(t)
    root = to_device(flat([[(1, 1, 0.0, 1)], [(101, 101, 0.5, 2)], []], [INF, INF, 0.0]), ctx)
    item = to_device(flat([[(2, 2, 0.25, 1)], []], [INF, 0.0]), ctx)
    rustfst_amd.replace(100, [(100, root), (101, item)], True)
    rustfst_amd.rm_epsilon_batch([a], ctx)
    rustfst_amd.tr_sum_batch([a], ctx)
    rustfst_amd.determinize_batch([r], ctx=ctx)
    rustfst_amd.minimize_batch([d], ctx=ctx)
    rustfst_amd.optimize_batch([a], ctx)
    rustfst_amd.compose_shortest_path_batch([to_device(synth.linear_acceptor_flat([1, 2, 1]), ctx)], t, ctx=ctx)
    la = rustfst_amd.LookAhead(a)  # one composition the wave answers, one item without a start state
    la.compose_batch([la.relabel(t), la.relabel(rustfst_amd.VectorFst().to_device(ctx))], ctx)
    ctx.synchronize()


def accessor(ctx, family):
    if hasattr(ctx, family + "_stats"):
        return getattr(ctx, family + "_stats")()
    return getattr(rustfst_amd, family + "_stats")(ctx)


def read_alone(fn, ctx, n, i):
    """the getter with out-pointer i alone, the others NULL: (status, the n words behind the n places)"""
    vals = [C.c_uint64(SENTINEL) for _ in range(n)]
    return fn(ctx._h, *[C.byref(v) if k == i else None for k, v in enumerate(vals)]), [v.value for v in vals]


@pytest.mark.gpu
def test_every_getter_pointer_by_pointer(wfst_lib):
    ctx = rustfst_amd.Context(0)
    run_every_family(ctx)
    full = {family: accessor(ctx, family) for family in _lib.COUNTERS}
    opt, bounded = rustfst_amd.optimize_batch_stats(ctx), ctx.bounded_stats()
    for family, stats in list(full.items()) + [("optimize_batch", opt), ("bounded", bounded)]:
        print(family, stats)
    # the calls above ran: what they cannot leave at zero is not zero
    assert full["determinize"]["levels"] > 0 and full["top_sort"]["levels"] > 0 and full["replace"]["states"] > 0
    for family in ("determinize_batch", "minimize_batch", "rm_epsilon_batch", "tr_sum_batch"):
        assert full[family]["items_in_kernel"] + full[family]["items_single"] == 1, family
    assert opt["items_in_kernel"] + opt["items_single"] == 1
    la = full["lookahead"]
    assert (la["items"], la["items_no_start"], la["wave_answered"], la["one_limits"]) == (2, 1, 1, 1)

    for family, (symbol, names) in _lib.COUNTERS.items():
        fn, n = getattr(wfst_lib, symbol), len(names)
        assert list(full[family]) == list(names)
        assert fn(ctx._h, *[None] * n) == 0, symbol
        for i, name in enumerate(names):
            status, vals = read_alone(fn, ctx, n, i)
            want = [SENTINEL] * n
            want[i] = full[family][name]
            assert status == 0 and vals == want, (symbol, name)

    # wfst_ctx_get_optimize_batch_stats: the four launch counts through the first pointer, then three plain counters
    fn = wfst_lib.wfst_ctx_get_optimize_batch_stats
    assert fn(ctx._h, None, None, None, None) == 0
    launches = (C.c_uint64 * 5)(*[SENTINEL] * 5)
    assert fn(ctx._h, launches, None, None, None) == 0
    assert list(launches) == list(opt["launches"].values()) + [SENTINEL]
    for i, name in enumerate(("items_in_kernel", "items_single", "items_transducer")):
        status, vals = read_alone(lambda h, *p: fn(h, None, *p), ctx, 3, i)
        want = [SENTINEL] * 3
        want[i] = opt[name]
        assert status == 0 and vals == want, name

    # wfst_ctx_get_bounded_stats: two plain counters, then the static string
    fn = wfst_lib.wfst_ctx_get_bounded_stats
    assert fn(ctx._h, None, None, None) == 0
    for i, name in enumerate(("stops", "full_solves")):
        status, vals = read_alone(lambda h, *p: fn(h, *p, None), ctx, 2, i)
        want = [SENTINEL] * 2
        want[i] = bounded[name]
        assert status == 0 and vals == want, name
    why = C.c_char_p()
    assert fn(ctx._h, None, None, C.byref(why)) == 0 and (why.value or b"").decode() == bounded["last_reason"]
