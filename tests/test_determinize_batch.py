"""wfst_determinize_batch, wfst_determinize_with_distance and its batch form: the C-ABI surface without a GPU, a Python
restatement of determinize_with_distance (test_determinize's determinize_ref extended with the subsets, the levels and
out_dist) checked against the oracle's shortest distances, and on the device parity of every batch item with the oracle,
the restatement and the single call, the in_kernel flags against their prediction from the level sizes (items on the kernel's
limits and one beyond included), arena growth, distances and error handling."""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest

from rustfst_amd._lib import TR_DTYPE
from oracle import model
import helpers
from helpers import assert_flat_identical, empty_flat, flat_of, golden, random_fst_flat, to_device, to_oracle
import inputs
import determinize_cases as dc
from oracle.model import determinize_ref

ROOT = helpers.ROOT
KDELTA, INF, f32, ACCEPTOR = model.KDELTA, model.INF, model.F32, model.ACCEPTOR
NARROW_STATES, NARROW_CANDS = 256, 8192  # include/wfst.h: the levels the batch kernel keeps
SCRATCH = ("lds", "global")


# ---------------------------------------------------------------- restatement (determinize_static.rs:24-39)
def determinize_with_distance_ref(flat, in_dist=(), delta=KDELTA, max_states=1 << 20):
    """determinize_ref (the same construction, statement by statement) that also returns the subsets, out_dist
    (state_table.rs:25-39,79-96: plus over the subset's elements in stored order of w (x) in_dist[q], q beyond in_dist =
    +inf) and, per breadth-first level, (states, raw candidates): (fst, out_dist, subsets, levels)."""
    if not flat["props"] & ACCEPTOR:
        raise ValueError("transducers are not supported")
    props = model.determinize_props(flat["props"], True)
    if flat["start"] is None or flat["n_states"] == 0:
        return (dict(n_states=0, start=None, offsets=np.zeros(1, np.uint32), arcs=np.zeros(0, TR_DTYPE),
                     finals=np.zeros(0, np.float32), props=props), np.zeros(0, np.float32), [], [])
    in_dist = np.asarray(in_dist, np.float32)
    off, arcs, fin = flat["offsets"], flat["arcs"], flat["finals"]
    tuples = [((int(flat["start"]), f32(0.0)),)]
    by_states = {(int(flat["start"]),): [0]}
    rows, finals, offsets = [], [], [0]

    def find(t):
        ids = by_states.setdefault(tuple(s for s, _ in t), [])
        for i in ids:
            if all(model.approx_eq(w, v) for (_, w), (_, v) in zip(t, tuples[i])):
                return i
        ids.append(len(tuples))
        tuples.append(t)
        if len(tuples) > max_states:
            raise RuntimeError("does not determinize")
        return len(tuples) - 1

    levels = []
    s, level_end = 0, 1
    n_level, k_level = 0, 0
    while s < len(tuples):
        cand = [(int(a["ilabel"]), int(a["nextstate"]), model.times(w, f32(a["weight"])))
                for q, w in tuples[s] for a in arcs[off[q]:off[q + 1]]]
        n_level += 1
        k_level += len(cand)
        cand.sort(key=lambda c: (c[0], c[1]))  # stable
        fw = INF
        for q, w in tuples[s]:
            fw = model.plus(fw, model.times(w, f32(fin[q])))
        i = 0
        while i < len(cand):
            j, weight = i, INF
            while j < len(cand) and cand[j][0] == cand[i][0]:
                weight = model.plus(weight, cand[j][2])
                j += 1
            merged = []
            for _, q, w in cand[i:j]:
                if merged and merged[-1][0] == q:
                    merged[-1][1] = model.plus(merged[-1][1], w)
                else:
                    merged.append([q, w])
            t = tuple((q, model.quantize(f32(w - weight), delta)) for q, w in merged)
            rows.append((cand[i][0], cand[i][0], weight, find(t)))
            i = j
        offsets.append(len(rows))
        finals.append(fw)
        s += 1
        if s == level_end:  # the states created while this level was expanded are the next one
            levels.append((n_level, k_level))
            n_level, k_level, level_end = 0, 0, len(tuples)
    a = np.zeros(len(rows), TR_DTYPE)
    for k, r in enumerate(rows):
        a[k] = r
    out_dist = np.zeros(len(tuples), np.float32)
    for k, t in enumerate(tuples):
        d = INF
        for q, w in t:
            d = model.plus(d, model.times(w, f32(in_dist[q]) if q < len(in_dist) else INF))
        out_dist[k] = d
    fst = dict(n_states=len(tuples), start=0, offsets=np.array(offsets, np.uint32), arcs=a,
               finals=np.array(finals, np.float32), props=props)
    return fst, out_dist, tuples, levels


def predict_in_kernel(flat, delta=KDELTA):
    """1 exactly when no level has more than NARROW_STATES states or NARROW_CANDS raw candidates (wfst.h)"""
    levels = determinize_with_distance_ref(flat, (), delta)[3]
    return int(all(n <= NARROW_STATES and k <= NARROW_CANDS for n, k in levels))


def golden_inputs():
    out = [(c["name"], flat_of(c["fst"]), KDELTA, 0) for c in golden("k12_determinize.json")]
    out += [(c["name"], flat_of(c["fst"]), c["delta"], c["det_type"]) for c in golden("k15_determinize.json")]
    return out


@functools.lru_cache(maxsize=None)
def collision_flat():
    return dc.collision_level(64, 200)


@functools.lru_cache(maxsize=None)
def collision_prediction():
    return predict_in_kernel(collision_flat())


def no_start(n=4):
    f = dc.random_acceptor(np.random.default_rng(3), n, 2, 2, acyclic=True)
    f["start"] = None
    return f


def cyclic_unweighted(seed=21):
    return dc.random_acceptor(np.random.default_rng(seed), 25, 3, 3, max_w=1, p_eps_i=0.1)


def non_determinizing():
    # no twins property: 0 -1/1-> 0, 0 -1/2-> 1, 1 -1/0-> 1 grows one subset per level
    arcs = np.array([(1, 1, 1.0, 0), (1, 1, 2.0, 1), (1, 1, 0.0, 1)], dtype=TR_DTYPE)
    return dict(n_states=2, start=0, offsets=np.array([0, 2, 3], np.uint32), arcs=arcs,
                finals=np.array([np.inf, 0.0], np.float32), props=ACCEPTOR)


def same(got, exp, what, props=True):
    assert_flat_identical(got, exp, what, check_props=props)


# ================================================================ no GPU
NEW_SYMBOLS = ("wfst_determinize_batch", "wfst_determinize_with_distance", "wfst_determinize_with_distance_batch",
               "wfst_ctx_get_determinize_batch_stats")


def test_new_symbols_declared_exported_and_bound(wfst_lib):
    from rustfst_amd import _lib
    with open(os.path.join(ROOT, "include", "wfst.h")) as f:
        header = f.read()
    bound = {name for name, _, _ in _lib.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert re.search(r"\bwfst_status\s+%s\s*\(" % name, header), name
        assert name in bound and hasattr(wfst_lib, name), name
    assert wfst_lib.wfst_abi_version() == 7
    # the limits the in_kernel flag is defined by are part of the header
    assert "256 states" in header and "8192 raw candidates" in header


def test_argument_validation_without_gpu(wfst_lib):
    from rustfst_amd import _lib
    ko = helpers.ko_message
    outs = (C.c_void_p * 3)(1, 1, 1)
    fsts = (C.c_void_p * 3)()
    assert wfst_lib.wfst_determinize_batch(None, None, 0, None, None, None) == 0  # n == 0: OK
    assert "null" in ko(wfst_lib.wfst_determinize_batch(None, fsts, 3, None, None, None))  # NULL outs
    assert "null" in ko(wfst_lib.wfst_determinize_batch(None, None, 3, None, outs, None))
    assert [outs[i] for i in range(3)] == [None] * 3
    bad = _lib.DeterminizeConfig(KDELTA, 3)
    assert "det_type" in ko(wfst_lib.wfst_determinize_batch(None, fsts, 3, C.byref(bad), outs, None))
    assert "det_type" in ko(wfst_lib.wfst_determinize_batch(None, None, 0, C.byref(bad), None, None))
    out, ptr, cnt = C.c_void_p(), C.c_void_p(), C.c_uint64()
    off = (C.c_uint64 * 4)()
    dists = (C.c_void_p * 3)()
    lens = (C.c_uint64 * 3)(0, 5, 0)
    for d in (0.0, -1.0, float("nan"), float("inf")):
        cfg = _lib.DeterminizeConfig(d, 0)
        assert "delta" in ko(wfst_lib.wfst_determinize_batch(None, fsts, 3, C.byref(cfg), outs, None))
        assert "delta" in ko(wfst_lib.wfst_determinize_with_distance(None, None, None, 0, d, C.byref(out), C.byref(ptr),
                                                                     C.byref(cnt)))
        assert "delta" in ko(wfst_lib.wfst_determinize_with_distance_batch(None, fsts, 3, dists, lens, d, outs,
                                                                           C.byref(ptr), off, None))
    # a NULL in_dist with a non-zero length
    msg = ko(wfst_lib.wfst_determinize_with_distance(None, None, None, 4, KDELTA, C.byref(out), C.byref(ptr), C.byref(cnt)))
    assert "in_dist is NULL" in msg
    msg = ko(wfst_lib.wfst_determinize_with_distance_batch(None, fsts, 3, dists, lens, KDELTA, outs, C.byref(ptr), off, None))
    assert "in_dist is NULL" in msg and "item 1" in msg
    assert "null" in ko(wfst_lib.wfst_determinize_with_distance_batch(None, fsts, 3, None, None, KDELTA, outs, C.byref(ptr),
                                                                      off, None))
    assert "null" in ko(wfst_lib.wfst_determinize_with_distance(None, None, None, 0, KDELTA, C.byref(out), C.byref(ptr),
                                                                C.byref(cnt)))
    assert "null" in ko(wfst_lib.wfst_ctx_get_determinize_batch_stats(None, None, None, None))
    # n == 0 of the distance batch: OK, an empty buffer and offsets [0]
    off[0] = 7
    assert wfst_lib.wfst_determinize_with_distance_batch(None, None, 0, None, None, KDELTA, None, C.byref(ptr), off, None) == 0
    assert off[0] == 0 and ptr.value is not None
    wfst_lib.wfst_bytes_destroy(ptr)
    assert out.value is None


def test_python_surface():
    import rustfst_amd
    for name in ("determinize_batch", "determinize_with_distance", "determinize_with_distance_batch",
                 "determinize_batch_stats"):
        assert name in rustfst_amd.__all__ and hasattr(rustfst_amd, name)
    assert list(inspect.signature(rustfst_amd.determinize_batch).parameters) == ["fsts", "config", "ctx", "want_flags"]
    p = inspect.signature(rustfst_amd.determinize_with_distance).parameters
    assert list(p) == ["fst", "in_dist", "delta"] and p["delta"].default == KDELTA
    assert rustfst_amd.determinize_batch([]) == []
    assert rustfst_amd.determinize_with_distance_batch([], []) == []


def test_restatement_equals_determinize_ref():
    for name, flat, delta in dc.parity_inputs():
        got = determinize_with_distance_ref(flat, (), delta)
        same(got[0], determinize_ref(flat, delta), name)
        assert len(got[1]) == got[0]["n_states"] == len(got[2])
        assert sum(n for n, _ in got[3]) == got[0]["n_states"]


def test_restatement_distances_are_reverse_distances(oracle):
    rng = np.random.default_rng(77)
    finite = 0
    for k in range(6):
        flat = dc.random_acceptor(rng, 30 + 5 * k, 4, 3, weight_grid=1, max_w=6, acyclic=True, min_fanout=1)
        flat["finals"][-1] = 2.0  # every state has an arc forward and the last one is final: every distance is finite
        rev = to_oracle(oracle, flat).reverse().shortest_distance()[1:]
        det, out_dist, _, _ = determinize_with_distance_ref(flat, rev)
        assert out_dist[0].view(np.uint32) == rev[flat["start"]].view(np.uint32), f"case {k}: total distance"
        det_rev = to_oracle(oracle, det).reverse().shortest_distance()[1:]
        np.testing.assert_array_equal(out_dist.view(np.uint32), det_rev.view(np.uint32), err_msg=f"case {k}")
        finite += int(np.isfinite(out_dist).all())
    assert finite == 6  # (the check above is not one of +inf against +inf)


def test_in_kernel_prediction_of_the_test_inputs():
    for name, flat, delta in dc.parity_inputs():
        assert predict_in_kernel(flat, delta) == 1, name
    for name, flat, delta, _ in golden_inputs():
        assert predict_in_kernel(flat, delta) == 1, name
    levels = determinize_with_distance_ref(collision_flat())[3]
    assert levels[1] == (64, 25_600)  # 64 states of 2 * 200 arcs (12 800 after merging): more than 8192 raw candidates
    assert collision_prediction() == 0


LIMIT_ITEMS = ("states_256", "states_257", "cands_8192", "cands_8193")  # test_determinize_limits: on a limit, one beyond
LDS_ITEMS = ("lds_496", "lds_497", "lds_alternating")
BATCH_LDS_CANDS = 496  # determinize.hip: the levels whose scratch WFST_DETERMINIZE_BATCH_SCRATCH=lds keeps in LDS


def limit_case(name):
    return dc.case(name)[0]


def test_in_kernel_prediction_of_the_limit_items():
    widest = {}
    for name in LIMIT_ITEMS + LDS_ITEMS:
        levels = determinize_with_distance_ref(limit_case(name))[3]
        widest[name] = (max(n for n, _ in levels), max(k for _, k in levels))
    assert widest["states_256"] == (NARROW_STATES, 256) and widest["states_257"] == (NARROW_STATES + 1, 257)
    assert widest["cands_8192"] == (64, NARROW_CANDS) and widest["cands_8193"] == (64, NARROW_CANDS + 1)
    assert [predict_in_kernel(limit_case(n)) for n in LIMIT_ITEMS] == [1, 0, 1, 0]
    assert widest["lds_496"][1] == BATCH_LDS_CANDS and widest["lds_497"][1] == BATCH_LDS_CANDS + 1
    levels = determinize_with_distance_ref(limit_case("lds_alternating"))[3]
    sides = [k > BATCH_LDS_CANDS for _, k in levels]
    assert sides == [False, True, False, True, False, False, True, False]  # the scratch moves at every level but one
    assert {k for _, k in levels} >= {BATCH_LDS_CANDS, BATCH_LDS_CANDS + 1}
    assert [predict_in_kernel(limit_case(n)) for n in LDS_ITEMS] == [1, 1, 1]


# ================================================================ GPU
def _cfg(delta=KDELTA, det_type=0):
    import rustfst_amd
    return rustfst_amd.DeterminizeConfig(rustfst_amd.DeterminizeType(det_type), delta)


def _batch(devs, ctx, delta=KDELTA, det_type=0):
    import rustfst_amd
    outs, flags = rustfst_amd.determinize_batch(devs, _cfg(delta, det_type), ctx, want_flags=True)
    return [o.to_flat() for o in outs], [int(x) for x in flags]


@pytest.mark.gpu
@pytest.mark.parametrize("scratch", SCRATCH)
def test_parity_with_oracle_and_single_call(gpu_ctx, oracle, monkeypatch, scratch):
    import rustfst_amd
    monkeypatch.setenv("WFST_DETERMINIZE_BATCH_SCRATCH", scratch)
    groups = {}
    for name, flat, delta in dc.parity_inputs():
        groups.setdefault((delta, 0), []).append((name, flat, True))
    for name, flat, delta, det_type in golden_inputs():
        groups.setdefault((delta, det_type), []).append((name, flat, False))
    assert len(groups) >= 4
    for (delta, det_type), items in groups.items():
        devs = [to_device(f, gpu_ctx) for _, f, _ in items]
        got, flags = _batch(devs, gpu_ctx, delta, det_type)
        assert flags == [predict_in_kernel(f, delta) for _, f, _ in items] == [1] * len(items)
        st = rustfst_amd.determinize_batch_stats(gpu_ctx)
        assert st["items_in_kernel"] == len(items) and st["items_single"] == 0 and st["launches"] >= 1
        for (name, flat, weigh_props), g, dev in zip(items, got, devs):
            exp = to_oracle(oracle, flat).determinize_fsa(delta).to_flat()
            exp["props"] = model.determinize_props(flat["props"], det_type != 1)
            same(g, exp, f"{name} {scratch} vs oracle")
            same(g, dev.determinize(_cfg(delta, det_type)).to_flat(), f"{name} {scratch} vs single")


@pytest.mark.gpu
@pytest.mark.parametrize("scratch", SCRATCH)
def test_items_on_the_kernel_limits(gpu_ctx, oracle, monkeypatch, scratch):
    """a level of 256 | 257 states, of 8192 | 8193 raw candidates: the flags and items_single against predict_in_kernel; a
    widest level of 496 | 497 raw candidates and levels on both sides of 496 in turn, under both scratch settings; every
    item bit-identical to the single call and the oracle"""
    import rustfst_amd
    monkeypatch.setenv("WFST_DETERMINIZE_BATCH_SCRATCH", scratch)
    names = LIMIT_ITEMS + LDS_ITEMS
    flats = [limit_case(n) for n in names]
    devs = [to_device(f, gpu_ctx) for f in flats]
    got, flags = _batch(devs, gpu_ctx)
    want = [predict_in_kernel(f) for f in flats]
    assert flags == want == [1, 0, 1, 0, 1, 1, 1]
    st = rustfst_amd.determinize_batch_stats(gpu_ctx)
    assert st["items_single"] == 2 and st["items_in_kernel"] == 5
    for name, flat, g, dev in zip(names, flats, got, devs):
        exp = to_oracle(oracle, flat).determinize_fsa(KDELTA).to_flat()
        exp["props"] = model.determinize_props(flat["props"], True)
        same(g, exp, f"{name} {scratch} vs oracle")
        same(g, dev.determinize().to_flat(), f"{name} {scratch} vs single")
    # the LDS items alone, in the other order: no item leaves the kernel
    got, flags = _batch(devs[:3:-1], gpu_ctx)
    assert flags == [1, 1, 1] and rustfst_amd.determinize_batch_stats(gpu_ctx)["items_single"] == 0
    for name, g, dev in zip(names[:3:-1], got, devs[:3:-1]):
        same(g, dev.determinize().to_flat(), f"{name} {scratch} alone")


@pytest.mark.gpu
@pytest.mark.parametrize("scratch", SCRATCH)
def test_mixed_batch(gpu_ctx, monkeypatch, scratch):
    import rustfst_amd
    monkeypatch.setenv("WFST_DETERMINIZE_BATCH_SCRATCH", scratch)
    rng = np.random.default_rng(8)
    tiny = dc.random_acceptor(rng, 6, 3, 2, acyclic=True)
    flats = [tiny, empty_flat(ACCEPTOR), no_start(), collision_flat(), tiny, inputs.diamond_chain(2000), cyclic_unweighted()]
    devs = [to_device(f, gpu_ctx) for f in flats]
    devs[4] = devs[0]  # the same handle twice
    got, flags = _batch(devs, gpu_ctx)
    want = [1, 1, 1, collision_prediction(), 1, 1, predict_in_kernel(flats[6])]
    assert want[3] == 0 and flags == want
    st = rustfst_amd.determinize_batch_stats(gpu_ctx)
    assert st["items_single"] == 1 and st["items_in_kernel"] == 6
    for k, (g, dev) in enumerate(zip(got, devs)):
        same(g, dev.determinize().to_flat(), f"item {k} {scratch}")
    # the neighbours of the fallback item against the restatement as well
    same(got[2], determinize_ref(flats[2]), "no start state")
    same(got[4], determinize_ref(tiny), "after the fallback item")
    assert got[1]["n_states"] == 0 and got[2]["n_states"] == 0 and got[5]["n_states"] == 2001


@pytest.mark.gpu
@pytest.mark.parametrize("scratch", SCRATCH)
def test_arena_growth(gpu_ctx, monkeypatch, scratch):
    import rustfst_amd
    monkeypatch.setenv("WFST_DETERMINIZE_BATCH_SCRATCH", scratch)
    rng = np.random.default_rng(40)
    flats = [dc.f32_weights(rng, dc.random_acceptor(rng, 40, 4, 3, acyclic=True)) for _ in range(12)]
    devs = [to_device(f, gpu_ctx) for f in flats]
    plain, flags0 = _batch(devs, gpu_ctx)
    monkeypatch.setenv("WFST_DETERMINIZE_BATCH_ARENA", "min")
    got, flags = _batch(devs, gpu_ctx)
    st = rustfst_amd.determinize_batch_stats(gpu_ctx)
    assert st["launches"] > 1 and flags == flags0 == [1] * len(flats)
    for k, (f, g, p) in enumerate(zip(flats, got, plain)):
        same(g, determinize_ref(f), f"item {k} grown")
        same(g, p, f"item {k} grown vs not")


@pytest.mark.gpu
def test_batch_sizes(gpu_ctx):
    rng = np.random.default_rng(300)
    flats = [dc.random_acceptor(rng, int(rng.integers(2, 41)), 4, 2 + k % 3, acyclic=True) for k in range(300)]
    devs = [to_device(f, gpu_ctx) for f in flats]
    got, flags = _batch(devs[:1], gpu_ctx)
    assert flags == [1]
    same(got[0], determinize_ref(flats[0]), "n = 1")
    got, flags = _batch(devs, gpu_ctx)  # more workgroups than compute units
    assert flags == [1] * 300
    for k, (f, g) in enumerate(zip(flats, got)):
        same(g, determinize_ref(f), f"item {k} of 300")


def _same_dist(got, exp, what):
    assert got.dtype == np.float32 and got.shape == exp.shape, f"{what}: {got.shape} != {exp.shape}"
    np.testing.assert_array_equal(got.view(np.uint32), exp.view(np.uint32), err_msg=f"{what}: out_dist (bit pattern)")


@pytest.mark.gpu
def test_distances_single_and_batch(gpu_ctx):
    import rustfst_amd
    rng = np.random.default_rng(55)
    flats = [dc.random_acceptor(rng, 35, 4, 3, weight_grid=1, max_w=6, acyclic=True),
             dc.f32_weights(rng, dc.random_acceptor(rng, 40, 4, 3, acyclic=True)),
             cyclic_unweighted(), dc.random_acceptor(rng, 30, 3, 3, p_eps_i=0.3, acyclic=True), no_start(), collision_flat()]
    devs = [to_device(f, gpu_ctx) for f in flats]

    def in_dists(kind):
        out = []
        for f, dev in zip(flats, devs):
            n = f["n_states"]
            if kind == "reverse":
                d = dev.shortest_distance(reverse=True) if f["start"] is not None else np.zeros(n, np.float32)
            elif kind == "random":
                d = (rng.random(n) * 5).astype(np.float32)
                d[rng.random(n) < 0.3] = np.inf
            elif kind == "short":
                d = (rng.random(n // 2) * 5).astype(np.float32)
            else:
                d = np.zeros(0, np.float32)
            out.append(d)
        return out

    for kind in ("reverse", "random", "short", "empty"):
        ds = in_dists(kind)
        res, flags = rustfst_amd.determinize_with_distance_batch(devs, ds, KDELTA, gpu_ctx, want_flags=True)
        assert [int(x) for x in flags] == [1, 1, 1, 1, 1, 0]
        st = rustfst_amd.determinize_batch_stats(gpu_ctx)
        assert st["items_single"] == 1 and st["items_in_kernel"] == 5
        for k, (f, dev, d, (o, od)) in enumerate(zip(flats, devs, ds, res)):
            got = o.to_flat()
            assert len(od) == got["n_states"], f"{kind} item {k}: the offsets follow the state counts"
            if k < 5:  # (the collision item: against the single call only; 12 800 candidates are slow in Python)
                exp, exp_d, _, _ = determinize_with_distance_ref(f, d)
                same(got, exp, f"{kind} item {k}")
                _same_dist(od, exp_d, f"{kind} item {k}")
            if k < 5 and kind != "reverse":
                continue
            so, sd = rustfst_amd.determinize_with_distance(dev, d)
            same(so.to_flat(), got, f"{kind} item {k}: single vs batch")
            _same_dist(sd, od, f"{kind} item {k}: single vs batch")
            same(so.to_flat(), dev.determinize().to_flat(), f"{kind} item {k}: with distance vs without")
    # reverse distances in, reverse distances of the result out (integer weights: exact)
    rev = devs[0].shortest_distance(reverse=True)
    o, od = rustfst_amd.determinize_with_distance(devs[0], rev)
    _same_dist(od, o.shortest_distance(reverse=True), "out_dist of reverse distances")
    assert od[0] == rev[0] and np.isfinite(od[0])


def _used_bytes():
    import torch
    free, total = torch.cuda.mem_get_info()
    return total - free


@pytest.mark.gpu
def test_ko_leaves_nothing_behind(gpu_ctx, monkeypatch):
    import rustfst_amd
    from rustfst_amd import _lib
    rng = np.random.default_rng(6)
    goods = [dc.random_acceptor(rng, 6, 2, 2, acyclic=True) for _ in range(5)]
    for f in goods:
        assert determinize_ref(f)["n_states"] <= 64
    devs = [to_device(f, gpu_ctx) for f in goods]
    good, _ = _batch(devs, gpu_ctx)
    assert rustfst_amd.determinize_batch_stats(gpu_ctx)["launches"] >= 1  # the sentinel the KO below must clear
    # a transducer word at index 2 of 5: KO before anything is launched
    t = random_fst_flat(rng, 10, 3, 4)
    assert not t["props"] & ACCEPTOR
    mixed = devs[:2] + [to_device(t, gpu_ctx)] + devs[3:]
    n = len(mixed)
    arr = (C.c_void_p * n)(*[d._h.value for d in mixed])
    outs = (C.c_void_p * n)(*([1] * n))
    msg = helpers.ko_message(_lib.lib().wfst_determinize_batch(gpu_ctx._h, arr, n, None, outs, None))
    assert "item 2" in msg and "transducers are not supported" in msg
    assert [outs[i] for i in range(n)] == [None] * n
    assert rustfst_amd.determinize_batch_stats(gpu_ctx) == dict(launches=0, items_in_kernel=0, items_single=0)
    for g, e in zip(_batch(devs, gpu_ctx)[0], good):
        same(g, e, "after the transducer KO")
    # the state limit, hit inside the batch kernel by item 3
    monkeypatch.setenv("WFST_DETERMINIZE_MAX_STATES", "64")
    mixed = devs[:3] + [to_device(non_determinizing(), gpu_ctx)] + devs[3:]
    n = len(mixed)
    arr = (C.c_void_p * n)(*[d._h.value for d in mixed])

    def ko():
        outs = (C.c_void_p * n)(*([1] * n))
        msg = helpers.ko_message(_lib.lib().wfst_determinize_batch(gpu_ctx._h, arr, n, None, outs, None))
        assert "item 3" in msg and "more than" in msg
        assert [outs[i] for i in range(n)] == [None] * n

    for _ in range(3):
        ko()
    for g, e in zip(_batch(devs, gpu_ctx)[0], good):
        same(g, e, "after the limit KO")
    gpu_ctx.synchronize()
    before = _used_bytes()
    for _ in range(50):
        ko()
    gpu_ctx.synchronize()
    assert _used_bytes() == before, "device memory in use grew over 50 KO calls"
    with pytest.raises(rustfst_amd.WfstError, match="item 3"):
        rustfst_amd.determinize_batch(mixed, None, gpu_ctx)
    monkeypatch.delenv("WFST_DETERMINIZE_MAX_STATES")
    for g, e in zip(_batch(devs, gpu_ctx)[0], good):
        same(g, e, "after the Python-level KO")


@pytest.mark.gpu
def test_python_surface_round_trip(gpu_ctx):
    import rustfst_amd
    rng = np.random.default_rng(12)
    flats = [dc.random_acceptor(rng, 12, 3, 3, acyclic=True) for _ in range(4)]
    vs = [to_device(f, gpu_ctx).to_vector_fst() for f in flats]
    devs = [v.to_device(gpu_ctx) for v in vs]
    outs = rustfst_amd.determinize_batch(devs)
    assert len(outs) == 4 and all(isinstance(o, rustfst_amd.DeviceFst) for o in outs)
    for f, v, o in zip(flats, vs, outs):
        same(o.to_flat(), determinize_ref(f), "determinize_batch", props=False)
        back = o.to_vector_fst()
        assert back == rustfst_amd.determinize(v) and back.num_states() == o.num_states
        assert back.to_device(gpu_ctx).to_flat()["n_states"] == o.num_states
