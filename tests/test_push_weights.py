"""shortest_distance(fst, reverse), reweight and push_weights (wfst_shortest_distance_with_config, wfst_reweight,
wfst_push_weights): C-ABI surface without a GPU, the K14 known answers, and on the device parity with a restatement of
rustfst's algorithms/reweight.rs + push.rs (oracle/model/push.py) over the oracle's distances, plus invariants that do not
depend on that restatement."""
import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest

from rustfst_amd import synth
from rustfst_amd._lib import TR_DTYPE

from oracle.model import (ACCESSIBLE, ACYCLIC, ALL, ARC_RELEVANT, COACCESSIBLE, CYCLIC, DFS_BITS, INITIAL_ACYCLIC,
                          INITIAL_CYCLIC, NOT_ACCESSIBLE, WEIGHT_INVARIANT, csr_next, dfs_bits, graph_facts, is_one,
                          is_zero, p_add_state, p_add_tr, p_set_final, p_set_start, push_ref, reach, reverse_len_rule,
                          reweight_ref, to_flat, transpose)
from helpers import ROOT, _oracle_dist, assert_same, ko_message, random_fst_flat, to_device, to_oracle

GOLDEN = os.path.join(ROOT, "tests", "golden", "k14_push.json")
NEW_SYMBOLS = ("wfst_shortest_distance_with_config", "wfst_push_weights", "wfst_reweight")


# ---------------------------------------------------------------- inputs
def golden_cases():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def k14_flat(c):
    arcs = np.array([tuple(a) for a in c["arcs"]], dtype=TR_DTYPE) if c["arcs"] else np.zeros(0, dtype=TR_DTYPE)
    fin = np.array([np.inf if f is None else f for f in c["finals"]], dtype=np.float32)
    return dict(n_states=c["n_states"], start=c["start"], offsets=np.array(c["offsets"], dtype=np.uint32), arcs=arcs,
                finals=fin, props=int(c["props"], 16))


def golden_expected(c):
    e = c["expected"]
    arcs = np.array([tuple(a) for a in e["arcs"]], dtype=TR_DTYPE) if e["arcs"] else np.zeros(0, dtype=TR_DTYPE)
    fin = np.array([np.inf if f is None else f for f in e["finals"]], dtype=np.float32)
    return dict(n_states=e["n_states"], start=e["start"], offsets=np.array(e["offsets"], dtype=np.uint32), arcs=arcs,
                finals=fin, props=int(e["props"], 16))


# ================================================================ no GPU
def test_new_symbols_declared_and_bound(wfst_lib):
    from rustfst_amd import _lib
    with open(os.path.join(ROOT, "include", "wfst.h")) as f:
        header = f.read()
    bound = {name for name, _, _ in _lib.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert re.search(r"\bwfst_status\s+" + name + r"\s*\(", header), name
        assert name in bound, name
        assert hasattr(wfst_lib, name), name


def test_config_structs_match_the_header():
    from rustfst_amd import _lib
    assert C.sizeof(_lib.ShortestDistanceConfig) == 8
    assert _lib.ShortestDistanceConfig.reverse.offset == 0 and _lib.ShortestDistanceConfig.delta.offset == 4
    assert C.sizeof(_lib.PushWeightsConfig) == 8
    assert _lib.PushWeightsConfig.delta.offset == 0 and _lib.PushWeightsConfig.remove_total_weight.offset == 4


def test_argument_validation_without_gpu(wfst_lib):
    from rustfst_amd import _lib
    out = C.c_void_p()
    assert "reweight_type" in ko_message(wfst_lib.wfst_reweight(None, None, None, 0, 2, C.byref(out)))
    assert "potentials" in ko_message(wfst_lib.wfst_reweight(None, None, None, 3, 0, C.byref(out)))
    assert "reweight_type" in ko_message(wfst_lib.wfst_push_weights(None, None, 7, None, C.byref(out)))
    bad = _lib.PushWeightsConfig(-1.0, 0)
    assert "delta" in ko_message(wfst_lib.wfst_push_weights(None, None, 0, C.byref(bad), C.byref(out)))
    for d in (-1e-3, float("nan"), float("inf")):
        cfg = _lib.ShortestDistanceConfig(1, d)
        assert "delta" in ko_message(wfst_lib.wfst_shortest_distance_with_config(None, None, C.byref(cfg), None, None))
    assert out.value is None
    # valid arguments, no handles: the usual null-pointer KO, nothing dereferenced
    assert "null" in ko_message(wfst_lib.wfst_reweight(None, None, None, 0, 1, C.byref(out)))


def test_python_surface():
    import rustfst_amd
    sig = inspect.signature(rustfst_amd.DeviceFst.shortest_distance)
    params = list(sig.parameters.values())
    assert params[1].name == "want_hops" and params[1].default is False  # the old positional signature
    assert sig.parameters["reverse"].default is False and sig.parameters["delta"].default is None
    assert rustfst_amd.ReweightType.REWEIGHT_TO_INITIAL.value == 0 and rustfst_amd.ReweightType.REWEIGHT_TO_FINAL.value == 1
    cfg = rustfst_amd.PushWeightsConfig()
    assert cfg.delta == 1.0 / 1024.0 and cfg.remove_total_weight is False
    for name in ("shortest_distance", "reweight", "push_weights", "push_weights_with_config"):
        assert callable(getattr(rustfst_amd, name))
    with pytest.raises(ValueError):
        rustfst_amd.DeviceFst.shortest_distance(None, want_hops=True, reverse=True)


def _golden_run_ref(c):
    flat = k14_flat(c)
    to_final = c["reweight_type"] == 1
    if c["op"] == "reweight":
        return to_flat(reweight_ref(flat, c["potentials"], to_final))
    return to_flat(push_ref(flat, c["distance"], to_final, c["remove_total_weight"]))


def test_k14_restatement_reproduces_the_derivations():
    """the hand derivations of K14_DERIVATION.md, replayed by this file's restatement (checks the restatement itself)"""
    cases = golden_cases()
    assert 6 <= len(cases) <= 8
    for c in cases:
        assert_same(_golden_run_ref(c), golden_expected(c), c["name"])


# ================================================================ GPU
def _dev_flat(d):
    return d.to_flat()


@pytest.mark.gpu
def test_k14_on_the_device(gpu_ctx):
    import rustfst_amd
    for c in golden_cases():
        dev = to_device(k14_flat(c), gpu_ctx)
        rt = rustfst_amd.ReweightType(c["reweight_type"])
        if c["op"] == "reweight":
            got = dev.reweight(np.array(c["potentials"], dtype=np.float32), rt)
        else:
            got = dev.push_weights(rt, rustfst_amd.PushWeightsConfig(remove_total_weight=c["remove_total_weight"]))
        assert_same(got.to_flat(), golden_expected(c), c["name"])


SHAPES = [(1, 2, 4), (2, 1, 3), (5, 3, 4), (17, 3, 6), (40, 4, 8), (120, 5, 16), (300, 2, 32), (1000, 6, 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_reverse_distances_match_the_oracle(gpu_ctx, oracle, shape):
    n, fan, sigma = shape
    for seed in range(4):
        rng = np.random.default_rng(1000 * n + seed)
        flat = random_fst_flat(rng, n, fan, sigma, p_final=0.25)
        exp = to_oracle(oracle, flat).reverse().shortest_distance()[1:]
        dev = to_device(flat, gpu_ctx)
        got, ln = dev.shortest_distance_with_len(reverse=True)
        np.testing.assert_array_equal(got.view(np.uint32), exp.view(np.uint32), err_msg=f"{shape} seed {seed}")
        assert ln == reverse_len_rule(flat), f"{shape} seed {seed}"
        assert np.all(np.isinf(got[ln:]))
        # forward: unchanged, and its length is 1 + the largest reachable id
        fwd, fl = dev.shortest_distance_with_len()
        np.testing.assert_array_equal(fwd.view(np.uint32), dev.shortest_distance().view(np.uint32))
        off, nxt = csr_next(flat)
        assert fl == int(np.nonzero(reach(n, off, nxt, [0]))[0].max()) + 1


@pytest.mark.gpu
def test_reverse_distances_transducer_and_no_start(gpu_ctx, oracle):
    t = synth.make_transducer(100_000)
    exp = to_oracle(oracle, t).reverse().shortest_distance()[1:]
    dev = to_device(t, gpu_ctx)
    got, ln = dev.shortest_distance_with_len(reverse=True)
    np.testing.assert_array_equal(got.view(np.uint32), exp.view(np.uint32))
    assert ln == reverse_len_rule(t)
    again = dev.shortest_distance(reverse=True)  # the cached reversed handle
    np.testing.assert_array_equal(again.view(np.uint32), got.view(np.uint32))
    # no start state: reverse distances are still defined
    rng = np.random.default_rng(5)
    flat = random_fst_flat(rng, 30, 3, 5)
    flat["start"] = None
    got, ln = to_device(flat, gpu_ctx).shortest_distance_with_len(reverse=True)
    exp = to_oracle(oracle, flat).reverse().shortest_distance()[1:]
    np.testing.assert_array_equal(got.view(np.uint32), exp.view(np.uint32))
    assert ln == reverse_len_rule(flat)


def _random_potentials(rng, n):
    k = int(rng.integers(0, n + 3))
    pot = rng.integers(-2000, 2000, k).astype(np.float32) / 256
    pot[rng.random(k) < 0.2] = np.inf
    if k and rng.random() < 0.5:
        pot[0] = rng.choice([0.0, 1.0 / 2048, -1.0 / 2048, 3.0])  # start potential: one, approximately one, or not
    return pot


@pytest.mark.gpu
def test_reweight_matches_the_restatement(gpu_ctx):
    import rustfst_amd
    for seed in range(48):
        rng = np.random.default_rng(7000 + seed)
        n = int(rng.integers(1, 40))
        flat = random_fst_flat(rng, n, 4, 6, p_eps_i=0.2, p_eps_o=0.2, acyclic=bool(seed % 3 == 0))
        flat["props"] |= [0, INITIAL_ACYCLIC, INITIAL_CYCLIC, ACYCLIC | INITIAL_ACYCLIC][seed % 4]
        pot = _random_potentials(rng, n)
        dev = to_device(flat, gpu_ctx)
        for rt in (0, 1):
            got = dev.reweight(pot, rustfst_amd.ReweightType(rt)).to_flat()
            exp = to_flat(reweight_ref(flat, list(pot), rt == 1))
            assert_same(got, exp, f"seed {seed} type {rt}")


@pytest.mark.gpu
@pytest.mark.parametrize("remove", [False, True])
def test_push_weights_matches_the_restatement(gpu_ctx, oracle, remove):
    import rustfst_amd
    cfg = rustfst_amd.PushWeightsConfig(remove_total_weight=remove)
    for seed in range(24):
        rng = np.random.default_rng(9000 + seed)
        n = int(rng.integers(1, 60))
        flat = random_fst_flat(rng, n, 4, 8, p_eps_i=0.1, acyclic=bool(seed % 2))
        dev = to_device(flat, gpu_ctx)
        for rt in (0, 1):
            got = dev.push_weights(rustfst_amd.ReweightType(rt), cfg).to_flat()
            exp = to_flat(push_ref(flat, _oracle_dist(oracle, flat, rt == 1), rt == 1, remove))
            assert_same(got, exp, f"seed {seed} type {rt} remove {remove}")


@pytest.mark.gpu
def test_push_invariants(gpu_ctx, oracle):
    import rustfst_amd
    for seed in range(12):
        rng = np.random.default_rng(300 + seed)
        flat = random_fst_flat(rng, 80, 4, 8, acyclic=bool(seed % 2))
        dev = to_device(flat, gpu_ctx)
        best = oracle.OracleFst.shortest_path(to_oracle(oracle, flat)).total_weight
        pushed = dev.push_weights(rustfst_amd.ReweightType.REWEIGHT_TO_INITIAL).to_flat()
        # every coaccessible state but the start: min(out-arc weights, final weight) is exactly 0
        n = flat["n_states"]
        off, nxt = csr_next(flat)
        roff, rsrc = transpose(n, off, nxt)
        fin = np.nonzero(np.isfinite(flat["finals"]))[0]
        coacc = reach(n, roff, rsrc, fin) if fin.size else np.zeros(n, dtype=bool)
        po, pa, pf = pushed["offsets"], pushed["arcs"], pushed["finals"]
        for s in np.nonzero(coacc)[0]:
            if s == pushed["start"] or s == flat["start"]:
                continue
            ws = list(pa["weight"][po[s]:po[s + 1]]) + [pf[s]]
            assert min(ws) == 0.0, f"seed {seed} state {s}: {ws}"
        # the best path's weight: unchanged, and 0 once the total weight is removed
        got = to_oracle(oracle, pushed).shortest_path().total_weight
        assert got == pytest.approx(best, abs=1e-3) or (np.isinf(got) and np.isinf(best))
        removed = dev.push_weights(rustfst_amd.ReweightType.REWEIGHT_TO_INITIAL,
                                   rustfst_amd.PushWeightsConfig(remove_total_weight=True)).to_flat()
        got = to_oracle(oracle, removed).shortest_path().total_weight
        if np.isfinite(best):
            assert abs(got) <= 1e-3, f"seed {seed}: {got}"
        fin_pushed = dev.push_weights(rustfst_amd.ReweightType.REWEIGHT_TO_FINAL,
                                      rustfst_amd.PushWeightsConfig(remove_total_weight=True)).to_flat()
        got = to_oracle(oracle, fin_pushed).shortest_path().total_weight
        if np.isfinite(best):
            assert abs(got) <= 1e-3, f"seed {seed} to final: {got}"


@pytest.mark.gpu
def test_compose_with_pushed_transducer(gpu_ctx):
    import rustfst_amd
    t = synth.make_transducer(2000, 8, 32, 0.0, seed=11)
    accs = synth.make_acceptors(t, 6, 12, seed0=77)
    dt = to_device(t, gpu_ctx)
    total = float(dt.shortest_distance(reverse=True)[0])
    for remove in (False, True):
        pt = dt.push_weights(rustfst_amd.ReweightType.REWEIGHT_TO_INITIAL,
                             rustfst_amd.PushWeightsConfig(remove_total_weight=remove))
        pt.tr_sort(True)  # (reweight keeps the arc order; the sort only restores the word's sortedness bit)
        for a in accs:
            da = to_device(a, gpu_ctx)
            p0 = da.compose(dt).shortest_path().to_flat()
            p1 = da.compose(pt).shortest_path().to_flat()

            def weight(p):
                if p["n_states"] == 0:
                    return np.inf
                return float(np.sum(p["arcs"]["weight"], dtype=np.float64) + np.sum(p["finals"][np.isfinite(p["finals"])]))
            w0, w1 = weight(p0), weight(p1)
            if np.isinf(w0):
                assert np.isinf(w1)
                continue
            assert w1 == pytest.approx(w0 - (total if remove else 0.0), abs=1e-2)


@pytest.mark.gpu
def test_start_state_cyclicity(gpu_ctx):
    """the start branch on FSTs whose word does not know INITIAL_ACYCLIC: both outcomes, the DFS bits in the word"""
    import rustfst_amd
    arcs = lambda rows: np.array(rows, dtype=TR_DTYPE)  # noqa: E731
    # 0 -> 1 -> 2 (final), 1 -> 0: the start on a cycle
    cyc = dict(n_states=3, start=0, offsets=np.array([0, 1, 3, 3], dtype=np.uint32),
               arcs=arcs([(1, 1, 1.0, 1), (2, 2, 0.5, 2), (3, 3, 2.0, 0)]),
               finals=np.array([np.inf, np.inf, 0.25], dtype=np.float32), props=0)
    # start 0 without arcs (final), 1 -> 2 (final) -> 1 unreachable from it
    acy = dict(n_states=3, start=0, offsets=np.array([0, 0, 1, 2], dtype=np.uint32),
               arcs=arcs([(2, 2, 0.5, 2), (3, 3, 2.0, 1)]),
               finals=np.array([0.75, np.inf, 0.25], dtype=np.float32), props=0)
    for flat, facts in ((cyc, (True, True, True, True)), (acy, (False, True, True, False))):
        assert graph_facts(flat) == facts
        dev = to_device(flat, gpu_ctx)
        for rt in (0, 1):
            pot = np.array([2.5, 1.0, 0.5][:flat["n_states"]], dtype=np.float32)
            got = dev.reweight(pot, rustfst_amd.ReweightType(rt)).to_flat()
            assert_same(got, to_flat(reweight_ref(flat, list(pot), rt == 1)), f"facts {facts} type {rt}")
            p = got["props"]
            assert bool(p & CYCLIC) and not p & ACYCLIC  # merged by the DFS, kept by every later step
            if facts[3]:  # a new start state; add_state drops ACCESSIBLE, set_start both INITIAL bits
                assert got["n_states"] == flat["n_states"] + 1 and got["start"] == flat["n_states"]
                assert not p & (INITIAL_CYCLIC | INITIAL_ACYCLIC | NOT_ACCESSIBLE)
            else:  # the start reweighted in place (no arcs: only set_final's mask)
                assert got["n_states"] == flat["n_states"] and got["start"] == 0
                assert p & INITIAL_ACYCLIC and not p & INITIAL_CYCLIC
                assert p & NOT_ACCESSIBLE and not p & ACCESSIBLE


@pytest.mark.gpu
def test_source_handle_unchanged(gpu_ctx):
    import rustfst_amd
    t = synth.make_transducer(5000, 6, 32, 0.0, seed=4)
    dev = to_device(t, gpu_ctx)
    before = dev.to_flat()
    sp0 = dev.shortest_path().to_flat()
    for rt in (0, 1):
        for remove in (False, True):
            dev.push_weights(rustfst_amd.ReweightType(rt), rustfst_amd.PushWeightsConfig(remove_total_weight=remove))
    dev.reweight(np.arange(5000, dtype=np.float32) / 64, rustfst_amd.ReweightType.REWEIGHT_TO_FINAL)
    after = dev.to_flat()
    assert_same(after, before, "source after push")
    sp1 = dev.shortest_path().to_flat()
    assert_same(sp1, sp0, "shortest_path on the source")


def _push_to_initial_numpy(flat, dist, facts):
    """the restatement for ToInitial with the Vec as long as the FST (past the end = +inf: the same thing for reweight),
    vectorised: the arc loop of reweight.rs:55-86 is one independent update per arc"""
    n = flat["n_states"]
    d = np.asarray(dist, dtype=np.float32)
    off = flat["offsets"].astype(np.int64)
    arcs = flat["arcs"].copy()
    src = np.repeat(np.arange(n), np.diff(off))
    d_s, d_n, w = d[src], d[arcs["nextstate"]], arcs["weight"]
    keep = np.isinf(d_s) | np.isinf(d_n)
    with np.errstate(invalid="ignore"):
        wt = np.where(np.isinf(w), w, (w + d_n).astype(np.float32))
        neww = (wt - d_s).astype(np.float32)
    arcs["weight"] = np.where(keep, w, neww)
    fin = flat["finals"].copy()
    sel = np.isfinite(fin) & np.isfinite(d)
    fin[sel] = (fin[sel] - d[sel]).astype(np.float32)
    out = dict(flat, arcs=arcs, finals=fin)
    # the word through the same steps as reweight_ref; the start branch needs only d[start], the word and the DFS facts
    p = int(flat["props"])
    if len(arcs):
        p &= ARC_RELEVANT
    if sel.any():
        p = p_set_final(p, None, None)
    s0, ds0 = flat["start"], d[flat["start"]]
    if not is_one(ds0) and not is_zero(ds0):
        if not (p & (INITIAL_CYCLIC | INITIAL_ACYCLIC)):
            p = (p & ~DFS_BITS) | dfs_bits(facts)
        assert not p & INITIAL_ACYCLIC  # (T: arc 0 of every state runs round a ring)
        p = p_set_start(p_add_tr(p_add_state(p), n, (0, 0, ds0, s0)))
        out["n_states"], out["start"] = n + 1, n
        out["offsets"] = np.r_[flat["offsets"], flat["offsets"][-1] + 1].astype(np.uint32)
        out["arcs"] = np.r_[arcs, np.array([(0, 0, ds0, s0)], dtype=TR_DTYPE)]
        out["finals"] = np.r_[fin, np.float32(np.inf)].astype(np.float32)
    out["props"] = p & WEIGHT_INVARIANT & ~COACCESSIBLE & ALL
    return out


@pytest.mark.gpu
def test_push_large_transducer(gpu_ctx, oracle):
    """T of 1M states / 10M arcs: push (ToInitial) and shortest_path, all on the device, against the vectorised
    restatement over the oracle's reverse distances"""
    import rustfst_amd
    t = synth.make_transducer(1_000_000)
    dev = to_device(t, gpu_ctx)
    pushed = dev.push_weights(rustfst_amd.ReweightType.REWEIGHT_TO_INITIAL)
    sp = pushed.shortest_path().to_flat()
    got = pushed.to_flat()
    dist = to_oracle(oracle, t).reverse().shortest_distance()[1:]
    exp = _push_to_initial_numpy(t, dist, graph_facts(t))
    assert_same(got, exp, "T 1M")
    assert sp["n_states"] > 0
    # the best path costs what it cost before the push
    sp0 = dev.shortest_path().to_flat()
    w = lambda p: float(np.sum(p["arcs"]["weight"], dtype=np.float64) + p["finals"][np.isfinite(p["finals"])].sum())  # noqa: E731
    assert w(sp) == pytest.approx(w(sp0), abs=1e-2)
