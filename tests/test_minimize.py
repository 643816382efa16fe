"""minimize / minimize_with_config of input-deterministic acyclic acceptors (wfst_minimize): the C-ABI surface without a
GPU, a literal sequential Python restatement of rustfst's minimize_with_config (AcyclicMinimizer branch;
oracle/model/minimize.py) checked against the hand-derived K16 known answers, the survivor rule checked against it, and on the device
parity with the restatement in every regime, closed-form answers at scale, invariants and error handling.

Bound on weights (used by the invariants): push_weights(ToInitial) replaces w by (w + d[t]) - d[s]; along a path these
telescope, so in exact arithmetic the weight of every string is unchanged.  Each of the two f32 operations rounds by at
most 2^-24 relative to a magnitude of at most 2 W (W = the largest |distance| or |weight| met), QuantizeMapper moves a
value by at most delta / 2 and its own division, floor and product round by at most 3 * 2^-24 relative.  A string with
L arcs and one final weight therefore moves by at most
    weight_bound(L, W, delta) = (L + 1) * (delta / 2 + 8 * 2^-24 * max(1, 2 W))."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from rustfst_amd._lib import TR_DTYPE

from oracle import model
from oracle.model import (ACCEPTOR, ACCESSIBLE, ACYCLIC, COACCESSIBLE, CYCLIC, EPSILONS, F32, INF, INITIAL_ACYCLIC,
                          I_DETERMINISTIC, I_EPSILONS, I_LABEL_SORTED, KSHORTESTDELTA, MSG_NONDET, NOT_ACCEPTOR,
                          NOT_I_DETERMINISTIC, NOT_I_LABEL_SORTED, NOT_O_LABEL_SORTED, NOT_TOP_SORTED, NO_EPSILONS,
                          NO_I_EPSILONS, NO_O_EPSILONS, O_DETERMINISTIC, O_EPSILONS, O_LABEL_SORTED, TOP_SORTED,
                          UNWEIGHTED, Unsupported, WEIGHTED, acyclic_partition, connect, flat_to_fst, fst_depth,
                          make_flat, minimize_ref)
from helpers import ROOT, assert_flat_identical, golden_flat, ko_message, to_device
from minimize_cases import (accepts, assert_idempotent, blow_up, cfg_of, check_invariants, closed_form_base,
                            far_apart_cases, golden_cases, no_start_cases, random_cases, random_dag, trie_flat)

PATHS = ("narrow", "wide", "auto")


# ================================================================ CPU
def test_symbol_declared_and_bound(wfst_lib):
    from rustfst_amd import _lib
    with open(os.path.join(ROOT, "include", "wfst.h")) as f:
        header = f.read()
    assert re.search(r"\bwfst_status\s+wfst_minimize\s*\(", header)
    assert "wfst_minimize" in {name for name, _, _ in _lib.SYMBOLS}
    assert hasattr(wfst_lib, "wfst_minimize")
    assert re.search(r"#define\s+WFST_ABI_VERSION\s+7\b", header)
    assert C.sizeof(_lib.MinimizeConfig) == 8
    assert _lib.MinimizeConfig.delta.offset == 0 and _lib.MinimizeConfig.allow_nondet.offset == 4


def test_argument_validation_without_gpu(wfst_lib):
    from rustfst_amd import _lib
    out = C.c_void_p(1)
    for d in (0.0, -1e-3, float("nan"), float("inf")):
        cfg = _lib.MinimizeConfig(d, 0)
        assert "delta" in ko_message(wfst_lib.wfst_minimize(None, None, C.byref(cfg), C.byref(out)))
        assert out.value is None
    assert "null" in ko_message(wfst_lib.wfst_minimize(None, None, None, C.byref(out)))
    good = _lib.MinimizeConfig(1e-6, 1)
    assert "null" in ko_message(wfst_lib.wfst_minimize(None, None, C.byref(good), None))


def test_python_surface():
    import rustfst_amd
    cfg = rustfst_amd.MinimizeConfig()
    assert cfg.delta == 1e-6 and cfg.allow_nondet is False
    cfg = rustfst_amd.MinimizeConfig(delta=0.5, allow_nondet=True)
    assert cfg.delta == 0.5 and cfg.allow_nondet is True
    assert rustfst_amd.KSHORTESTDELTA == 1e-6
    for name in ("minimize", "minimize_with_config", "MinimizeConfig"):
        assert name in rustfst_amd.__all__ and callable(getattr(rustfst_amd, name))
    assert inspect.signature(rustfst_amd.DeviceFst.minimize).parameters["config"].default is None
    assert inspect.signature(rustfst_amd.VectorFst.minimize).parameters["config"].default is None


def test_k16_restatement_reproduces_the_derivations():
    """the hand derivations of K16_DERIVATION.md, replayed by this file's restatement (checks the restatement itself)"""
    cases = golden_cases()
    assert len(cases) >= 8
    for c in cases:
        delta, nondet = cfg_of(c)
        got = minimize_ref(golden_flat(c), delta, nondet)
        assert_flat_identical(got, golden_flat(c, "expected"), c["name"])
        for labels, weight in c.get("accepts", []):
            for f in (golden_flat(c), got):
                w = accepts(f, labels)
                assert (w is None) == (weight is None), (c["name"], labels)
                if w is not None:
                    assert abs(w - weight) <= 1e-5, (c["name"], labels, w)


def survivors_by_rule(fst):
    """the closed rule: at every height the class holding the height's highest state id keeps its highest id, every other
    class its lowest — on the connected, label-sorted FST acyclic_partition sees; returns {state: survivor}"""
    heights = fst_depth(fst)
    cls = [None] * len(heights)
    for h in range(max(heights) + 1):
        members = [s for s in range(len(heights)) if heights[s] == h]
        groups = {}
        for s in members:
            f = fst["finals"][s]
            k = (float(INF if f is None else f), len(fst["rows"][s]), tuple((tr[0], cls[tr[3]]) for tr in fst["rows"][s]))
            groups.setdefault(k, []).append(s)
        top = max(members)
        for g in groups.values():
            keep = max(g) if top in g else min(g)
            for s in g:
                cls[s] = keep
    return cls


def test_survivor_rule_against_the_partition_lists():
    rng = np.random.default_rng(16)
    several = 0
    for i in range(300):
        flat = trie_flat(rng, int(rng.integers(5, 50)), 3, 5, False) if i % 2 else random_dag(rng, int(rng.integers(2, 50)), 3, False)
        fst = flat_to_fst(flat)
        connect(fst)
        if not fst["rows"]:
            continue
        for row in fst["rows"]:
            row.sort(key=lambda t: t[0])
        part = acyclic_partition(fst)
        rule = survivors_by_rule(fst)
        for c in range(len(part.head)):
            mem = list(part.members(c))
            several += len(mem) > 1
            for s in mem:
                assert rule[s] == mem[0], (i, c, mem, rule[s])
    assert several > 300


def test_generator_shrinks_and_restatement_is_idempotent():
    cases = random_cases(7, 80)
    shrunk = reordered = 0
    for name, flat in cases:
        got = minimize_ref(flat)
        trimmed = flat_to_fst(flat)
        connect(trimmed)
        shrunk += got["n_states"] < len(trimmed["rows"])
        again = minimize_ref(got)
        assert_idempotent(again, got, name + " idempotent")
        reordered += not np.array_equal(again["arcs"]["ilabel"], got["arcs"]["ilabel"])
    assert 2 * shrunk >= len(cases), shrunk
    assert reordered > 0  # (the case assert_idempotent describes does occur)


def test_restatement_errors():
    nd = make_flat(2, 0, [[(1, 1, 0.0, 1), (1, 1, 0.0, 1)], []], [INF, 0.0])
    with pytest.raises(Unsupported, match="Refusing"):
        minimize_ref(nd)
    with pytest.raises(Unsupported, match="non-deterministic inputs"):
        minimize_ref(nd, allow_nondet=True)
    with pytest.raises(Unsupported, match="transducers"):
        minimize_ref(make_flat(2, 0, [[(1, 2, 0.0, 1)], []], [INF, 0.0]))
    with pytest.raises(Unsupported, match="cyclic"):
        minimize_ref(make_flat(2, 0, [[(1, 1, 0.0, 1)], [(1, 1, 0.0, 0)]], [INF, 0.0]))


def test_restatement_without_a_start_state():
    for flat, message in no_start_cases():
        if message is None:
            got = minimize_ref(flat)
            assert got["n_states"] == 0 and got["start"] is None and len(got["arcs"]) == 0
            assert got["props"] & (ACCESSIBLE | COACCESSIBLE | ACCEPTOR | UNWEIGHTED) == ACCESSIBLE | COACCESSIBLE | ACCEPTOR | UNWEIGHTED
        else:
            with pytest.raises(Unsupported, match=message):
                minimize_ref(flat)
    # the stored determinism bits: set_weight_unchecked on the one reweighted arc drops them, the recomputation does not
    # ask for them again
    assert not minimize_ref(no_start_cases()[1][0])["props"] & (I_DETERMINISTIC | O_DETERMINISTIC)


def test_restatement_keeps_both_arcs_when_merged_weights_are_far_apart():
    """what the reference does where the device answers KO: merge_states appends the member's arc, tr_unique's approximate
    == does not drop it, and the survivor ends with two arcs of one label"""
    for flat in far_apart_cases():
        got = minimize_ref(flat)
        assert got["n_states"] == 3
        seg = got["arcs"][got["offsets"][1]:got["offsets"][2]]
        assert seg["ilabel"].tolist() == [3, 3] and seg["nextstate"].tolist() == [2, 2]
        assert sorted(seg["weight"].tolist()) == sorted(F32(flat["arcs"]["weight"][2:4]).tolist())


# ================================================================ GPU
def dev_minimize(flat, ctx, delta=None, allow_nondet=False):
    import rustfst_amd
    cfg = None if delta is None and not allow_nondet else rustfst_amd.MinimizeConfig(delta, allow_nondet)
    return to_device(flat, ctx).minimize(cfg)


@pytest.mark.gpu
def test_k16_on_the_device(gpu_ctx, monkeypatch):
    for path in PATHS:
        monkeypatch.setenv("WFST_MINIMIZE_PATH", path)
        for c in golden_cases():
            delta, nondet = cfg_of(c)
            got_dev = dev_minimize(golden_flat(c), gpu_ctx, delta, nondet)
            assert_flat_identical(got_dev.to_flat(), golden_flat(c, "expected"), f"{c['name']} [{path}]")
            check_invariants(golden_flat(c), got_dev, delta, gpu_ctx, np.random.default_rng(1), c["name"])


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
def test_random_acceptors_match_the_restatement(gpu_ctx, monkeypatch, path):
    monkeypatch.setenv("WFST_MINIMIZE_PATH", path)
    rng = np.random.default_rng(3)
    cases = random_cases(11, 60)
    shrunk = 0
    for name, flat in cases:
        dev = to_device(flat, gpu_ctx)
        before = dev.to_flat()
        got_dev = dev.minimize()
        got = got_dev.to_flat()
        exp = minimize_ref(flat)
        assert_flat_identical(got, exp, f"{name} [{path}]")
        assert_flat_identical(dev.to_flat(), before, "source handle")
        trimmed = flat_to_fst(flat)
        connect(trimmed)
        shrunk += got["n_states"] < len(trimmed["rows"])
        check_invariants(flat, got_dev, KSHORTESTDELTA, gpu_ctx, rng, name)
    assert 2 * shrunk >= len(cases), shrunk


@pytest.mark.gpu
def test_determinized_lattices(gpu_ctx):
    """determinize -> minimize -> compose on handles, no download in between; the minimized lattice equals the restatement"""
    from helpers import random_fst_flat
    import rustfst_amd
    rng = np.random.default_rng(21)
    shrunk = 0
    for i in range(12):
        lat = random_fst_flat(rng, int(rng.integers(8, 40)), 3, 3, acyclic=True, weight_grid=1, max_w=3)
        lat["arcs"]["olabel"] = lat["arcs"]["ilabel"]
        lat["props"] = ACCEPTOR | ACYCLIC | INITIAL_ACYCLIC
        lat["finals"][-1] = 0.0
        det = to_device(lat, gpu_ctx).determinize()
        mini = det.minimize()
        det_flat, got = det.to_flat(), mini.to_flat()
        assert_flat_identical(got, minimize_ref(det_flat), f"lattice {i}")
        shrunk += got["n_states"] < det_flat["n_states"]
        check_invariants(det_flat, mini, KSHORTESTDELTA, gpu_ctx, rng, f"lattice {i}")
        if got["n_states"]:
            # (the weighted result's arcs are in first-occurrence order and its word says nothing about label order:
            # compose wants sorted labels, as in the reference; tr_sort works on the handle)
            comp = mini.tr_sort().compose(mini)
            assert comp.to_flat()["n_states"] >= got["n_states"]
    assert shrunk >= 3


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
def test_fan_out_above_64(gpu_ctx, monkeypatch, path):
    """two hub states with 200 arcs each that merge (a wave per state), next to one that differs in a single target"""
    monkeypatch.setenv("WFST_MINIMIZE_PATH", path)
    rng = np.random.default_rng(5)
    labs = rng.permutation(np.arange(1, 201))
    # states: 0 start -> 1, 2, 3 (hubs) -> 4..9 (leaves: 4, 5 final 0; 6, 7 final 1; 8, 9 one arc to 4 / 5)
    rows = [[(1, 1, 0.0, 1), (2, 2, 0.0, 2), (3, 3, 0.0, 3)], [], [], [], [], [], [], [], [(7, 7, 1.0, 4)], [(7, 7, 1.0, 5)]]
    for k, lab in enumerate(labs):
        t = (4, 6, 8)[k % 3]
        rows[1].append((int(lab), int(lab), float(k % 2), t))
        rows[2].append((int(lab), int(lab), float(k % 2), t + 1))
        rows[3].append((int(lab), int(lab), float(k % 2), t + 1 if k != 150 else 4 + (k + 1) % 3 * 2))
    finals = [INF, INF, INF, INF, 0.0, 0.0, 1.0, 1.0, INF, INF]
    for props in (ACCEPTOR, 0):
        flat = make_flat(10, 0, rows, finals, props)
        got_dev = dev_minimize(flat, gpu_ctx)
        got = got_dev.to_flat()
        assert_flat_identical(got, minimize_ref(flat), f"fan-out [{path}]")
        check_invariants(flat, got_dev, KSHORTESTDELTA, gpu_ctx, rng, f"fan-out [{path}]")
        nxt = got["arcs"]["nextstate"][:3]  # the start's three arcs: hubs 1 and 2 are one state, hub 3 another
        assert nxt[0] == nxt[1] != nxt[2] and got["n_states"] < 10
    unweighted = make_flat(10, 0, [[(a[0], a[1], 0.0, a[3]) for a in r] for r in rows], [INF] * 4 + [0.0] * 4 + [INF] * 2)
    got_dev = dev_minimize(unweighted, gpu_ctx)
    assert_flat_identical(got_dev.to_flat(), minimize_ref(unweighted), f"fan-out unweighted [{path}]")
    check_invariants(unweighted, got_dev, KSHORTESTDELTA, gpu_ctx, rng, f"fan-out unweighted [{path}]")


@pytest.mark.gpu
@pytest.mark.parametrize("delta", [1e-6, 1.0 / 1024.0])
def test_real_valued_weights(gpu_ctx, delta):
    rng = np.random.default_rng(9)
    for i in range(10):
        flat = random_dag(rng, int(rng.integers(5, 80)), 4, True, real=True)
        got_dev = dev_minimize(flat, gpu_ctx, delta)
        assert_flat_identical(got_dev.to_flat(), minimize_ref(flat, delta), f"real {i} delta {delta}")
        # (idempotent=False: the second push computes (w - d) + d at the start state, which need not round back to w on
        # real-valued weights; the second call is still compared bit for bit with the restatement of that call)
        check_invariants(flat, got_dev, delta, gpu_ctx, rng, f"real {i}", idempotent=False)


def test_closed_form_on_the_restatement():
    """the closed form of the scale test, checked on the CPU at k = 3 and k = 7 with the restatement itself"""
    rng = np.random.default_rng(33)
    m = closed_form_base(rng)
    exp = minimize_ref(m)
    assert exp["n_states"] == m["n_states"] and np.array_equal(exp["arcs"], m["arcs"])
    for k in (3, 7):
        assert_flat_identical(minimize_ref(blow_up(rng, m, k)), exp, f"k = {k}")


@pytest.mark.gpu
def test_scale_closed_form(gpu_ctx):
    rng = np.random.default_rng(33)
    m = closed_form_base(rng)
    for k in (3, (1 << 20) // m["n_states"] + 1):
        big = blow_up(rng, m, int(k))
        got_dev = dev_minimize(big, gpu_ctx)
        assert_flat_identical(got_dev.to_flat(), minimize_ref(m), f"k = {k}, {big['n_states']} states")
        check_invariants(big, got_dev, KSHORTESTDELTA, gpu_ctx, rng, f"k = {k}")
    assert big["n_states"] >= 1_000_000


@pytest.mark.gpu
def test_word_list(gpu_ctx):
    """200 k random words = random prefix + one of 300 suffixes: the suffixes are shared after minimization"""
    rng = np.random.default_rng(44)
    suffixes = [tuple(rng.integers(1, 6, size=int(rng.integers(3, 9))).tolist()) for _ in range(300)]
    words = set()
    while len(words) < 200_000:
        pre = rng.integers(1, 6, size=(20_000, 9))
        ln = rng.integers(6, 10, size=20_000)
        sx = rng.integers(0, 300, size=20_000)
        for p, l, x in zip(pre, ln, sx):
            words.add(tuple(p[:l].tolist()) + suffixes[x])
    words = sorted(words)
    # trie by sorted insertion (vectorised enough: a dict per depth)
    nxt, rows_src, rows_lab, rows_dst, final = {}, [], [], [], set()
    n = 1
    for w in words:
        s = 0
        for lab in w:
            key = (s, lab)
            t = nxt.get(key)
            if t is None:
                t = n
                n += 1
                nxt[key] = t
                rows_src.append(s)
                rows_lab.append(lab)
                rows_dst.append(t)
            s = t
        final.add(s)
    src = np.array(rows_src)
    order = np.argsort(src, kind="stable")
    arcs = np.zeros(len(src), dtype=TR_DTYPE)
    arcs["ilabel"] = arcs["olabel"] = np.array(rows_lab)[order]
    arcs["nextstate"] = np.array(rows_dst)[order]
    off = np.zeros(n + 1, dtype=np.uint32)
    off[1:] = np.cumsum(np.bincount(src, minlength=n))
    finals = np.full(n, np.inf, dtype=np.float32)
    finals[list(final)] = 0.0
    flat = dict(n_states=n, start=0, offsets=off, arcs=arcs, finals=finals, props=ACCEPTOR)
    mini = dev_minimize(flat, gpu_ctx)
    got = mini.to_flat()
    assert got["n_states"] < n // 2
    acc, co, cyc, _ = model.graph_facts(got)
    assert acc and co and not cyc
    for w in [words[i] for i in rng.integers(0, len(words), size=300)]:
        assert accepts(got, w) == 0.0
    for _ in range(300):
        w = tuple(rng.integers(1, 6, size=int(rng.integers(1, 18))).tolist())
        assert (accepts(got, w) is None) == (accepts(flat, w) is None)
    check_invariants(flat, mini, KSHORTESTDELTA, gpu_ctx, rng, "word list")
    # the number of states of the minimal automaton is unique: the sequential restatement agrees on it
    if n <= 3_000_000:
        assert minimize_ref(flat)["n_states"] == got["n_states"]


@pytest.mark.gpu
def test_errors(gpu_ctx):
    import rustfst_amd
    from rustfst_amd import _lib

    def ko(flat, match, **kw):
        with pytest.raises(rustfst_amd.WfstError, match=match):
            dev_minimize(flat, gpu_ctx, **kw)
        # (WfstError carries wfst_last_error's text: _lib.check reads it, which also clears it)
        out = C.c_void_p()
        cfg = _lib.MinimizeConfig(kw.get("delta") or 1e-6, 1 if kw.get("allow_nondet") else 0)
        src = to_device(flat, gpu_ctx)
        assert _lib.lib().wfst_minimize(gpu_ctx._h, src._h, C.byref(cfg), C.byref(out)) == 1 and out.value is None
        assert re.search(match, ko_message(1))

    nd = make_flat(3, 0, [[(1, 1, 0.0, 1), (1, 1, 1.0, 2)], [], []], [INF, 0.0, 0.0])
    for props in (0, ACCEPTOR | NOT_I_DETERMINISTIC | WEIGHTED):
        nd["props"] = props
        ko(nd, MSG_NONDET)
        ko(nd, "non-deterministic inputs are not supported", allow_nondet=True)
    tr = make_flat(2, 0, [[(1, 2, 0.0, 1)], []], [INF, 0.0])
    for props in (0, NOT_ACCEPTOR | I_DETERMINISTIC | UNWEIGHTED):
        tr["props"] = props
        ko(tr, "transducers are not supported")
    cyc = make_flat(3, 0, [[(1, 1, 1.0, 1)], [(1, 1, 0.0, 2), (2, 2, 0.0, 0)], []], [INF, INF, 0.0])
    for props in (0, ACCEPTOR | I_DETERMINISTIC | WEIGHTED | CYCLIC, ACCEPTOR):
        cyc["props"] = props
        ko(cyc, "cyclic inputs are not supported")
    cyc["arcs"]["weight"] = 0.0
    cyc["props"] = 0
    ko(cyc, "cyclic inputs are not supported")
    # merged states whose arc weights tr_unique would not unite: the reference keeps both arcs, the device says so
    for flat in far_apart_cases():
        ko(flat, "arc weights further than 1/1024 apart")
    # a weighted input without a start state: the empty FST when pushing leaves no weight, else the reference's error
    for flat, message in no_start_cases():
        if message is None:
            got = dev_minimize(flat, gpu_ctx).to_flat()
            assert_flat_identical(got, minimize_ref(flat), "no start state")
            assert got["n_states"] == 0 and got["start"] is None
        else:
            ko(flat, message)
    # the context still works, and empty results are the empty FST
    dead = make_flat(3, 0, [[(1, 1, 1.0, 1)], [(1, 1, 2.0, 2)], []], [INF, INF, INF], ACCEPTOR)
    for f in (dead, make_flat(2, None, [[(1, 1, 0.0, 1)], []], [INF, 0.0], ACCEPTOR), make_flat(0, None, [], [], 0)):
        got = dev_minimize(f, gpu_ctx).to_flat()
        assert_flat_identical(got, minimize_ref(f), "empty")
        assert got["n_states"] == 0 and got["start"] is None


# ---------------------------------------------------------------- the facts of an arc, one at a time
# (fact bit, its pair in the property word when the fact is present / absent): fst_props.h FACT_* and add_trs_by_facts
FACT_PAIRS = ((1, NOT_ACCEPTOR, ACCEPTOR), (2, I_EPSILONS, NO_I_EPSILONS), (4, EPSILONS, NO_EPSILONS), (8, O_EPSILONS, NO_O_EPSILONS),
              (16, NOT_I_LABEL_SORTED, I_LABEL_SORTED), (32, NOT_O_LABEL_SORTED, O_LABEL_SORTED), (64, WEIGHTED, UNWEIGHTED),
              (128, NOT_TOP_SORTED, TOP_SORTED))
_KD_UP = float(np.nextafter(model.KDELTA, F32(1.0)))


def _fact_fst(rows, finals=(INF, INF, INF), start=2):
    return make_flat(3, start, rows, list(finals))


# name -> (the FST, the facts reverse() finds).  Three states, start 2, arcs running down (2 -> 1 -> 0) and no final state
# unless the fact needs one: reverse() then adds no super-initial arcs and turns every arc s -> t into (t + 1) -> (s + 1), which
# runs upwards, so the reversed FST's arcs carry exactly the facts listed (a fact that implies another, as eps:eps does,
# brings it along).  minimize() sees the same arcs from their own side, running downwards (always "nextstate <= state").
FACT_CASES = {
    "none": (_fact_fst([[], [(4, 4, 0.0, 0)], [(3, 3, 0.0, 1)]]), 0),
    "1_not_acceptor": (_fact_fst([[], [(4, 4, 0.0, 0)], [(3, 4, 0.0, 1)]]), 1),
    "2_ilabel_epsilon": (_fact_fst([[], [(4, 4, 0.0, 0)], [(0, 4, 0.0, 1)]]), 1 | 2),
    "4_epsilon": (_fact_fst([[], [(4, 4, 0.0, 0)], [(0, 0, 0.0, 1)]]), 2 | 4 | 8),
    "8_olabel_epsilon": (_fact_fst([[], [(4, 4, 0.0, 0)], [(3, 0, 0.0, 1)]]), 1 | 8),
    # two arcs of one state into one state: the pair is consecutive for minimize() and, reversed, for reverse()
    # (state 0's in-arcs, in reverse()'s order: the one from state 1, then these two)
    "16_ilabel_order": (_fact_fst([[], [(1, 1, 0.0, 0)], [(5, 3, 0.0, 0), (3, 4, 0.0, 0)]]), 1 | 16),
    "32_olabel_order": (_fact_fst([[], [(1, 1, 0.0, 0)], [(3, 5, 0.0, 0), (4, 3, 0.0, 0)]]), 1 | 32),
    # is_one is the approximate ==: a weight of exactly KDELTA is still one, the next f32 is a weight
    "64_weight_kdelta": (_fact_fst([[], [(4, 4, 0.0, 0)], [(3, 3, float(model.KDELTA), 1)]]), 0),
    "64_weight_above_kdelta": (_fact_fst([[], [(4, 4, 0.0, 0)], [(3, 3, _KD_UP, 1)]]), 64),
    "64_weighted": (_fact_fst([[], [(4, 4, 0.75, 0)], [(3, 3, 0.0, 1)]]), 64),
    # one arc running up, 0 -> 1: reversed it runs down
    "128_not_top_sorted": (_fact_fst([[(3, 3, 0.0, 1)], [], [(4, 4, 0.0, 1)]]), 128),
    # ... and all of them running up from start 0: minimize() finds no fact at all, reverse() finds both arcs running down
    "128_top_sorted_for_minimize": (_fact_fst([[(3, 3, 0.0, 1)], [(4, 4, 0.0, 2)], []], start=0), 128),
    # a final weight that is not one (minimize.hip's FACT_FINAL_WEIGHTED): reverse() turns it into the weight of the
    # super-initial state's eps:eps arc
    "256_final_weight": (_fact_fst([[], [(4, 4, 0.0, 0)], [(3, 3, 0.0, 1)]], finals=(F32(0.75), INF, INF)), 2 | 4 | 8 | 64),
    "256_final_weight_kdelta": (_fact_fst([[], [(4, 4, 0.0, 0)], [(3, 3, 0.0, 1)]], finals=(model.KDELTA, INF, INF)), 2 | 4 | 8),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FACT_CASES))
def test_each_arc_fact_reaches_the_property_word(gpu_ctx, oracle, name):
    """One tiny FST per fact of fst_props.h's arc_facts (and FACT_FINAL_WEIGHTED), uploaded with an EMPTY property word, so
    that reverse() (rev_facts_kernel and the host loop over the super-initial arcs) and minimize() (facts_kernel) have to
    find the fact in the content.  reverse(): FST and word are the oracle's, and the word holds, pair by pair, the negative
    bit of every listed fact and the positive bit of every other one.  minimize(): FST and word are the restatement's, or
    both refuse the input in the same words (a transducer)."""
    from helpers import to_oracle
    import rustfst_amd
    flat, rev_facts = FACT_CASES[name]
    assert flat["props"] == 0
    got = to_device(flat, gpu_ctx).reverse().to_flat()
    assert_flat_identical(got, to_oracle(oracle, flat).reverse().to_flat(), f"reverse {name}")
    for bit, present, absent in FACT_PAIRS:
        assert got["props"] & (present | absent) == (present if rev_facts & bit else absent), f"reverse {name}: fact {bit}"
    try:
        want = minimize_ref(flat)
    except Unsupported as e:
        with pytest.raises(rustfst_amd.WfstError, match=re.escape(e.args[0])):
            dev_minimize(flat, gpu_ctx)
    else:
        assert_flat_identical(dev_minimize(flat, gpu_ctx).to_flat(), want, f"minimize {name}")
