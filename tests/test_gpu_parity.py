"""GPU parity tests (run with -m gpu on an MI355X): every result of the HIP path, obtained through the
C-ABI, is compared with the CPU oracle on the same seeded inputs.

Bars: compose — bit-exact state ids, arc order, labels, weight bit patterns, finals, property word.
Shortest path — bit-exact against the oracle's canonical-tie mode on ALL inputs; against the
reference-order mode (KDELTA, AutoQueue) whenever the optimum is unique (the reference's own contract,
tests_openfst/algorithms/shortest_path.rs:69-92); total weight within 1e-5 always.
"""
import json
import os
import sys

import numpy as np
import pytest

import rustfst_amd
from rustfst_amd import ComposeConfig, ComposeFilter, ShortestPathConfig, Tr, VectorFst, synth
from helpers import FILTERS, assert_flat_identical, flat_matches_spec, random_fst_flat, to_device, to_oracle
from small_path_cases import predict_nbest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def vbuild(spec):
    f = VectorFst()
    for _ in range(spec["n_states"]):
        f.add_state()
    if spec.get("start") is not None:
        f.set_start(spec["start"])
    for s, il, ol, w, ns in spec["arcs"]:
        f.add_tr(s, Tr(il, ol, w, ns))
    for s, w in spec["finals"]:
        f.set_final(s, w)
    return f


def golden(name):
    with open(os.path.join(GOLDEN, name)) as fh:
        return json.load(fh)


# ------------------------------------------------------------------ the reference's own python tests, from their vectors
def vector_fst_from_golden(g):
    """a VectorFst built through the MutableFst calls the reference's tests use (add_state / set_start / set_final /
    add_tr), from a fixture {n_states, start, arcs [[state, ilabel, olabel, weight, nextstate] ...], finals [[state, w] ...]}"""
    f = VectorFst()
    for _ in range(g["n_states"]):
        f.add_state()
    if g["start"] is not None:
        f.set_start(g["start"])
    for s, w in g["finals"]:
        f.set_final(s, w)
    for s, il, ol, w, nxt in g["arcs"]:
        f.add_tr(s, Tr(il, ol, w, nxt))
    return f


def test_compose_fst(gpu_ctx):
    """K1: the vectors of rustfst-python/tests/algorithms/test_compose.py:13-81 (tests/golden/k1_compose.json)"""
    g = golden("k1_compose.json")
    fst1, fst2, expected_fst = (vector_fst_from_golden(g[k]) for k in ("fst1", "fst2", "expected"))
    assert fst1.compose(fst2) == expected_fst
    # explicit Sequence filter + connect (compose_with_config) gives the same machine
    assert fst1.compose(fst2, ComposeConfig(ComposeFilter.SEQUENCEFILTER, True)) == expected_fst


def test_compose_config(gpu_ctx):
    """rustfst-python/tests/algorithms/test_compose.py:84-154: the K1 pair under ComposeConfig(TRIVIALFILTER, connect=True)
    — the reference's stored vector for a non-default filter — gives the same expected machine."""
    g = golden("k1_compose.json")
    fst1, fst2, expected_fst = (vector_fst_from_golden(g[k]) for k in ("fst1", "fst2", "expected"))
    compose_config = ComposeConfig(ComposeFilter.TRIVIALFILTER, True)
    assert fst1.compose(fst2, compose_config) == expected_fst


def test_shortest_path(gpu_ctx):
    """K2: the vectors of rustfst-python/tests/algorithms/test_shortest_path.py:5-51 (tests/golden/k2_shortest_path.json)"""
    g = golden("k2_shortest_path.json")
    fst1, expected_fst = vector_fst_from_golden(g["fst"]), vector_fst_from_golden(g["expected"])
    assert fst1.shortest_path(ShortestPathConfig(1, True)) == expected_fst
    assert fst1.shortest_path() == expected_fst


def test_b3_vectors(gpu_ctx, oracle):
    g = golden("b3_fst_003_004.json")
    c3 = vbuild(g["fst_003"]).compose(vbuild(g["fst_003_compose"]))
    assert c3 == vbuild(g["fst_003_expected_compose"])
    assert c3.shortest_path() == vbuild(g["fst_003_expected_shortest_path"])
    c4 = vbuild(g["fst_004"]).compose(vbuild(g["fst_004_compose"]))  # MatchOutput-only branch
    assert c4 == vbuild(g["fst_004_expected_compose"])
    assert c4.shortest_path() == vbuild(g["fst_004_expected_shortest_path"])
    empty = vbuild(g["fst_003"]).compose(vbuild(g["fst_004"]))  # literal BASELINE config 1: empty FST
    assert empty.num_states() == 0 and empty.start() is None
    sp = empty.shortest_path()
    assert sp.num_states() == 0 and sp.start() is None


def test_error_behaviour(gpu_ctx):
    a = VectorFst()
    a.add_state()
    a.add_state()
    a.set_start(0)
    a.add_tr(0, Tr(1, 5, 0.0, 1))
    a.add_tr(0, Tr(1, 3, 0.0, 1))
    b = VectorFst()
    b.add_state()
    b.add_state()
    b.set_start(0)
    b.add_tr(0, Tr(7, 1, 0.0, 1))
    b.add_tr(0, Tr(2, 1, 0.0, 1))
    with pytest.raises(rustfst_amd.WfstError, match=r"sort\?"):  # compose_fst_op.rs:194
        a.compose(b)
    with pytest.raises(rustfst_amd.WfstError, match="expected acceptor"):  # determinize_fsa_op.rs:138-140
        b.shortest_path(ShortestPathConfig(nshortest=3, unique=True))
    one = rustfst_amd.acceptor([1])  # a single string: `unique` changes nothing
    assert one.shortest_path(ShortestPathConfig(nshortest=3, unique=True)).num_states() == one.shortest_path(ShortestPathConfig(nshortest=3)).num_states()
    assert rustfst_amd.acceptor([1]).shortest_path(ShortestPathConfig(nshortest=0)).num_states() == 0
    # invalid CSR is rejected at the boundary, not on the device
    with pytest.raises(rustfst_amd.WfstError, match="nextstate"):
        bad = synth.linear_acceptor_flat([1, 2])
        bad["arcs"]["nextstate"][1] = 99
        to_device(bad)


# ------------------------------------------------------------------ compose: bit-exact vs oracle
CASES = [
    # (n1, fan1, n2, fan2, sigma, p_eps_o(fst1), p_eps_i(fst2), sort1, sort2)
    (6, 3, 8, 4, 4, 0.0, 0.0, "olabel", "ilabel"),
    (10, 3, 12, 3, 3, 0.3, 0.3, "olabel", "ilabel"),     # epsilons on both sides: sequence filter states 0/1
    (12, 4, 9, 5, 5, 0.5, 0.1, "olabel", "ilabel"),
    (8, 2, 15, 6, 6, 0.2, 0.4, "olabel", "none"),        # only fst1 sorted -> MatchOutput
    (8, 5, 15, 3, 6, 0.2, 0.4, "none", "ilabel"),        # only fst2 sorted -> MatchInput
    (40, 3, 60, 8, 12, 0.1, 0.1, "olabel", "ilabel"),
    (5, 70, 7, 90, 40, 0.05, 0.05, "olabel", "ilabel"),  # fan-out > 64: binary-search path + multi-chunk items
    (30, 2, 30, 2, 2, 0.0, 0.0, "olabel", "ilabel"),     # dense label collisions, cyclic
]


@pytest.mark.parametrize("case", range(len(CASES)))
@pytest.mark.parametrize("connect", [True, False])
def test_compose_bit_exact_vs_oracle(gpu_ctx, oracle, case, connect):
    n1, f1, n2, f2, sigma, pe1, pe2, sort1, sort2 = CASES[case]
    for seed in range(4):
        rng = np.random.default_rng(1000 * case + seed)
        a = random_fst_flat(rng, n1, f1, sigma, p_eps_o=pe1, p_eps_i=0.1 if pe1 else 0.0, sort=sort1)
        b = random_fst_flat(rng, n2, f2, sigma, p_eps_i=pe2, p_eps_o=0.1 if pe2 else 0.0, sort=sort2)
        if sort1 == "none" and (a["props"] & synth.O_LABEL_SORTED):
            continue
        exp = to_oracle(oracle, a).compose(to_oracle(oracle, b), connect=connect).to_flat()
        got = to_device(a).compose(to_device(b), ComposeConfig(ComposeFilter.AUTOFILTER, connect)).to_flat()
        assert_flat_identical(got, exp, f"case {case} seed {seed} connect {connect}")


def test_compose_acceptor_with_synthetic_transducer(gpu_ctx, oracle):
    t = synth.make_transducer(3000, 6, 16, 0.05, seed=21)
    accs = synth.make_acceptors(t, 4, 40, seed0=500)
    dt, ot = to_device(t), to_oracle(oracle, t)
    for a in accs:
        for connect in (True, False):
            exp = to_oracle(oracle, a).compose(ot, connect=connect).to_flat()
            got = to_device(a).compose(dt, ComposeConfig(connect=connect)).to_flat()
            assert_flat_identical(got, exp, f"A o T connect={connect}")
            assert exp["n_states"] > 40


def test_compose_wide_lattice_grows_arena(gpu_ctx, oracle, monkeypatch):
    """Sigma=4 makes the BFS frontier grow every level: on the wave-per-problem kernel (pinned) that exercises arena
    overflow + retry; by default the pair is handed to the wide driver as soon as a level is wider than one wave."""
    t = synth.make_transducer(400, 8, 4, 0.0, seed=33)
    a = synth.make_acceptors(t, 1, 30, seed0=9)[0]
    raw = to_oracle(oracle, a).compose(to_oracle(oracle, t), connect=False).to_flat()
    assert raw["n_states"] > 3000
    monkeypatch.setenv("WFST_COMPOSE_PATH", "wave")
    before = gpu_ctx.stats()["compose_retries"]
    got = to_device(a).compose(to_device(t), ComposeConfig(connect=False)).to_flat()
    assert_flat_identical(got, raw, "wide lattice, untrimmed, wave kernel")
    assert gpu_ctx.stats()["compose_retries"] > before
    monkeypatch.delenv("WFST_COMPOSE_PATH")
    got = to_device(a).compose(to_device(t), ComposeConfig(connect=False)).to_flat()
    assert_flat_identical(got, raw, "wide lattice, untrimmed")
    exp = to_oracle(oracle, a).compose(to_oracle(oracle, t)).to_flat()
    got = to_device(a).compose(to_device(t)).to_flat()
    assert_flat_identical(got, exp, "wide lattice, trimmed")


# ------------------------------------------------------------------ shortest path
def check_shortest_path(oracle, flat, dev=None, what=""):
    of = to_oracle(oracle, flat)
    dev = dev or to_device(flat)
    got = dev.shortest_path().to_flat()
    can = of.shortest_path_canonical()
    assert_flat_identical(got, can.to_flat(), f"{what}: vs canonical oracle")
    ref = of.shortest_path()  # reference order + KDELTA
    gw = path_weight(got)
    if np.isinf(ref.total_weight):
        assert got["n_states"] == 0
    else:
        assert abs(gw - ref.total_weight) <= 1e-5, f"{what}: weight {gw} vs reference-mode {ref.total_weight}"
        ok, _ = of.contains_path(oracle.OracleFst.from_flat(**{k: got[k] for k in ("n_states", "start", "offsets", "arcs", "finals", "props")}))
        assert ok, f"{what}: path is not a path of the input"
        if can.n_tied_choices == 0:
            assert_flat_identical(got, ref.to_flat(), f"{what}: unique optimum must equal the reference-mode output")
    return can


def path_weight(flat):
    return np.inf if flat["n_states"] == 0 else float(sum_left_fold(flat))


def sum_left_fold(flat):
    # path arcs are stored from the final end backwards; the reference accumulates from the start state
    acc = np.float32(0.0)
    for w in flat["arcs"]["weight"][::-1]:
        acc = np.float32(acc + w)
    return np.float32(acc + flat["finals"][0])


@pytest.mark.parametrize("seed", range(16))
def test_shortest_path_small_random(gpu_ctx, oracle, seed):
    rng = np.random.default_rng(300 + seed)
    flat = random_fst_flat(rng, int(rng.integers(2, 80)), 4, 6, p_eps_i=0.1, p_final=0.15, min_fanout=0)
    check_shortest_path(oracle, flat, what=f"seed {seed}")


def test_shortest_path_ties_and_zero_weight_cycles(gpu_ctx, oracle):
    """Unweighted cyclic FST: every arc is tight; the hop-layered parent rule must still give a simple path."""
    rng = np.random.default_rng(4)
    flat = random_fst_flat(rng, 50, 4, 3, p_final=0.1, max_w=1, min_fanout=1)  # all weights 0
    can = check_shortest_path(oracle, flat, what="unweighted")
    assert can.n_tied_choices > 0
    flat2 = random_fst_flat(rng, 200, 5, 3, p_final=0.05, max_w=3, weight_grid=1, min_fanout=1)  # weights in {0,1,2}
    check_shortest_path(oracle, flat2, what="small integer weights")


def test_shortest_path_negative_weights_and_unreachable(gpu_ctx, oracle):
    rng = np.random.default_rng(8)
    flat = random_fst_flat(rng, 30, 3, 4, p_final=0.3, acyclic=True, min_fanout=1)
    flat["arcs"]["weight"] -= np.float32(1.5)  # negative weights on a DAG (reference test weights go negative too)
    check_shortest_path(oracle, flat, what="negative")
    # no final reachable -> empty result
    flat["finals"][:] = np.inf
    assert to_device(flat).shortest_path().num_states == 0
    # start None
    flat["start"] = None
    assert to_device(flat).shortest_path().num_states == 0


def test_shortest_distance_matches_oracle(gpu_ctx, oracle):
    t = synth.make_transducer(20000, 10, 256, 0.0, seed=3)
    dist, hops = to_device(t).shortest_distance(want_hops=True)
    can = to_oracle(oracle, t).shortest_path_canonical()
    np.testing.assert_array_equal(dist.view(np.uint32), can.distance.view(np.uint32))
    np.testing.assert_array_equal(hops, can.hops)
    ref = to_oracle(oracle, t).shortest_path(want_distance=True)  # reference order + KDELTA on grid weights
    np.testing.assert_array_equal(dist.view(np.uint32), ref.distance.view(np.uint32))


def test_shortest_path_on_transducer_100k(gpu_ctx, oracle):
    """BASELINE config 2 sized T (100k states / 1M arcs): direct shortest_path(T)."""
    t = synth.make_transducer(100_000, 10, 256, 0.0, seed=2)
    check_shortest_path(oracle, t, what="T 100k")


# ------------------------------------------------------------------ compose -> shortest path, single and batched
def test_config2_compose_then_shortest_path(gpu_ctx, oracle):
    """BASELINE config 2: T = 100k states / 1M arcs, one 1000-arc acceptor (random walk), seed 2."""
    t = synth.make_transducer(100_000, 10, 256, 0.0, seed=2)
    a = synth.make_acceptors(t, 1, 1000, seed0=2)[0]
    dt, da = to_device(t), to_device(a)
    ot, oa = to_oracle(oracle, t), to_oracle(oracle, a)
    oc = oa.compose(ot)
    dc = da.compose(dt)
    assert_flat_identical(dc.to_flat(), oc.to_flat(), "config2 compose")
    got = dc.shortest_path().to_flat()
    can = oc.shortest_path_canonical()
    assert_flat_identical(got, can.to_flat(), "config2 shortest path")
    ref = oc.shortest_path()
    assert abs(float(sum_left_fold(got)) - ref.total_weight) <= 1e-5
    if can.n_tied_choices == 0:
        assert_flat_identical(got, ref.to_flat(), "config2 vs reference mode")
    # fused single-problem batch gives the same path
    outs, n_arcs = rustfst_amd.compose_shortest_path_batch([da], dt)
    assert_flat_identical(outs[0].to_flat(), got, "fused == compose then shortest_path")
    assert n_arcs == oa.compose(ot, connect=False).num_arcs


@pytest.mark.parametrize("p_eps", [0.0, 0.05])
def test_batch_fused_vs_oracle(gpu_ctx, oracle, p_eps):
    t = synth.make_transducer(5000, 8, 32, p_eps, seed=41)
    accs = synth.make_acceptors(t, 24, 30, seed0=1000)
    accs.append(synth.linear_acceptor_flat([1, 2, 3]))         # almost surely no successful path
    accs.append(synth.linear_acceptor_flat([]))                # empty string acceptor
    dt = to_device(t)
    daccs = rustfst_amd.DeviceFst.upload_many(accs)
    outs, n_arcs = rustfst_amd.compose_shortest_path_batch(daccs, dt)
    ot = to_oracle(oracle, t)
    tot = 0
    for i, a in enumerate(accs):
        oc_raw = to_oracle(oracle, a).compose(ot, connect=False)
        tot += oc_raw.num_arcs
        oc = to_oracle(oracle, a).compose(ot, connect=True)
        can = oc.shortest_path_canonical()
        assert_flat_identical(outs[i].to_flat(), can.to_flat(), f"batch item {i}")
        ref = oc.shortest_path()
        if can.n_tied_choices == 0:
            assert_flat_identical(outs[i].to_flat(), ref.to_flat(), f"batch item {i} vs reference mode")
    assert n_arcs == tot
    # oracle batch driver (used as the CPU baseline) agrees with the per-item oracle calls
    o_outs, o_arcs, _ = oracle.compose_shortest_path_batch([to_oracle(oracle, a) for a in accs], ot, n_threads=2)
    assert o_arcs == tot
    for i in range(len(accs)):
        wo, wg = path_weight_or_inf(o_outs[i].to_flat()), path_weight_or_inf(outs[i].to_flat())
        assert (np.isinf(wo) and np.isinf(wg)) or abs(wo - wg) <= 1e-5


def path_weight_or_inf(flat):
    return np.inf if flat["n_states"] == 0 else float(sum_left_fold(flat))


def test_batch_cyclic_composition_needs_fixup(gpu_ctx, oracle):
    """fst1 with cycles: the composition is not layered, the in-kernel relaxation must iterate."""
    rng = np.random.default_rng(12)
    a = random_fst_flat(rng, 12, 3, 4, p_eps_o=0.2, p_final=0.3, sort="olabel", min_fanout=1)
    t = random_fst_flat(rng, 40, 5, 4, p_eps_i=0.2, p_final=0.2, sort="ilabel", min_fanout=1)
    outs, _ = rustfst_amd.compose_shortest_path_batch([to_device(a)], to_device(t))
    oc = to_oracle(oracle, a).compose(to_oracle(oracle, t))
    assert_flat_identical(outs[0].to_flat(), oc.shortest_path_canonical().to_flat(), "cyclic fused")


# ------------------------------------------------------------------ I/O and round trips
@pytest.mark.parametrize("name", ["sigma_matcher_2_left.fst", "sigma_matcher_2_right.fst"])
def test_openfst_binary_round_trip(gpu_ctx, oracle, name):
    data = open(os.path.join(GOLDEN, name), "rb").read()
    d = rustfst_amd.DeviceFst.from_bytes(data)
    o = oracle.OracleFst.load(data)
    assert_flat_identical(d.to_flat(), o.to_flat(), name)
    assert d.to_bytes() == o.store()
    v = VectorFst.from_bytes(data)
    assert VectorFst.from_bytes(v.to_bytes()) == v


def test_upload_device_pointers(gpu_ctx, oracle):
    torch = pytest.importorskip("torch")
    t = synth.make_transducer(1000, 5, 16, 0.0, seed=5)
    off = torch.from_numpy(t["offsets"].astype(np.int64)).to(torch.int32).cuda()
    arcs = torch.from_numpy(t["arcs"].view(np.uint8).reshape(-1, 16)).cuda()
    fin = torch.from_numpy(t["finals"]).cuda()
    torch.cuda.synchronize()
    d = rustfst_amd.DeviceFst.from_device_arrays(t["n_states"], 0, off.data_ptr(), arcs.data_ptr(), fin.data_ptr(),
                                                 t["props"])
    assert_flat_identical(d.to_flat(), t, "device upload")


# ------------------------------------------------------------------ size-independent properties at BASELINE size
def test_config3_properties_1m_states(gpu_ctx, oracle):
    """BASELINE config 3 (1M states / 10M arcs): properties that do not need the oracle at full size."""
    t = synth.make_transducer(1_000_000, 10, 256, 0.0, seed=3)
    accs = synth.make_acceptors(t, 8, 200, seed0=1000)
    dt = to_device(t)
    dist, hops = dt.shortest_distance(want_hops=True)
    arcs, off = t["arcs"], t["offsets"]
    src = np.repeat(np.arange(t["n_states"], dtype=np.int64), np.diff(off.astype(np.int64)))
    cand = (dist[src] + arcs["weight"]).astype(np.float32)
    # fixed point: no arc can still improve its head; every reached non-start state has a tight incoming arc
    assert np.all(cand >= dist[arcs["nextstate"]])
    tight = cand == dist[arcs["nextstate"]]
    has_tight = np.zeros(t["n_states"], dtype=bool)
    has_tight[arcs["nextstate"][tight]] = True
    reached = np.isfinite(dist)
    assert reached.all() and has_tight[1:].all() and dist[0] == 0.0
    # idempotence + path checks
    sp = dt.shortest_path()
    spf = sp.to_flat()
    assert spf["n_states"] >= 2
    fin_states = np.flatnonzero(np.isfinite(t["finals"]))
    best = np.min((dist[fin_states] + t["finals"][fin_states]).astype(np.float32))
    assert float(sum_left_fold(spf)) == float(best)
    assert_flat_identical(sp.shortest_path().to_flat(), spf, "shortest_path is idempotent on its own output", check_props=False)
    # batch: each result reads exactly its acceptor's label string, and the oracle agrees on a sample
    outs, _ = rustfst_amd.compose_shortest_path_batch(rustfst_amd.DeviceFst.upload_many(accs), dt)
    ot = to_oracle(oracle, t)
    for i, (a, o) in enumerate(zip(accs, outs)):
        f = o.to_flat()
        assert f["n_states"] == 201
        np.testing.assert_array_equal(f["arcs"]["ilabel"][::-1], a["arcs"]["ilabel"])
        if i < 2:
            can = to_oracle(oracle, a).compose(ot).shortest_path_canonical()
            assert_flat_identical(f, can.to_flat(), f"1M batch item {i}")


@pytest.mark.parametrize("kernel", ["mailbox", "mailbox_no_narrow", "mailbox_one_level", "atomic", "binned", "binned_every_level"])
def test_config3_benched_solve_bit_exact_vs_oracle(oracle, monkeypatch, kernel):
    """The solve bench.py times — shortest_path(T), T = 1M states / 10M arcs, seed 3 — against the canonical oracle at full
    size: every distance, every hop count and the path itself bit-identical, for the mailbox launches (with and without
    the NARROW hand-over), for the atomic sweeps, and for the atomic sweeps with their dense levels as binned passes (chosen
    per level on the device / every level), on a first and on a repeated (predicted, gate-hinted) query."""
    monkeypatch.setenv("WFST_SSSP_MAILBOX", "0" if kernel in ("atomic", "binned", "binned_every_level") else "1")
    if kernel.startswith("binned"):
        monkeypatch.setenv("WFST_SSSP_BINNED", "1")
    if kernel == "binned_every_level":
        monkeypatch.setenv("WFST_SSSP_DENSE_LOW", "0")
    if kernel == "mailbox_no_narrow":
        monkeypatch.setenv("WFST_SSSP_NARROW", "0")
    if kernel == "mailbox_one_level":
        monkeypatch.setenv("WFST_SSSP_RESIDENT", "0")
    ctx = rustfst_amd.Context(0)
    t = synth.make_transducer(1_000_000, 10, 256, 0.0, seed=3)
    d = to_device(t, ctx)
    can = to_oracle(oracle, t).shortest_path_canonical()
    for q in range(3):
        dist, hops = d.shortest_distance(want_hops=True)
        assert ctx.stats()["relax_kernel"] == {"atomic": 0, "mailbox_one_level": 1, "binned": 3, "binned_every_level": 3}.get(kernel, 2)
        np.testing.assert_array_equal(dist.view(np.uint32), can.distance.view(np.uint32))
        np.testing.assert_array_equal(hops, can.hops)
        assert_flat_identical(d.shortest_path().to_flat(), can.to_flat(), f"benched solve, {kernel}, query {q}")
    assert ctx.stats()["resident_aborts"] == 0


def test_config3_512_acceptors_and_one_long_string_against_1m_states(gpu_ctx, oracle):
    """BASELINE configs[3] in its one-GPU form: all 512 linear acceptors (len 200) of the batch against the shared
    1M-state / 10M-arc T in one fused call — every path spells its acceptor, a random 16 are bit-identical to the oracle —
    and the single-string case of SURVEY §8(d) (C3-S2): ONE acceptor of length 1000 against the same T, composition and
    shortest path bit-identical to the oracle, through the two-step route and through the fused call."""
    t = synth.make_transducer(1_000_000, 10, 256, 0.0, seed=3)
    accs = synth.make_acceptors(t, 512, 200, seed0=1000)
    long_acc = synth.make_acceptors(t, 1, 1000, seed0=31)[0]
    dt, ot = to_device(t), to_oracle(oracle, t)
    outs, n_arcs = rustfst_amd.compose_shortest_path_batch(rustfst_amd.DeviceFst.upload_many(accs), dt)
    assert len(outs) == 512 and n_arcs >= 512 * 200
    flats = [o.to_flat() for o in outs]
    for a, f in zip(accs, flats):
        assert f["n_states"] == 201
        np.testing.assert_array_equal(f["arcs"]["ilabel"][::-1], a["arcs"]["ilabel"])
    for i in np.random.default_rng(5).choice(512, 16, replace=False):
        can = to_oracle(oracle, accs[i]).compose(ot).shortest_path_canonical()
        assert_flat_identical(flats[i], can.to_flat(), f"512-batch item {i}")
    # one long string
    oc = to_oracle(oracle, long_acc).compose(ot)
    dc = to_device(long_acc).compose(dt)
    assert_flat_identical(dc.to_flat(), oc.to_flat(), "A(1000) o T(1M)")
    can = oc.shortest_path_canonical().to_flat()
    assert can["n_states"] == 1001
    assert_flat_identical(dc.shortest_path().to_flat(), can, "shortest_path(A(1000) o T(1M))")
    one, _ = rustfst_amd.compose_shortest_path_batch([to_device(long_acc)], dt)
    assert_flat_identical(one[0].to_flat(), can, "fused A(1000) o T(1M)")


def test_config5_lookahead_compose_and_nbest_at_scale_invariants_only():
    """BASELINE configs[4] end to end (tools/config5_lookahead.py): the 5M-state / 50M-arc HCLG-shaped FST with 5 %
    epsilons as the look-ahead operand (reachability data built once), 64 linear acceptors of 200 labels — relabel,
    look-ahead composition (one by one and as ONE batch), n = 10 shortest paths of every result.  Checked without an
    oracle at this size: the 10 best path weights equal those of the plain composition (+ connect) of the same pair,
    the best path spells the acceptor, the batch gives the same state counts as the one-by-one calls."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "config5_lookahead.py"), "5000000", "64"], capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-2000:]


def test_config5_lookahead_full_size_sample_vs_oracle(oracle):
    """BASELINE configs[4] at its FULL operand size against the oracle on a sample: the 5M-state / 50M-arc HCLG-shaped FST (5 %
    output epsilons) as the look-ahead operand, two of the 200-label acceptors — the look-ahead composition (label
    reachability over 5M states, relabelling, the filter stack) bit-identical to the oracle's: states, arc order, labels,
    weight bits, finals; and the n = 10 shortest paths of the first result identical to the oracle's on ITS result.  (The
    oracle redoes MatcherFst::new per composition, as rustfst-cli does: ~9 s each on one core.)  WFST_TEST_CONFIG5_SAMPLE=k
    takes k acceptors of the batch instead of 2 (the long run: 8 of 64 is ~80 s of oracle time)."""
    n = 5_000_000
    t = synth.make_transducer(n, 10, 256, 0.05, seed=9)
    accs = synth.make_acceptors(t, max(2, min(64, int(os.environ.get("WFST_TEST_CONFIG5_SAMPLE", "2")))), 200, seed0=77)
    arcs = t["arcs"].copy()
    arcs["ilabel"], arcs["olabel"] = t["arcs"]["olabel"].copy(), t["arcs"]["ilabel"].copy()
    t1 = dict(t, arcs=arcs, props=synth.O_LABEL_SORTED)
    ctx = rustfst_amd.Context(0)
    la = rustfst_amd.LookAhead(to_device(t1, ctx))
    o1 = to_oracle(oracle, t1)
    for i, a in enumerate(accs):
        got = la.compose(la.relabel(to_device(a, ctx)))
        exp = o1.compose_lookahead(to_oracle(oracle, a))
        g, e = got.to_flat(), exp.to_flat()
        assert g["n_states"] == e["n_states"] and g["n_states"] > 100, (i, g["n_states"], e["n_states"])
        assert_flat_identical(g, e, f"look-ahead composition at 5M states, acceptor {i}")
        if i == 0:
            assert_flat_identical(got.shortest_path(ShortestPathConfig(nshortest=10)).to_flat(), exp.shortest_path_n(10).to_flat(),
                                  "n = 10 shortest paths of the 5M-state look-ahead composition")


@pytest.mark.parametrize("delta", ["0", "0.7", "3", "1000"])
def test_near_far_schedule_does_not_change_results(oracle, delta, monkeypatch):
    """The near-far threshold schedule only reorders relaxations: distances, hops and the path are the
    fixed point regardless of delta (0 = plain frontier sweeps)."""
    os.environ["WFST_SSSP_DELTA"] = delta
    monkeypatch.setenv("WFST_SSSP_MAILBOX", "0")
    try:
        ctx = rustfst_amd.Context(0)
        for n, fan, seed in ((20_000, 8, 1), (3_000, 20, 2), (200_000, 10, 3)):
            t = synth.make_transducer(n, fan, 64, 0.02, seed=seed)
            d = to_device(t, ctx)
            dist, hops = d.shortest_distance(want_hops=True)
            can = to_oracle(oracle, t).shortest_path_canonical()
            np.testing.assert_array_equal(dist.view(np.uint32), can.distance.view(np.uint32))
            np.testing.assert_array_equal(hops, can.hops)
            assert_flat_identical(d.shortest_path().to_flat(), can.to_flat(), f"delta={delta} n={n}")
    finally:
        del os.environ["WFST_SSSP_DELTA"]


@pytest.mark.parametrize("cap,budget,low", [(0, 0, 0), (1, 1, 1 << 30), (8, 3, 1 << 30), (32, 8, 4096), (128, 1000, 1 << 30),
                                            (128, 1000, 64), (5, 1000, 1 << 30)])
@pytest.mark.parametrize("delta", [None, "0", "0.7"])
def test_chasing_does_not_change_results(oracle, monkeypatch, cap, budget, low, delta):
    """Waves relaxing their own near discoveries inside the same launch only reorder relaxations:
    list capacity, per-launch budget and the small-sweep gate (1<<30 = chase in every sweep) leave distances, hops
    and the path untouched, on branching graphs (with and without epsilons), a sparse deep one and small cyclic FSTs
    with many ties."""
    monkeypatch.setenv("WFST_SSSP_CHASE_CAP", str(cap))
    monkeypatch.setenv("WFST_SSSP_CHASE_ROUNDS", str(budget))
    monkeypatch.setenv("WFST_SSSP_CHASE_LOW", str(low))
    if delta is not None:
        monkeypatch.setenv("WFST_SSSP_DELTA", delta)
    ctx = rustfst_amd.Context(0)
    for n, fan, p_eps, seed in ((70_000, 8, 0.02, 1), (3_000, 20, 0.0, 2), (30_000, 2, 0.3, 3)):
        t = synth.make_transducer(n, fan, 64, p_eps, seed=seed)
        d = to_device(t, ctx)
        can = to_oracle(oracle, t).shortest_path_canonical()
        for q in range(2):
            dist, hops = d.shortest_distance(want_hops=True)
            np.testing.assert_array_equal(dist.view(np.uint32), can.distance.view(np.uint32))
            np.testing.assert_array_equal(hops, can.hops)
            assert_flat_identical(d.shortest_path().to_flat(), can.to_flat(), f"chase {cap}/{budget}/{low} n={n} q={q}")
    rng = np.random.default_rng(cap * 1000 + budget)
    for k in range(6):  # small cyclic FSTs with epsilons and ties
        f = random_fst_flat(rng, int(rng.integers(2, 200)), 5, 3, p_eps_i=0.1, p_eps_o=0.1, p_final=0.2, weight_grid=4, max_w=12)
        ref = to_oracle(oracle, f).shortest_path_canonical().to_flat()
        assert_flat_identical(to_device(f, ctx).shortest_path().to_flat(), ref, f"chase small {k}")


@pytest.mark.parametrize("mailbox", ["1", "1:narrow=0", "1:narrow=1000000000", "1:narrow=64", "1:hint=0", "1:hint=1", "0",
                                     "1:res=0", "1:reslevels=2", "1:reslevels=3", "1:restlim=0"])
@pytest.mark.parametrize("delta", [None, "0", "0.7", "1000"])
def test_mailbox_sweeps_do_not_change_results(oracle, monkeypatch, mailbox, delta):
    """The owner-computes (mailbox) sweeps and the atomic sweeps reach the same fixed point: distances, hop counts and
    the path are bit-identical to the canonical oracle on graphs of less than one block, a partial last block, many
    blocks, a sparse deep graph, epsilons, ties everywhere, and whatever the near-far band width is — with the hand-over
    to NARROW launches off (narrow=0), at its default, forced whenever a sweep was busy (narrow=1e9: WIDE / COLLECT /
    NARROW in turn, segments that overflow), and with every launch / no launch gated (hint).  The WIDE levels run inside
    resident launches by default (sssp_mbox_resident_kernel): also without them (res=0), with launches cut after two / three
    levels (every level a first or a last one, hand-overs between the two kernels in both directions), and with a wait
    limit of zero (the first header that is not there yet makes the launch give up: the solve is repeated with one launch
    per level and the context stays in that mode)."""
    monkeypatch.setenv("WFST_SSSP_MAILBOX", mailbox.split(":")[0])
    monkeypatch.setenv("WFST_SSSP_RES_RETRY_MS", "600000")  # (after an abort: no second resident attempt inside this test)
    if ":" in mailbox:
        k, v = mailbox.split(":")[1].split("=")
        monkeypatch.setenv({"narrow": "WFST_SSSP_NARROW", "hint": "WFST_SSSP_HINT", "res": "WFST_SSSP_RESIDENT",
                            "reslevels": "WFST_SSSP_RES_LEVELS", "restlim": "WFST_SSSP_RES_TLIM_US"}[k], v)
    if delta is not None:
        monkeypatch.setenv("WFST_SSSP_DELTA", delta)
    ctx = rustfst_amd.Context(0)
    for n, fan, p_eps, seed in ((70_000, 8, 0.02, 1), (3_000, 20, 0.0, 2), (30_000, 2, 0.3, 3), (4_096, 6, 0.0, 4),
                                (4_097, 6, 0.0, 5), (150_000, 10, 0.0, 6)):
        t = synth.make_transducer(n, fan, 64, p_eps, seed=seed)
        d = to_device(t, ctx)
        can = to_oracle(oracle, t).shortest_path_canonical()
        for q in range(3):
            dist, hops = d.shortest_distance(want_hops=True)
            np.testing.assert_array_equal(dist.view(np.uint32), can.distance.view(np.uint32))
            np.testing.assert_array_equal(hops, can.hops)
            assert_flat_identical(d.shortest_path().to_flat(), can.to_flat(), f"mailbox={mailbox} delta={delta} n={n} q={q}")
    rng = np.random.default_rng(77)
    for k in range(8):  # small cyclic FSTs with epsilons and ties (integer weights)
        f = random_fst_flat(rng, int(rng.integers(2, 300)), 5, 3, p_eps_i=0.1, p_eps_o=0.1, p_final=0.2, weight_grid=1, max_w=4)
        ref = to_oracle(oracle, f).shortest_path_canonical().to_flat()
        assert_flat_identical(to_device(f, ctx).shortest_path().to_flat(), ref, f"mailbox small {k}")


def _reweighted(t, family, seed):
    """T with its arc weights replaced by an arbitrary-f32 family (the fixtures and benchmarks all use k/512: there the exact ==
    of this engine and the reference's approximate one cannot differ, and neither can an ordering bug of the encoded keys hide)"""
    rng = np.random.default_rng(seed)
    t = dict(t)
    arcs = t["arcs"].copy()
    e = arcs.shape[0]
    if family == "uniform_1e-3":
        w = rng.random(e, dtype=np.float32) * np.float32(1e-3)
    elif family == "lognormal_12_decades":
        w = np.power(10.0, rng.uniform(-6.0, 6.0, e)).astype(np.float32)
    elif family == "subnormal":  # k x 2^-149, and a few ordinary tiny values among them: sums cross the subnormal boundary
        w = (rng.integers(0, 1 << 22, e).astype(np.uint32)).view(np.float32).copy()
        pick = rng.random(e) < 0.05
        w[pick] = (rng.random(int(pick.sum()), dtype=np.float32) * np.float32(1e-37)).astype(np.float32)
    elif family == "huge":  # sums overflow to +inf (which never improves, shortest_path.rs:226) on most two-arc paths
        w = (rng.random(e, dtype=np.float32) * np.float32(3.0e38)).astype(np.float32)
        w[rng.random(e) < 0.3] = np.float32(1.0)
    elif family == "negative_dag":  # arcs forward only (window 40 000 states: crosses blocks), weights in [-5, 5)
        n = t["n_states"]
        src = np.repeat(np.arange(n, dtype=np.int64), np.diff(t["offsets"].astype(np.int64)))
        room = np.maximum(1, np.minimum(40_000, n - 1 - src))
        ns = src + 1 + (arcs["nextstate"].astype(np.int64) % room)
        keep = src < n - 1
        arcs, src, ns = arcs[keep], src[keep], ns[keep]
        arcs["nextstate"] = ns.astype(np.uint32)
        t["offsets"] = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=n))]).astype(np.uint32)
        w = (rng.random(arcs.shape[0], dtype=np.float32) * np.float32(10.0) - np.float32(5.0)).astype(np.float32)
        t["props"] = int(synth.I_LABEL_SORTED | synth.ACYCLIC | synth.INITIAL_ACYCLIC | synth.TOP_SORTED)
        t["finals"] = t["finals"].copy()
        t["finals"][n - 1] = np.float32(0.25)
    else:
        raise ValueError(family)
    arcs["weight"] = w
    t["arcs"] = arcs
    return t


@pytest.mark.parametrize("kernel", ["resident", "mailbox_one_level", "atomic"])
@pytest.mark.parametrize("family", ["uniform_1e-3", "lognormal_12_decades", "subnormal", "huge", "negative_dag"])
def test_arbitrary_f32_weights_bit_exact_vs_canonical_oracle(oracle, monkeypatch, family, kernel):
    """Distances, hop counts and the path on weights that are NOT on a coarse grid — uniform [0, 1e-3), twelve decades,
    subnormals, values whose sums overflow, negative weights on a DAG — bit-identical to the canonical oracle (the exact (min,+)
    fixed point of left-folded f32 sums) under the resident launches, the one-level mailbox launches and the atomic
    sweeps (negative weights always take the atomic sweeps).  What this pins: the order-preserving u32 encoding of f32 distances
    inside the 64-bit keys (f32_key / key_f32, incl. negative values and subnormals), `+ 0.0f` normalisation, +inf candidates
    dropped, and that no kernel flushes subnormals.  semirings/semiring.rs:159-168 is the reference's approximate compare this
    engine does not use."""
    monkeypatch.setenv("WFST_SSSP_MAILBOX", "0" if kernel == "atomic" else "1")
    if kernel == "mailbox_one_level":
        monkeypatch.setenv("WFST_SSSP_RESIDENT", "0")
    ctx = rustfst_amd.Context(0)
    t = _reweighted(synth.make_transducer(150_000, 8, 64, 0.0, seed=11), family, seed=5)
    d = to_device(t, ctx)
    can = to_oracle(oracle, t).shortest_path_canonical()
    assert np.isfinite(can.distance).sum() > 1000  # (the search is not trivial under any family)
    for q in range(2):
        dist, hops = d.shortest_distance(want_hops=True)
        if family != "negative_dag":
            assert ctx.stats()["relax_kernel"] == {"atomic": 0, "mailbox_one_level": 1, "resident": 2}[kernel]
        np.testing.assert_array_equal(dist.view(np.uint32), can.distance.view(np.uint32))
        # The hop component of a key is a tie-breaking device.  With INEXACT sums it is not a function of the graph alone:
        # when two sources' different distances round to the same sum (absorption: d + w == d across twelve decades), the
        # (d, hops) recurrence is not monotone and a state may keep a hop count derived from a label its predecessor has
        # since improved — which relaxation came first decides, in the oracle's FIFO as in any kernel's
        # schedule.  Distances are the unique fixed point whatever the schedule; the hop counts agree wherever no such
        # collision occurs (every state of the other families; all but a few dozen of 150 000 here).
        n_diff = int(np.count_nonzero(hops != can.hops))
        if family == "lognormal_12_decades":
            assert n_diff <= 150, n_diff
        else:
            assert n_diff == 0, n_diff
        # the path: forced when the optimum is unique (no state of it has a second tight in-arc), whatever the hop counts say
        assert can.n_tied_choices == 0
        assert_flat_identical(d.shortest_path().to_flat(), can.to_flat(), f"{family}, {kernel}, query {q}")
    assert ctx.stats()["resident_aborts"] == 0


@pytest.mark.parametrize("narrow", [None, "0", "1000000000"])
def test_mailbox_sweeps_beyond_2_20_states(oracle, monkeypatch, narrow):
    """More than 256 blocks of 4096 states (2.1M states, 10.5M arcs): the owner-computes sweeps visit their inbox regions
    in passes and stage fewer messages per destination; distances, hop counts and the path are bit-identical to the
    canonical oracle, and the mailbox kernel is what ran."""
    if narrow is not None:
        monkeypatch.setenv("WFST_SSSP_NARROW", narrow)
    ctx = rustfst_amd.Context(0)
    t = synth.make_transducer(2_100_000, 5, 64, 0.0, seed=11)
    d = to_device(t, ctx)
    can = to_oracle(oracle, t).shortest_path_canonical()
    for q in range(2):
        dist, hops = d.shortest_distance(want_hops=True)
        assert ctx.stats()["relax_kernel"] == 1  # (more than 256 blocks: one launch per level)
        np.testing.assert_array_equal(dist.view(np.uint32), can.distance.view(np.uint32))
        np.testing.assert_array_equal(hops, can.hops)
        assert_flat_identical(d.shortest_path().to_flat(), can.to_flat(), f"2.1M states q={q}")


@pytest.mark.parametrize("variant", ["default", "dense_low=0", "dense_low=3000", "dense_low=4000000000", "log=14", "hopcap=3",
                                     "dense_low=0,log=14,hopcap=2"])
@pytest.mark.parametrize("delta", ["0.7", "3", "1000"])
def test_binned_levels_do_not_change_results(oracle, monkeypatch, variant, delta):
    """The dense levels of the atomic sweeps as owner-computes passes (sssp_bin_expand_kernel / sssp_bin_apply_kernel, chosen
    per level on the device: sssp_binned.h) reach the same fixed point: distances, hop counts and the path bit-identical to
    the canonical oracle — with the choice left to the device, with every level but the first binned (dense_low=0), with a
    low and an unreachable threshold, with 16384-state bins, and with a hop limit of two / three arcs in the message format (deeper states relax through the atomic path inside the
    expand kernel) — on graphs of one bin, a partial last bin, several source ranges, epsilons, a sparse deep graph."""
    monkeypatch.setenv("WFST_SSSP_MAILBOX", "0")
    monkeypatch.setenv("WFST_SSSP_BINNED", "1")
    monkeypatch.setenv("WFST_SSSP_DELTA", delta)
    if variant != "default":
        for kv in variant.split(","):
            k, v = kv.split("=")
            monkeypatch.setenv({"dense_low": "WFST_SSSP_DENSE_LOW", "log": "WFST_SSSP_BIN_LOG", "hopcap": "WFST_SSSP_BIN_HOPCAP"}[k], v)
    ctx = rustfst_amd.Context(0)
    for n, fan, p_eps, seed in ((70_000, 8, 0.02, 1), (3_000, 20, 0.0, 2), (30_000, 2, 0.3, 3), (8_192, 6, 0.0, 4),
                                (8_193, 6, 0.0, 5), (300_000, 10, 0.0, 6)):
        t = synth.make_transducer(n, fan, 64, p_eps, seed=seed)
        d = to_device(t, ctx)
        can = to_oracle(oracle, t).shortest_path_canonical()
        for q in range(3):
            dist, hops = d.shortest_distance(want_hops=True)
            assert ctx.stats()["relax_kernel"] == 3
            np.testing.assert_array_equal(dist.view(np.uint32), can.distance.view(np.uint32))
            np.testing.assert_array_equal(hops, can.hops)
            assert_flat_identical(d.shortest_path().to_flat(), can.to_flat(), f"binned {variant} delta={delta} n={n} q={q}")
    rng = np.random.default_rng(78)
    for k in range(8):  # small cyclic FSTs with epsilons and ties (integer weights)
        f = random_fst_flat(rng, int(rng.integers(2, 300)), 5, 3, p_eps_i=0.1, p_eps_o=0.1, p_final=0.2, weight_grid=1, max_w=4)
        ref = to_oracle(oracle, f).shortest_path_canonical().to_flat()
        assert_flat_identical(to_device(f, ctx).shortest_path().to_flat(), ref, f"binned small {k}")


def test_binned_levels_are_what_runs_the_dense_levels(monkeypatch):
    """A profiled solve reports what ran each level (wfst_ctx_get_sweep_modes): with the choice left to the device, the
    first levels of a 400k-state search are atomic sweeps, its widest ones binned passes; the per-level arc counts add up
    to the same relaxation whichever kernel ran them."""
    monkeypatch.setenv("WFST_SSSP_MAILBOX", "0")
    monkeypatch.setenv("WFST_SSSP_BINNED", "1")
    ctx = rustfst_amd.Context(0)
    t = synth.make_transducer(400_000, 10, 256, 0.0, seed=9)
    d = to_device(t, ctx)
    d.shortest_path()
    ctx.reset_stats(); ctx.set_profiling(True); d.shortest_path(); ctx.set_profiling(False)
    ms, arcs, states = ctx.sweep_trace()
    modes = ctx.sweep_modes()
    assert ctx.stats()["relax_kernel"] == 3
    assert modes[0] == 0 and set(modes.tolist()) == {0, 7}
    assert states[modes == 7].min() > states[modes == 0].max() // 8  # (the prediction is a bound, not the count)
    assert int(arcs.sum()) >= int(t["arcs"].shape[0])  # every arc of a strongly connected T at least once


@pytest.mark.parametrize("kernel", ["hybrid", "binned_every_level", "atomic"])
def test_config5_size_solve_bit_exact_vs_oracle(oracle, monkeypatch, kernel):
    """configs[4]'s size — 5M states / 50M arcs, the generator of `roofline_vs_size` — against the canonical oracle at FULL size:
    every distance, every hop count and the path bit-identical with the atomic sweeps (the default there), with their dense
    levels as binned passes chosen per level on the device, and with every level binned."""
    if not kernel.startswith("atomic"):
        monkeypatch.setenv("WFST_SSSP_BINNED", "1")
    if kernel == "binned_every_level":
        monkeypatch.setenv("WFST_SSSP_DENSE_LOW", "0")
    ctx = rustfst_amd.Context(0)
    t = synth.make_transducer(5_000_000, 10, 256, 0.0, seed=3)
    d = to_device(t, ctx)
    can = to_oracle(oracle, t).shortest_path_canonical()
    for q in range(2):
        dist, hops = d.shortest_distance(want_hops=True)
        assert ctx.stats()["relax_kernel"] == (0 if kernel.startswith("atomic") else 3)
        np.testing.assert_array_equal(dist.view(np.uint32), can.distance.view(np.uint32))
        np.testing.assert_array_equal(hops, can.hops)
        assert_flat_identical(d.shortest_path().to_flat(), can.to_flat(), f"5M-state solve, {kernel}, query {q}")


@pytest.mark.parametrize("variant", [None, "reslevels=3", "restlim=0", "narrow=0", "fail13=1"])
def test_resident_launches_with_8192_state_blocks(oracle, monkeypatch, variant):
    """Between 2^20 and 2^21 states a block of 4096 states per compute unit no longer covers the FST: the resident kernel
    then owns blocks of 8192 states (64 KB of keys in LDS) and runs EVERY launch of the solve, the NARROW ones included.
    1.3M states / 6.5M arcs: distances, hop counts and the path bit-identical to the canonical oracle; with launches cut
    after three levels (hand-overs inside the one kernel), without the NARROW hand-over, and with a wait limit of zero
    (the launch gives up, the solve is repeated with 4096-state blocks and one launch per level), and with the 8192-state plan
    refused (a pool too tight for it, a region buffer beyond the descriptor range: the solve is planned again with 4096-state
    blocks, never refused)."""
    monkeypatch.setenv("WFST_SSSP_RES_RETRY_MS", "600000")  # (after an abort: no second resident attempt inside this test)
    if variant:
        k, v = variant.split("=")
        monkeypatch.setenv({"reslevels": "WFST_SSSP_RES_LEVELS", "restlim": "WFST_SSSP_RES_TLIM_US", "narrow": "WFST_SSSP_NARROW",
                            "fail13": "WFST_SSSP_TEST_FAIL_LOG13"}[k], v)
    ctx = rustfst_amd.Context(0)
    t = synth.make_transducer(1_300_000, 5, 64, 0.0, seed=12)
    d = to_device(t, ctx)
    can = to_oracle(oracle, t).shortest_path_canonical()
    for q in range(3):
        dist, hops = d.shortest_distance(want_hops=True)
        st = ctx.stats()
        if variant == "restlim=0":
            assert st["resident_aborts"] == 1 and st["relax_kernel"] == 1
        elif variant == "fail13=1":
            assert st["resident_aborts"] == 0 and st["relax_kernel"] == 1
        else:
            assert st["resident_aborts"] == 0 and st["relax_kernel"] == 2
        np.testing.assert_array_equal(dist.view(np.uint32), can.distance.view(np.uint32))
        np.testing.assert_array_equal(hops, can.hops)
        assert_flat_identical(d.shortest_path().to_flat(), can.to_flat(), f"1.3M states ({variant}) q={q}")


def test_resident_launches_are_tried_again_after_an_abort(oracle, monkeypatch):
    """A resident launch that gives up waiting (wait limit 0 here) costs that solve a repeat with one launch per level and
    the context a PAUSE, not the resident path for good: inside the pause solves take one launch per level without trying,
    after it the next solve is a resident one again (wfst_ctx::resident_retry_at_ns; the pause doubles with every abort in a
    row and is forgotten by the first resident solve that completes).  Every result bit-identical to the canonical oracle."""
    ctx = rustfst_amd.Context(0)
    t = synth.make_transducer(300_000, 8, 64, 0.0, seed=14)
    d = to_device(t, ctx)
    can = to_oracle(oracle, t).shortest_path_canonical().to_flat()

    def solve(label, kernel, aborts):
        got = d.shortest_path().to_flat()
        st = ctx.stats()
        assert (st["relax_kernel"], st["resident_aborts"]) == (kernel, aborts), (label, st["relax_kernel"], st["resident_aborts"])
        assert_flat_identical(got, can, label)

    solve("first", 2, 0)
    monkeypatch.setenv("WFST_SSSP_RES_TLIM_US", "0")
    monkeypatch.setenv("WFST_SSSP_RES_RETRY_MS", "0")
    solve("aborts, no pause", 1, 1)
    solve("aborts again at once", 1, 2)
    monkeypatch.delenv("WFST_SSSP_RES_TLIM_US")
    solve("resident again", 2, 2)
    monkeypatch.setenv("WFST_SSSP_RES_TLIM_US", "0")
    monkeypatch.setenv("WFST_SSSP_RES_RETRY_MS", "600000")
    solve("aborts, long pause", 1, 3)
    monkeypatch.delenv("WFST_SSSP_RES_TLIM_US")
    solve("inside the pause: one launch per level, no attempt", 1, 3)


def test_resident_solve_next_to_a_batch_that_fills_the_compute_units(oracle, monkeypatch):
    """shortest_path(T) (1M states: a resident grid of 245 workgroups, one per compute unit) issued while a 4096-acceptor
    fused batch holds the compute units on another context: bit-identical to the canonical oracle every time, at most one
    abort per solve, and the solve after the batch is a resident one again."""
    torch = pytest.importorskip("torch")
    monkeypatch.setenv("WFST_SSSP_RES_RETRY_MS", "0")
    t = synth.make_transducer(1_000_000, 10, 256, 0.0, seed=3)
    accs = synth.make_acceptors(t, 4096, 200, seed0=1000)
    ctx = rustfst_amd.Context(0)
    s2 = torch.cuda.Stream()
    ctx2 = rustfst_amd.Context(0, stream=s2.cuda_stream)
    dt = to_device(t, ctx)
    daccs = rustfst_amd.DeviceFst.upload_many(accs, ctx2)
    can = to_oracle(oracle, t).shortest_path_canonical().to_flat()
    for _ in range(3):
        assert_flat_identical(dt.shortest_path().to_flat(), can, "alone")
    assert ctx.stats()["relax_kernel"] == 2 and ctx.stats()["resident_aborts"] == 0
    first = None
    reps = 5
    for rep in range(reps):
        job = rustfst_amd.compose_shortest_path_batch_begin(daccs, dt, ctx=ctx2)
        sp = dt.shortest_path()
        outs, n_arcs = job.finish()
        assert_flat_identical(sp.to_flat(), can, f"next to the batch, rep {rep}")
        flat = [o.to_flat() for o in outs[:8]]
        if first is None:
            first = flat
        for a, b in zip(flat, first):
            assert_flat_identical(a, b, f"batch results, rep {rep}")
    assert ctx.stats()["resident_aborts"] <= reps
    assert_flat_identical(dt.shortest_path().to_flat(), can, "after the batches")
    assert ctx.stats()["relax_kernel"] == 2


@pytest.mark.parametrize("order", ["s1-first", "s2-first"])
def test_resident_share_half_runs_beside_a_512_string_batch(oracle, order):
    """configs[3] on ONE GPU: shortest_path(T) (1M states) and the fused batch of all 512 acceptors, overlapped on two contexts,
    in both enqueue orders, with the query's context set to HALF the device (wfst_ctx_set_resident_share(ctx, 1): 123
    workgroups of 8192 states instead of 245 of 4096, so that the batch's 64 compute units and the solve's 123 fit side by
    side).  Every repetition: the path and all distances bit-identical to the canonical oracle, a sample of the batch
    bit-identical to the oracle's compose -> shortest path, no resident launch gives up; and the default share still takes
    4096-state blocks afterwards."""
    torch = pytest.importorskip("torch")
    t = synth.make_transducer(1_000_000, 10, 256, 0.0, seed=3)
    accs = synth.make_acceptors(t, 512, 200, seed0=50_000)
    ctx = rustfst_amd.Context(0)
    s2 = torch.cuda.Stream()
    ctx2 = rustfst_amd.Context(0, stream=s2.cuda_stream)
    ctx.set_resident_share(1)
    dt = to_device(t, ctx)
    daccs = rustfst_amd.HandleArray(rustfst_amd.DeviceFst.upload_many(accs, ctx2))
    ot = to_oracle(oracle, t)
    can = ot.shortest_path_canonical()
    can_flat = can.to_flat()
    exp = {i: to_oracle(oracle, accs[i]).compose(ot, connect=True).shortest_path_canonical().to_flat() for i in (0, 255, 511)}
    dist, hops = dt.shortest_distance(want_hops=True)
    np.testing.assert_array_equal(dist.view(np.uint32), can.distance.view(np.uint32))
    np.testing.assert_array_equal(hops, can.hops)
    assert ctx.stats()["relax_kernel"] == 2
    for rep in range(6):
        if order == "s1-first":
            sp_job = dt.shortest_path_begin()
            job = rustfst_amd.compose_shortest_path_batch_begin(daccs, dt, ctx=ctx2)
        else:
            job = rustfst_amd.compose_shortest_path_batch_begin(daccs, dt, ctx=ctx2)
            sp_job = dt.shortest_path_begin()
        outs, n_arcs = job.finish()
        sp = sp_job.finish()
        assert_flat_identical(sp.to_flat(), can_flat, f"{order}, rep {rep}: the query")
        for i, e in exp.items():
            assert_flat_identical(outs[i].to_flat(), e, f"{order}, rep {rep}: batch item {i}")
    st = ctx.stats()
    assert st["resident_aborts"] == 0 and st["relax_kernel"] == 2
    ctx.set_resident_share(0)
    assert_flat_identical(dt.shortest_path().to_flat(), can_flat, "whole-device share again")
    assert ctx.stats()["relax_kernel"] == 2


def test_two_half_device_queries_run_at_the_same_time(oracle, monkeypatch):
    """The resident lease of a device has two units (sssp.hip ResidentLease): two contexts set to half the device
    (wfst_ctx_set_resident_share(ctx, 1)) answer two shortest_path queries — different FSTs, different sources — AT THE SAME TIME,
    both with resident launches, neither giving up; a third query queued while both are in flight finds no unit and takes one
    launch per level; a whole-device context finds the lease taken while a half-device query runs.  Every path and every
    distance bit-identical to the canonical oracle, in both enqueue orders, repeatedly."""
    monkeypatch.setenv("WFST_SSSP_MAILBOX", "1")
    ta = synth.make_transducer(300_000, 8, 64, 0.0, seed=31)
    tb = dict(synth.make_transducer(260_000, 9, 64, 0.0, seed=32), start=12_345)
    c1, c2, c3, cw = (rustfst_amd.Context(0) for _ in range(4))
    for c in (c1, c2, c3):
        c.set_resident_share(1)
    da, db = to_device(ta, c1), to_device(tb, c2)
    dc = to_device(ta, c3)
    dw = to_device(tb, cw)
    ca, cb = to_oracle(oracle, ta).shortest_path_canonical(), to_oracle(oracle, tb).shortest_path_canonical()
    for d, c, can in ((da, c1, ca), (db, c2, cb), (dc, c3, ca), (dw, cw, cb)):
        for q in range(3):  # (plan, transpose, predicted batch)
            assert_flat_identical(d.shortest_path().to_flat(), can.to_flat(), f"alone, query {q}")
        assert c.stats()["relax_kernel"] == 2
    for rep in range(8):
        first, second = ((da, db) if rep % 2 == 0 else (db, da))
        j1 = first.shortest_path_begin()
        j2 = second.shortest_path_begin()
        j3 = dc.shortest_path_begin() if rep >= 4 else None  # both units are out: one launch per level
        jw = dw.shortest_path_begin() if rep >= 6 else None  # wants both units
        r1, r2 = j1.finish(), j2.finish()
        assert c1.stats()["relax_kernel"] == 2 and c2.stats()["relax_kernel"] == 2, (rep, c1.stats()["relax_kernel"], c2.stats()["relax_kernel"])
        ra, rb = (r1, r2) if rep % 2 == 0 else (r2, r1)
        assert_flat_identical(ra.to_flat(), ca.to_flat(), f"rep {rep}: first FST")
        assert_flat_identical(rb.to_flat(), cb.to_flat(), f"rep {rep}: second FST")
        if j3 is not None:
            assert_flat_identical(j3.finish().to_flat(), ca.to_flat(), f"rep {rep}: third query")
            assert c3.stats()["relax_kernel"] == 1
        if jw is not None:
            assert_flat_identical(jw.finish().to_flat(), cb.to_flat(), f"rep {rep}: whole-device query")
            assert cw.stats()["relax_kernel"] == 1
    for c in (c1, c2, c3, cw):
        assert c.stats()["resident_aborts"] == 0
    for d, can in ((da, ca), (db, cb)):
        dist, hops = d.shortest_distance(want_hops=True)
        np.testing.assert_array_equal(dist.view(np.uint32), can.distance.view(np.uint32))
        np.testing.assert_array_equal(hops, can.hops)


def test_two_processes_solving_on_one_gpu():
    """Two PROCESSES query the same kind of FST on one GPU at the same time.  A resident launch needs every workgroup on a
    compute unit of its own, so only one process at a time may run one: the lease is an advisory file lock per device
    (ResidentLease), whoever does not get it takes one launch per level for that solve.  Both processes: every result equal
    to their first, no resident launch ever gives up, and each of them ran resident launches."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "tools", "two_process_resident.py"), "600000", "150"]
    procs = [subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for _ in range(2)]
    outs = [p.communicate(timeout=600) for p in procs]
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0 and so.strip().splitlines()[-1].startswith("OK"), so[-1500:] + se[-1500:]
        fields = dict(kv.split("=") for kv in so.strip().splitlines()[-1].split()[1:])
        assert int(fields["aborts"]) == 0 and int(fields["resident"]) > 0, so[-500:]


def test_reference_tie_order_on_acyclic_inputs(oracle):
    """wfst_ctx_set_tie_order(ctx, 1): on acyclic inputs shortest_path returns the path RUSTFST returns when optima tie —
    first strict improver in the topological order of its depth-first visit (auto_queue.rs:23-99, top_order_queue.rs:12-94,
    shortest_path.rs:214-232) — bit-identical to the oracle's reference-order mode on tied inputs (weights on a 1/2 grid
    and integer weights: ties everywhere), on random DAGs in arbitrary state numbering (random permutations), on composed
    lattices with unit-spaced weights, and with the TOP_SORTED / ACYCLIC property bits set.  Inputs on which the
    reference uses another queue (a cycle -> SCC queue; all weights zero / one -> LIFO) have no rule to follow: there the
    call returns the path only when the optimum is UNIQUE (it is then the reference's path AND the canonical one,
    wfst_stats.tied_choices == 0) and is KO "ambiguous optimum" when the canonical oracle counts a tied choice."""
    ctx = rustfst_amd.Context(0)
    ctx.set_tie_order(True)
    rng = np.random.default_rng(8080)
    n_ref = n_tied = n_diff = n_other_unique = n_other_tied = 0
    for k in range(90):
        n = int(rng.integers(2, 120))
        f = random_fst_flat(rng, n, 4, 3, p_eps_i=0.1, p_final=0.25, acyclic=(k % 6 != 5), min_fanout=1,
                            weight_grid=int(rng.choice([2, 1])), max_w=int(rng.choice([2, 3, 5])))
        if k % 2:  # renumber the states at random: the topological order is then not the state order
            perm = rng.permutation(n).astype(np.uint32)
            inv = np.argsort(perm)
            rows, offsets = [], [0]
            for new in range(n):
                old = int(inv[new])
                seg = f["arcs"][f["offsets"][old]:f["offsets"][old + 1]].copy()
                seg["nextstate"] = perm[seg["nextstate"]]
                rows.append(seg)
                offsets.append(offsets[-1] + len(seg))
            f = dict(f, arcs=np.concatenate(rows) if rows else f["arcs"], offsets=np.array(offsets, np.uint32),
                     finals=f["finals"][inv], start=int(perm[f["start"]]) if f["start"] is not None else None)
        if k % 7 == 3 and k % 2 == 0 and k % 6 != 5:
            f = dict(f, props=f["props"] | synth.ACYCLIC)
        o = to_oracle(oracle, f)
        ref = o.shortest_path()  # the reference's order (AutoQueue restatement, approximate ==)
        can = o.shortest_path_canonical()
        if ref.queue_kind in ("top_order", "top_order_scc", "state_order"):
            got = to_device(f, ctx).shortest_path().to_flat()
            n_ref += 1
            n_tied += can.n_tied_choices > 0
            rf, cf = ref.to_flat(), can.to_flat()
            n_diff += not (rf["n_states"] == cf["n_states"] and np.array_equal(rf["arcs"], cf["arcs"]))
            assert_flat_identical(got, rf, f"reference tie order, case {k} ({ref.queue_kind})")
        elif can.n_tied_choices > 0:
            n_other_tied += 1
            with pytest.raises(rustfst_amd.WfstError, match="ambiguous optimum"):
                to_device(f, ctx).shortest_path()
        else:
            n_other_unique += 1
            got = to_device(f, ctx).shortest_path().to_flat()
            assert ctx.stats()["tied_choices"] == 0
            assert_flat_identical(got, can.to_flat(), f"unique optimum, canonical, case {k} ({ref.queue_kind})")
            assert_flat_identical(got, ref.to_flat(), f"unique optimum, the reference's path, case {k} ({ref.queue_kind})")
    # (the cases are not vacuous: optima tie, and the reference's choice differs from the canonical one on some of them)
    assert n_ref >= 45 and n_tied >= 8 and n_diff >= 3, (n_ref, n_tied, n_diff)
    assert n_other_unique >= 3 and n_other_tied >= 3, (n_other_unique, n_other_tied)
    # composed lattices with integer weights (ties along the lattice)
    t = synth.make_transducer(3000, 6, 4, 0.0, seed=12)  # (no input epsilons: the lattices are acyclic)
    t["arcs"]["weight"] = np.round(t["arcs"]["weight"])
    t["finals"] = np.where(np.isfinite(t["finals"]), np.round(t["finals"]), np.inf).astype(np.float32)
    accs = synth.make_acceptors(t, 6, 25, seed0=31)
    dt, ot = to_device(t, ctx), to_oracle(oracle, t)
    for a in accs:
        lat = to_device(a, ctx).compose(dt)
        ref = to_oracle(oracle, a).compose(ot).shortest_path()
        assert ref.queue_kind in ("top_order", "top_order_scc", "state_order")
        assert_flat_identical(lat.shortest_path().to_flat(), ref.to_flat(), "reference tie order on a composed lattice")
    ctx.set_tie_order(False)


def test_tied_choices_are_reported_and_tie_order_1_is_total_on_cyclic_inputs(oracle):
    """SURVEY F6 / shortest_path.rs:214-232: on a cyclic input rustfst's choice among tied optima depends on its dequeue
    history.  The library tells the caller whether that matters: wfst_stats.tied_choices = states of the returned path with
    more than one optimal predecessor (+ 1 for tied final states), counted by the tail kernel's walk over the in-arcs —
    equal to the canonical oracle's count.  Tie order 0 always returns the canonical path; tie order 1 returns it only when
    the count is 0 (then rustfst's path is the same one: compared with the oracle's reference mode) and is KO otherwise.
    Cyclic branching graphs with integer weights (ties likely) and with k/512 weights (ties rare), 70k - 300k arcs."""
    n_unique = n_tied = n_ref_differs = 0
    for case, (n, fan, seed, integer) in enumerate([(9000, 8, 1, True), (9000, 8, 2, False), (40000, 8, 3, True), (40000, 8, 4, False),
                                                    (2000, 40, 5, True), (2000, 40, 6, False), (30000, 3, 7, True), (30000, 3, 8, False)]):
        t = synth.make_transducer(n, fan, 64, 0.0, seed=seed)
        if integer:
            t["arcs"]["weight"] = np.round(t["arcs"]["weight"] / 4.0) + 1.0  # (1, 2, 3, 4: optima tie)
            t["finals"] = np.where(np.isfinite(t["finals"]), np.round(t["finals"]), np.inf).astype(np.float32)
        o = to_oracle(oracle, t)
        can = o.shortest_path_canonical()
        ref = o.shortest_path()
        assert ref.queue_kind not in ("top_order", "top_order_scc", "state_order")  # (a ring backbone: cyclic)
        ctx = rustfst_amd.Context(0)
        d = to_device(t, ctx)
        for q in range(3):  # tie order 0: the canonical path, and from the second query on (transpose cached) the count
            got = d.shortest_path().to_flat()
            assert_flat_identical(got, can.to_flat(), f"case {case} q {q}")
            ties = ctx.stats()["tied_choices"]
            if t["arcs"].shape[0] >= 1 << 18 and q >= 1:
                assert ties == can.n_tied_choices, (case, q, ties, can.n_tied_choices)
            else:
                assert ties in (can.n_tied_choices, rustfst_amd._lib.TIES_UNKNOWN)
        ctx.set_tie_order(True)
        if can.n_tied_choices == 0:
            n_unique += 1
            got = d.shortest_path().to_flat()
            assert ctx.stats()["tied_choices"] == 0
            assert_flat_identical(got, ref.to_flat(), f"case {case}: unique optimum = the reference's path")
        else:
            n_tied += 1
            rf, cf = ref.to_flat(), can.to_flat()
            n_ref_differs += not (rf["n_states"] == cf["n_states"] and np.array_equal(rf["arcs"], cf["arcs"]))
            with pytest.raises(rustfst_amd.WfstError, match="ambiguous optimum"):
                d.shortest_path()
            assert ctx.stats()["tied_choices"] == can.n_tied_choices
        ctx.set_tie_order(False)
    assert n_unique >= 2 and n_tied >= 2, (n_unique, n_tied, n_ref_differs)


def test_handles_outlive_their_context():
    """wfst_ctx_destroy before wfst_fst_destroy (interpreter shutdown destroys in any order; a Rust host may drop a context
    first): a handle shares ownership of the context's memory pool, so its arena and its cached derived data (mailbox
    plan, transpose) are still released into a live pool."""
    import ctypes as C
    from rustfst_amd import _lib
    L = _lib.lib()
    t = synth.make_transducer(70_000, 8, 64, 0.0, seed=1)
    ctx = C.c_void_p()
    _lib.check(L.wfst_ctx_create(0, C.byref(ctx)))
    h = C.c_void_p()
    _lib.check(L.wfst_fst_upload(ctx, t["n_states"], t["start"], t["offsets"].ctypes.data, t["arcs"].ctypes.data,
                                 t["finals"].ctypes.data, t["props"], C.byref(h)))
    outs = []
    for _ in range(3):  # region plan on the first solve, transpose on the second
        o = C.c_void_p()
        _lib.check(L.wfst_shortest_path(ctx, h, None, C.byref(o)))
        outs.append(o)
    _lib.check(L.wfst_ctx_destroy(ctx))
    for o in outs:
        _lib.check(L.wfst_fst_destroy(o))
    _lib.check(L.wfst_fst_destroy(h))
    # and a fresh context still works afterwards
    ctx2 = rustfst_amd.Context(0)
    assert to_device(t, ctx2).shortest_path().num_states > 0


def test_kdelta_gap_on_real_valued_weights(gpu_ctx):
    """The reference relaxes only when the improvement exceeds its approximate == (KDELTA = 1/1024, semiring.rs:159-168,
    shortest_path.rs:226); this engine returns the exact (min,+) fixed point.  On real-valued weights of the BASELINE
    shapes (T and A o T lattices with U[0,10) f32 weights, the reference's HCL o G files) the two path weights must agree
    within north_star's 1e-5; the GPU weight is bit-equal to the CPU restatement with exact == and never above the
    reference-mode weight (tools/kdelta_gap.py: the full table is in DESIGN.md §5)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import kdelta_gap
    rows = kdelta_gap.main(quick=True)
    for name, n, over, gmax in rows:
        if not name.startswith("STRESS"):
            assert over == 0 and gmax <= 1e-5, (name, n, over, gmax)
        else:
            assert gmax <= 200 / 1024.0  # at most one KDELTA per arc of the path


# ------------------------------------------------------------------ n > 1 shortest paths (B4-B6)
def test_nshortest_known_graph(gpu_ctx, oracle):
    """The K2 graph (test_shortest_path.py:5-30) asked for 2 and 3 paths."""
    g = golden("k2_shortest_path.json")
    v = vbuild(g["fst"])
    o = oracle.OracleFst()
    for _ in range(4):
        o.add_state()
    o.set_start(0)
    o.set_final(3, 2.0)
    for s, il, ol, w, ns in g["fst"]["arcs"]:
        o.add_tr(s, il, ol, w, ns)
    for n in (2, 3, 7):
        got = v.to_device().shortest_path(ShortestPathConfig(nshortest=n)).to_flat()
        assert_flat_identical(got, o.shortest_path_n(n).to_flat(), f"K2 graph n={n}")


@pytest.mark.parametrize("lazy", ["0", "1"], ids=["reverse_on_host", "reverse_in_hbm"])
@pytest.mark.parametrize("seed", range(10))
def test_nshortest_random_vs_oracle(gpu_ctx, oracle, seed, lazy, monkeypatch):
    # lazy = 1: the reversed FST stays on the device and the host search fetches the segments it visits (the path
    # large FSTs take); forced here on small ones, where the oracle can check the result
    monkeypatch.setenv("WFST_NBEST_LAZY", lazy)
    rng = np.random.default_rng(700 + seed)
    flat = random_fst_flat(rng, int(rng.integers(3, 60)), 4, 5, p_eps_i=0.1, p_final=0.2, min_fanout=1,
                           acyclic=bool(seed % 2))
    for n in (2, 5):
        exp = to_oracle(oracle, flat).shortest_path_n(n).to_flat()
        got = to_device(flat).shortest_path(ShortestPathConfig(nshortest=n)).to_flat()
        assert_flat_identical(got, exp, f"seed {seed} n={n}")


def test_nshortest_unique_batch_vs_oracle(gpu_ctx, oracle):
    """unique = true over a batch: distances and arrays of all small inputs in one launch, reversal / determinization /
    search on host threads — every result bit-identical to the oracle's and to the single call; inputs without a final
    state or a start state in between; a transducer anywhere in the batch makes the call KO, as the single call would."""
    rng = np.random.default_rng(4400)
    flats = []
    for k in range(24):
        f = random_fst_flat(rng, int(rng.integers(2, 60)), 4, 2 + k % 3, p_eps_i=0.1 * (k % 2), p_final=0.3, min_fanout=1,
                            acyclic=True, weight_grid=4 if k % 2 else 512, max_w=12 if k % 2 else 2560, sort="none")
        f["arcs"]["olabel"] = f["arcs"]["ilabel"]
        f["props"] = 0x0000_0000_0001_0000
        flats.append(f)
    flats[4]["finals"][:] = np.inf
    flats[9]["start"] = None
    ds = [to_device(f) for f in flats]
    cfg = ShortestPathConfig(nshortest=4, unique=True)
    outs = rustfst_amd.shortest_path_batch(ds, cfg)
    for k, (f, d, out) in enumerate(zip(flats, ds, outs)):
        got = out.to_flat()
        assert_flat_identical(got, to_oracle(oracle, f).shortest_path_n(4, unique=True).to_flat(), f"unique batch item {k} vs the oracle")
        assert_flat_identical(got, d.shortest_path(cfg).to_flat(), f"unique batch item {k} vs the single call")
    tr = random_fst_flat(rng, 10, 3, 3, p_final=0.4, acyclic=True, min_fanout=1)  # ilabel != olabel somewhere, no ACCEPTOR bit
    with pytest.raises(rustfst_amd.WfstError, match="expected acceptor"):
        rustfst_amd.shortest_path_batch(ds[:3] + [to_device(tr)], cfg)


@pytest.mark.parametrize("device", ["1", "0"], ids=["wave_kernel", "one_by_one"])
def test_shortest_path_batch_one_best_vs_oracle(gpu_ctx, oracle, device, monkeypatch):
    """wfst_shortest_path_batch with nshortest = 1: small inputs are solved by ONE launch, one wavefront each (keys in LDS,
    the canonical predecessor rule, the walk) — the same FSTs as one shortest_path call each returns and as the oracle's
    canonical path, bit for bit: cyclic and acyclic inputs, coarse weight grids (ties), epsilons, inputs without a final
    state or without a start state, a single state; an input with a negative weight takes the single-FST path."""
    monkeypatch.setenv("WFST_SP1_DEVICE", device)
    rng = np.random.default_rng(8800)
    flats = []
    for k in range(40):
        flats.append(random_fst_flat(rng, int(rng.integers(1, 300)), int(rng.integers(1, 6)), 5, p_eps_i=0.1 * (k % 2), p_final=0.05 + 0.3 * rng.random(),
                                     min_fanout=k % 2, acyclic=bool(k % 3 == 0), weight_grid=1 if k % 4 == 0 else 512, max_w=4 if k % 4 == 0 else 2560))
    flats[3]["finals"][:] = np.inf  # no final state: the empty FST
    flats[5]["start"] = None
    flats[7] = synth.linear_acceptor_flat([4])
    neg = random_fst_flat(rng, 30, 3, 4, p_final=0.3, acyclic=True, min_fanout=1)
    neg["arcs"]["weight"][0] = np.float32(-1.5)
    flats.append(neg)
    ds = [to_device(f) for f in flats]
    outs = rustfst_amd.shortest_path_batch(ds, ShortestPathConfig(nshortest=1))
    assert len(outs) == len(flats)
    for k, (f, d, out) in enumerate(zip(flats, ds, outs)):
        got = out.to_flat()
        assert_flat_identical(got, d.shortest_path().to_flat(), f"batch item {k} vs the single call")
        if k < len(flats) - 1:  # (the canonical oracle is defined for non-negative weights)
            assert_flat_identical(got, to_oracle(oracle, f).shortest_path_canonical().to_flat(), f"batch item {k} vs the oracle")


@pytest.mark.parametrize("seed", range(12))
def test_nshortest_unique_vs_oracle(gpu_ctx, oracle, seed):
    """nshortest > 1 with unique = true (shortest_path.rs:157-165): distances and reverse() on the GPU, determinization of the
    reversed acceptor and the search on the host — bit-identical to the oracle's restatement of that branch (both keep a
    weighted subset in ascending state order where the reference's order is unspecified), single call and batch call."""
    rng = np.random.default_rng(4300 + seed)
    flat = random_fst_flat(rng, int(rng.integers(3, 40)), 4, 2 + seed % 3, p_eps_i=0.1 * (seed % 2), p_final=0.3, min_fanout=1,
                           acyclic=True, weight_grid=4 if seed % 2 else 512, max_w=12 if seed % 2 else 2560, sort="none")
    flat["arcs"]["olabel"] = flat["arcs"]["ilabel"]
    flat["props"] = 0x0000_0000_0001_0000  # ACCEPTOR
    d, o = to_device(flat), to_oracle(oracle, flat)
    for n in (2, 5, 20):
        exp = o.shortest_path_n(n, unique=True).to_flat()
        got = d.shortest_path(ShortestPathConfig(nshortest=n, unique=True)).to_flat()
        assert_flat_identical(got, exp, f"unique, seed {seed} n={n}")
    outs = rustfst_amd.shortest_path_batch([d, d], ShortestPathConfig(nshortest=5, unique=True))
    for out in outs:
        assert_flat_identical(out.to_flat(), o.shortest_path_n(5, unique=True).to_flat(), f"unique batch, seed {seed}")


@pytest.mark.parametrize("device", ["1", "0", "tiny_tree"])
def test_nshortest_batch_wave_kernel_vs_oracle(gpu_ctx, oracle, device, monkeypatch):
    """wfst_shortest_path_batch with nshortest > 1: the one-wave-per-input kernel (distances, reverse, the reference's heap
    search, connect) against the oracle's n_shortest_path on random cyclic / acyclic FSTs with epsilons, ties (integer
    weights) and unreachable finals, on composed lattices (the configs[4] shape) and on degenerate inputs; the host search
    (device = 0) and the fall-back of inputs whose search tree outgrows the kernel's arena (tiny_tree) give the same FSTs."""
    if device == "tiny_tree":
        monkeypatch.setenv("WFST_NBEST_TREE", "40")
    else:
        monkeypatch.setenv("WFST_NBEST_DEVICE", device)
    rng = np.random.default_rng(4711)
    flats = []
    for k in range(40):
        flats.append(random_fst_flat(rng, int(rng.integers(1, 80)), 4, 5, p_eps_i=0.1, p_final=0.2, min_fanout=int(k % 2),
                                     acyclic=bool(k % 3 == 0), weight_grid=int(rng.choice([512, 1])), max_w=6))
    t = synth.make_transducer(20_000, 8, 64, 0.02, seed=5)
    ot = to_oracle(oracle, t)
    accs = synth.make_acceptors(t, 6, 40, seed0=1000)
    dt = to_device(t)
    lattices = [to_device(a).compose(dt) for a in accs]
    flats += [d.to_flat() for d in lattices]
    empty = dict(n_states=0, start=None, offsets=np.zeros(1, np.uint32), arcs=np.zeros(0, rustfst_amd.TR_DTYPE),
                 finals=np.zeros(0, np.float32), props=0)
    flats.append(empty)
    devs = [to_device(f) for f in flats]
    for n in (2, 10):
        got = rustfst_amd.shortest_path_batch(devs, ShortestPathConfig(nshortest=n))
        n_dev = int(rustfst_amd.default_context().stats()["nbest_device_problems"])
        if device == "1":
            # the routing rules and the search's tree growth, restated in small_path_cases: every input but the empty
            # one is offered (one without a reachable final state is answered by the kernel too) and none outgrows T = 2048
            want = predict_nbest(flats, n)
            assert want["nbest_in_kernel"] == len(flats) - 1 and want["nbest_tree_full"] == 0
            assert n_dev == want["nbest_in_kernel"], n_dev
            assert rustfst_amd.default_context().small_path_stats()["nbest_tree_capacity"] == want["nbest_tree_capacity"] == 2048
        elif device == "0":
            assert n_dev == 0
        for i, (f, g) in enumerate(zip(flats, got)):
            exp = to_oracle(oracle, f).shortest_path_n(n).to_flat()
            assert_flat_identical(g.to_flat(), exp, f"n-best batch ({device}) input {i} n={n}")
    # n = 1 and n = 0 through the same call
    one = rustfst_amd.shortest_path_batch(devs[:5], ShortestPathConfig(nshortest=1))
    for f, g in zip(flats[:5], one):
        assert_flat_identical(g.to_flat(), to_oracle(oracle, f).shortest_path_canonical().to_flat(), "batch n=1")


def test_k13_nshortest_hand_traced_known_answers(gpu_ctx):
    """n = 2, 3 on the K2 graph against the answers traced by hand through the reference's source
    (tests/golden/K13_DERIVATION.md, shortest_path.rs:409-518): the tie between 0-2-3 and 0-1-1-3 resolved as the
    reference's heap resolves it — through the single call (host search) and through the batch call (wave kernel)."""
    g = golden("k13_nshortest_k2.json")
    d = vbuild(g["fst"]).to_device()
    for n, key in ((2, "n2"), (3, "n3")):
        flat_matches_spec(d.shortest_path(ShortestPathConfig(nshortest=n)).to_flat(), g[key])
        both = rustfst_amd.shortest_path_batch([d, d], ShortestPathConfig(nshortest=n))
        assert int(rustfst_amd.default_context().stats()["nbest_device_problems"]) == 2
        for o in both:
            flat_matches_spec(o.to_flat(), g[key])


@pytest.mark.parametrize("seed", range(8))
def test_nshortest_host_search_vs_wave_kernel_vs_brute_force(gpu_ctx, seed, monkeypatch):
    """Evidence for the n-best code that does not pass through the oracle: the host heap search (nshortest.hip, what large
    inputs take) and the wave kernel (nbest_batch.hip: an independent implementation of shortest_path.rs:409-518 on the
    device) return bit-identical FSTs on the same inputs — acyclic and cyclic, with ties —, and on the acyclic ones both
    hold exactly the n lightest paths of an exhaustive enumeration written in Python (tests/helpers.py)."""
    from helpers import check_nbest_against_brute_force
    rng = np.random.default_rng(5200 + seed)
    flats = []
    for k in range(10):
        flats.append(random_fst_flat(rng, int(rng.integers(3, 13 if k < 6 else 50)), 3, 4, p_eps_i=0.15, p_final=0.35, min_fanout=1,
                                     acyclic=k < 6, weight_grid=4 if k % 2 else 512, max_w=12 if k % 2 else 2560))
    devs = [to_device(f) for f in flats]
    ctx = rustfst_amd.default_context()
    for n in (2, 5):
        cfg = ShortestPathConfig(nshortest=n)
        monkeypatch.setenv("WFST_NBEST_DEVICE", "1")
        wave = [o.to_flat() for o in rustfst_amd.shortest_path_batch(devs, cfg)]
        assert int(ctx.stats()["nbest_device_problems"]) == len(flats)
        monkeypatch.setenv("WFST_NBEST_DEVICE", "0")
        host = [o.to_flat() for o in rustfst_amd.shortest_path_batch(devs, cfg)]
        assert int(ctx.stats()["nbest_device_problems"]) == 0
        for k, (f, w, h) in enumerate(zip(flats, wave, host)):
            assert_flat_identical(w, h, f"seed {seed} input {k} n={n}: wave kernel vs host search")
            if k < 6:
                check_nbest_against_brute_force(w, f, n, f"seed {seed} input {k} n={n}")


@pytest.mark.parametrize("lazy", ["0", "1"], ids=["reverse_on_host", "reverse_in_hbm"])
def test_nshortest_on_transducer_and_lattice(gpu_ctx, oracle, lazy, monkeypatch):
    monkeypatch.setenv("WFST_NBEST_LAZY", lazy)
    t = synth.make_transducer(20_000, 8, 64, 0.02, seed=5)
    accs = synth.make_acceptors(t, 2, 40, seed0=1000)
    dt, ot = to_device(t), to_oracle(oracle, t)
    exp = ot.shortest_path_n(10).to_flat()
    got = dt.shortest_path(ShortestPathConfig(nshortest=10)).to_flat()
    assert_flat_identical(got, exp, "T n=10")
    assert exp["n_states"] > 10
    # BASELINE config 5 shape (without look-ahead): compose then 10 shortest paths
    dc = to_device(accs[0]).compose(dt)
    oc = to_oracle(oracle, accs[0]).compose(ot)
    assert_flat_identical(dc.shortest_path(ShortestPathConfig(nshortest=10)).to_flat(), oc.shortest_path_n(10).to_flat(),
                          "lattice n=10")
    # reverse distance bookkeeping: asking twice reuses the cached transpose and gives the same answer
    assert_flat_identical(dt.shortest_path(ShortestPathConfig(nshortest=10)).to_flat(), exp, "T n=10 again")


def test_pack_paths_matches_python_packing(gpu_ctx, oracle):
    from rustfst_amd import dist as wdist
    t = synth.make_transducer(3000, 8, 32, 0.0, seed=9)
    accs = synth.make_acceptors(t, 5, 20, seed0=50)
    accs.append(synth.linear_acceptor_flat([1, 2, 3]))
    outs, _ = rustfst_amd.compose_shortest_path_batch(rustfst_amd.DeviceFst.upload_many(accs), to_device(t))
    a = wdist.pack_device_paths(outs, 28)
    b = wdist.pack_paths([o.to_flat() for o in outs], 28)
    np.testing.assert_array_equal(a, b)
    back = wdist.unpack_paths(a)
    for o, u in zip(outs, back):
        f = o.to_flat()
        assert f["n_states"] == u["n_states"] and np.array_equal(f["arcs"], u["arcs"])
    with pytest.raises(rustfst_amd.WfstError, match="longer"):
        wdist.pack_device_paths(outs, 3)


# ------------------------------------------------------------------ §8(f) N3: const-format loader; N2: device tr_sort
@pytest.mark.parametrize("name", ["fst_012_hcl.fst", "fst_014_hcl.fst", "fst_012_gp.fst", "fst_014_g.fst",
                                  "fst_020_patterns_fst.fst"])
def test_openfst_loader_const_and_vector(gpu_ctx, oracle, name):
    data = open(os.path.join(GOLDEN, name), "rb").read()
    d = rustfst_amd.DeviceFst.from_bytes(data)
    o = oracle.OracleFst.load(data)
    assert_flat_identical(d.to_flat(), o.to_flat(), name)
    assert d.to_bytes() == o.store()
    assert d.to_bytes("const") == o.store("const")
    again = rustfst_amd.DeviceFst.from_bytes(d.to_bytes("const"))
    assert_flat_identical(again.to_flat(), o.to_flat(), name + " via const v2")


def _unsorted_flat(rng, n_states, max_fanout, sigma, hub_degrees=(), acceptor=False):
    f = random_fst_flat(rng, n_states, max_fanout, sigma, p_eps_i=0.15, p_eps_o=0.15, sort="none")
    # re-build with a few hub states of prescribed degree (exercise the 17..256 rank path and the rocPRIM path)
    offsets = [0]
    rows = []
    for s in range(n_states):
        a = f["arcs"][f["offsets"][s]:f["offsets"][s + 1]]
        if s < len(hub_degrees):
            k = hub_degrees[s]
            a = np.zeros(k, dtype=f["arcs"].dtype)
            a["ilabel"] = rng.integers(0, sigma + 1, k)
            a["olabel"] = rng.integers(0, sigma + 1, k)
            a["weight"] = rng.integers(0, 2560, k) / 512.0
            a["nextstate"] = rng.integers(0, n_states, k)
        rows.append(a)
        offsets.append(offsets[-1] + len(a))
    arcs = np.concatenate(rows) if rows else f["arcs"]
    props = 0
    if acceptor:
        arcs["olabel"] = arcs["ilabel"]
        props |= synth.ACCEPTOR
    return dict(n_states=n_states, start=0, offsets=np.array(offsets, dtype=np.uint32), arcs=arcs, finals=f["finals"],
                props=props)


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("ilabel_cmp", [True, False])
def test_tr_sort_matches_oracle(gpu_ctx, oracle, seed, ilabel_cmp):
    rng = np.random.default_rng(900 + seed)
    hubs = [(), (17, 64, 255), (256, 257, 1000), (5000, 3), (16, 15, 1), (300,)][seed]
    flat = _unsorted_flat(rng, int(rng.integers(6, 400)), 14, int(rng.integers(2, 40)), hubs, acceptor=(seed == 4))
    d = to_device(flat)
    o = to_oracle(oracle, flat)
    d.tr_sort(ilabel_cmp)
    o.tr_sort(by_olabel=not ilabel_cmp)
    assert_flat_identical(d.to_flat(), o.to_flat(), f"tr_sort seed {seed}")
    # the derived {weight,next} array was rebuilt too: distances over the sorted arcs agree with the oracle
    np.testing.assert_allclose(d.shortest_distance(), o.shortest_path_canonical().distance, rtol=0, atol=1e-5)
    before = d.to_flat()
    d.tr_sort(ilabel_cmp)  # idempotent
    assert_flat_identical(d.to_flat(), before, "tr_sort twice")


def test_tr_sort_large_is_sorted_and_stable(gpu_ctx):
    """BASELINE-sized T (1M states / ~10M arcs) sorted by olabel: size-independent properties — per-state
    non-decreasing olabels, stability (ties keep their ilabel-sorted input order), multiset preserved."""
    t = synth.make_transducer(1_000_000, 10, 50_000, 0.1, seed=42)
    d = to_device(t)
    d.tr_sort(False)
    out = d.to_flat()
    assert out["props"] & synth.O_LABEL_SORTED and not out["props"] & synth.I_LABEL_SORTED
    a, off = out["arcs"], out["offsets"].astype(np.int64)
    state_of = np.repeat(np.arange(t["n_states"]), np.diff(off))
    same = state_of[1:] == state_of[:-1]
    ol = a["olabel"].astype(np.int64)
    assert np.all(ol[1:][same] >= ol[:-1][same])
    tie = same & (ol[1:] == ol[:-1])
    il = a["ilabel"].astype(np.int64)
    assert np.all(il[1:][tie] >= il[:-1][tie])  # input was ilabel-sorted => stable output keeps that order on ties
    ref = t["arcs"].copy()
    order = np.lexsort((np.arange(len(ref)), ref["olabel"], np.repeat(np.arange(t["n_states"]), np.diff(off))))
    np.testing.assert_array_equal(a.view(np.uint32), ref[order].view(np.uint32))
    d.tr_sort(True)  # and back by ilabel: ties now keep the olabel-sorted order
    order2 = np.lexsort((np.arange(len(a)), a["ilabel"], state_of))
    back = d.to_flat()
    np.testing.assert_array_equal(back["arcs"].view(np.uint32), a[order2].view(np.uint32))
    assert back["props"] & synth.I_LABEL_SORTED and not back["props"] & synth.O_LABEL_SORTED


@pytest.mark.parametrize("hcl,g", [("fst_014_hcl.fst", "fst_014_g.fst"), ("fst_012_hcl.fst", "fst_012_gp.fst")])
def test_hcl_compose_g(gpu_ctx, oracle, hcl, g):
    """HCL (const file) o G (vector file), the pairing of the reference's fst_014.h / fst_012.h, with the
    arc sorting done on the device."""
    da, db = (open(os.path.join(GOLDEN, n), "rb").read() for n in (hcl, g))
    a, b = rustfst_amd.DeviceFst.from_bytes(da), rustfst_amd.DeviceFst.from_bytes(db)
    oa, ob = oracle.OracleFst.load(da), oracle.OracleFst.load(db)
    a.tr_sort(False), b.tr_sort(True)
    oa.tr_sort(by_olabel=True), ob.tr_sort(by_olabel=False)
    for connect in (True, False):
        c = a.compose(b, ComposeConfig(connect=connect))
        oc = oa.compose(ob, connect=connect)
        assert_flat_identical(c.to_flat(), oc.to_flat(), f"{hcl} o {g} connect={connect}")
    sp = c.shortest_path()
    assert_flat_identical(sp.to_flat(), oc.shortest_path_canonical().to_flat(), "shortest path of HCL o G")
    outs, _ = rustfst_amd.compose_shortest_path_batch([a], b)
    assert_flat_identical(outs[0].to_flat(), oa.compose(ob).shortest_path_canonical().to_flat(), "fused HCL o G")


def test_async_batch_overlaps_with_shortest_path(gpu_ctx, oracle):
    """begin/end form of the fused batch on a second context, with shortest_path(T) issued in between on the
    first: both results are bit-identical to the synchronous calls and to the oracle."""
    torch = pytest.importorskip("torch")
    t = synth.make_transducer(20000, 6, 32, 0.0, seed=11)
    accs = synth.make_acceptors(t, 24, 60, seed0=500)
    ctx = rustfst_amd.default_context()
    s2 = torch.cuda.Stream()
    ctx2 = rustfst_amd.Context(0, stream=s2.cuda_stream)
    dt = to_device(t, ctx)
    daccs = rustfst_amd.DeviceFst.upload_many(accs, ctx2)
    sync_outs, sync_arcs = rustfst_amd.compose_shortest_path_batch(daccs, dt, ctx=ctx2)
    sync_sp = dt.shortest_path().to_flat()
    for _ in range(3):
        job = rustfst_amd.compose_shortest_path_batch_begin(daccs, dt, ctx=ctx2)
        with pytest.raises(rustfst_amd.WfstError, match="in flight"):
            rustfst_amd.compose_shortest_path_batch_begin(daccs, dt, ctx=ctx2)
        sp = dt.shortest_path()
        outs, n_arcs = job.finish()
        assert n_arcs == sync_arcs
        assert_flat_identical(sp.to_flat(), sync_sp, "shortest_path(T) while a batch is in flight")
        for a, b in zip(outs, sync_outs):
            assert_flat_identical(a.to_flat(), b.to_flat(), "async batch vs sync batch")
    ot = to_oracle(oracle, t)
    for i in (0, 7, 23):
        ref = to_oracle(oracle, accs[i]).compose(ot).shortest_path_canonical().to_flat()
        assert_flat_identical(outs[i].to_flat(), ref, f"async batch problem {i}")
    with pytest.raises(rustfst_amd.WfstError):
        job.finish()
    del rustfst_amd.compose_shortest_path_batch_begin(daccs, dt, ctx=ctx2)._keep  # abandoned job is reclaimed


@pytest.mark.parametrize("seed", range(3))
def test_shortest_path_repeated_queries_use_transpose(gpu_ctx, oracle, seed):
    """From the second query on a large FST the backtrace runs over the cached transpose instead of the parent
    pass: every query returns the oracle's canonical path bit for bit; tr_sort invalidates the cache."""
    t = synth.make_transducer(40000 + 5000 * seed, 8, 64, 0.05 * seed, seed=300 + seed)
    assert t["offsets"][-1] >= 1 << 18
    d = to_device(t)
    ref = to_oracle(oracle, t).shortest_path_canonical().to_flat()
    for q in range(4):
        assert_flat_identical(d.shortest_path().to_flat(), ref, f"query {q}")
    d.tr_sort(False)  # olabel order: arc positions change, so must the transpose
    o = to_oracle(oracle, t)
    o.tr_sort(by_olabel=True)
    ref2 = o.shortest_path_canonical().to_flat()
    for q in range(3):
        assert_flat_identical(d.shortest_path().to_flat(), ref2, f"after tr_sort, query {q}")


def _ragged_transducer(n, max_deg, seed):
    """synth.make_transducer's arcs with a random out-degree per state in [0, max_deg]: rows of no arcs, of fewer than 16, of
    more than 16 and of more than 32 (the 16-lane groups of the transpose kernels take a row 16 arcs at a time)."""
    t = synth.make_transducer(n, max_deg, 64, 0.0, seed=seed)
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, max_deg + 1, n).astype(np.uint32)
    deg[0] = max_deg
    keep = np.tile(np.arange(max_deg, dtype=np.uint32), n) < np.repeat(deg, max_deg)
    offsets = np.zeros(n + 1, np.uint32)
    offsets[1:] = np.cumsum(deg, dtype=np.uint64).astype(np.uint32)
    props = int(t["props"]) & ~(synth.ACCESSIBLE | synth.INITIAL_CYCLIC)  # (no longer known)
    arcs = np.ascontiguousarray(t["arcs"][keep])
    arcs["weight"] = np.floor(arcs["weight"] / np.float32(2.5)) + np.float32(1.0)  # 1..4: many in-arcs of a state are tight at once
    return dict(n_states=n, start=0, offsets=offsets, arcs=arcs, finals=t["finals"], props=props)


@pytest.mark.parametrize("n,max_deg,picks", [(40_000, 40, 6), (1_010_000, 18, 2)], ids=["4096_state_blocks", "8192_state_blocks"])
def test_transpose_through_the_plan_on_ragged_rows(oracle, monkeypatch, n, max_deg, picks):
    """rev_bucket_kernel / rev_place_kernel (sssp.hip) on rows of every length, with both block sizes of the mailbox plan:
    handles with ONE final state each (a different walk through the transpose per handle), the second and third query of
    each — the ones that walk the in-arcs — bit-identical to the canonical oracle, with its count of tied choices: with weights
    1..4 most states have several tight in-arcs, so both the predecessor chosen (the smallest (source, position) among them)
    and the count depend on every in-arc record of the states on the walk."""
    monkeypatch.setenv("WFST_SSSP_MAILBOX", "1")
    monkeypatch.setenv("WFST_SSSP_TRANSPOSE_PLAN", "1")
    ctx = rustfst_amd.Context(0)
    t = _ragged_transducer(n, max_deg, seed=77)
    assert len(t["arcs"]) >= 1 << 18 and int(np.diff(t["offsets"].astype(np.int64)).max()) > 16
    dist = to_device(t, ctx).shortest_distance()
    reach = np.flatnonzero(np.isfinite(dist))
    assert len(reach) > n // 2
    far = reach[np.argsort(dist[reach], kind="stable")[-(len(reach) // 50):]]  # the farthest 2 %: the longest walks, most ties
    rng = np.random.default_rng(n)
    tied = 0
    for pick in rng.choice(far, size=picks, replace=False):
        finals = np.full(n, np.inf, np.float32)
        finals[pick] = np.float32(0.25)
        tp = dict(t, finals=finals)
        can = to_oracle(oracle, tp).shortest_path_canonical()
        assert can.to_flat()["n_states"] > 1
        d = to_device(tp, ctx)
        for q in range(3):  # parent pass; the query that builds the transpose; the predicted batch with the one-launch tail
            assert_flat_identical(d.shortest_path().to_flat(), can.to_flat(), f"final state {pick}, query {q + 1}")
            if q:
                assert ctx.stats()["tied_choices"] == can.n_tied_choices
        tied += can.n_tied_choices
    assert tied > 0


def test_resident_rounds_on_heavy_tailed_out_degrees(oracle, monkeypatch):
    """A decoding-graph-like degree profile: most states have 2 arcs, one in a hundred has 300 - 600.  The plan's rule for the
    lanes per listed state (mbox_plan, sssp.hip) must not pick a narrow lane group from the MANY short rows when most ARCS sit in
    the few long ones; whatever it picks, the long-row pass of rs_expand_round does most of the work here.  Distances, hop counts
    and the path bit-identical to the canonical oracle under the resident launches, also with the narrowest group forced."""
    monkeypatch.setenv("WFST_SSSP_MAILBOX", "1")
    n, max_deg = 24_000, 600
    t = synth.make_transducer(n, max_deg, 64, 0.0, seed=13)
    rng = np.random.default_rng(13)
    deg = np.full(n, 2, np.uint32)
    heavy = rng.choice(n, n // 100, replace=False)
    deg[heavy] = rng.integers(300, max_deg + 1, len(heavy)).astype(np.uint32)
    deg[0] = max_deg
    keep = np.tile(np.arange(max_deg, dtype=np.uint32), n) < np.repeat(deg, max_deg)
    offsets = np.zeros(n + 1, np.uint32)
    offsets[1:] = np.cumsum(deg, dtype=np.uint64).astype(np.uint32)
    arcs = np.ascontiguousarray(t["arcs"][keep])
    props = int(t["props"]) & ~(synth.ACCESSIBLE | synth.INITIAL_CYCLIC)
    t = dict(n_states=n, start=0, offsets=offsets, arcs=arcs, finals=t["finals"], props=props)
    assert len(arcs) > 100_000 and deg[heavy].sum() > len(arcs) // 2
    can = to_oracle(oracle, t).shortest_path_canonical()
    assert np.isfinite(can.distance).sum() > n // 2
    for lps in (None, "2"):
        if lps is not None:
            monkeypatch.setenv("WFST_SSSP_LPS", lps)
        ctx = rustfst_amd.Context(0)
        d = to_device(t, ctx)
        for q in range(3):
            dist, hops = d.shortest_distance(want_hops=True)
            assert ctx.stats()["relax_kernel"] == 2 and ctx.stats()["resident_aborts"] == 0
            np.testing.assert_array_equal(dist.view(np.uint32), can.distance.view(np.uint32))
            np.testing.assert_array_equal(hops, can.hops)
            assert_flat_identical(d.shortest_path().to_flat(), can.to_flat(), f"lanes {lps}, query {q}")


def test_set_start_on_a_resident_handle_queries_from_any_source(oracle, monkeypatch):
    """wfst_fst_set_start (MutableFst::set_start, mutable_fst.rs:35-44): one resident FST, a shortest-path query from each of
    several sources — every result bit-identical to the canonical oracle's on an FST built with that start state, the
    property word as the reference updates it, the derived data of the handle (region plan, transpose) reused; a state beyond
    the FST is KO with the reference's message.  The launch pattern differs from source to source: solves that outrun the
    prediction taken from the previous source are continued (no result depends on the prediction)."""
    monkeypatch.setenv("WFST_SSSP_MAILBOX", "1")
    ctx = rustfst_amd.Context(0)
    t = synth.make_transducer(200_000, 8, 64, 0.0, seed=23)
    d = to_device(t, ctx)
    for q in range(3):
        d.shortest_path()  # (plan, transpose and the predicted batch exist before the start state moves)
    with pytest.raises(Exception, match="doesn't exist"):
        d.set_start(200_000)
    rng = np.random.default_rng(4)
    for src in [int(x) for x in rng.integers(0, 200_000, 5)] + [0, 199_999]:
        d.set_start(src)
        ts = dict(t, start=src)
        o = to_oracle(oracle, ts)
        can = o.shortest_path_canonical()
        for q in range(2):
            got = d.shortest_path()
            assert ctx.stats()["relax_kernel"] == 2
            assert_flat_identical(got.to_flat(), can.to_flat(), f"source {src}, query {q}")
        dist, hops = d.shortest_distance(want_hops=True)
        np.testing.assert_array_equal(dist.view(np.uint32), can.distance.view(np.uint32))
        np.testing.assert_array_equal(hops, can.hops)
        # set_start_properties (mutate_properties.rs:7-13) keeps everything but what is said relative to the start state
        assert d.properties == int(t["props"]) & ~int(synth.INITIAL_CYCLIC | synth.ACCESSIBLE)


@pytest.mark.parametrize("lps,umax", [("2", "4"), ("3", "2"), ("5", "4"), ("6", "2"), ("7", "4"), ("8", "2"), (None, None)],
                         ids=["2x4", "3x2", "5x4", "6x2", "7x4", "8x2", "from_the_degrees"])
def test_resident_rounds_with_every_lane_group_size(oracle, monkeypatch, lps, umax):
    """rs_expand_round (sssp_resident.h) with 2 .. 8 lanes per listed state and 2 or 4 states per lane group, on rows of 0 .. 24
    arcs: with few lanes most rows overflow the first pass (2 x lps arcs) and are finished by the long-row pass, with many
    lanes some lanes of a group have no arc, and a lane's second arc may lie beyond its row.  Distances, hop counts and the
    path bit-identical to the canonical oracle under the resident launches, twice per handle (the second solve runs as one
    predicted batch), and — last case — with the group size the plan derives from the out-degrees itself (mbox_degree_kernel)."""
    monkeypatch.setenv("WFST_SSSP_MAILBOX", "1")
    if lps is not None:
        monkeypatch.setenv("WFST_SSSP_LPS", lps)
        monkeypatch.setenv("WFST_SSSP_UMAX", umax)
    ctx = rustfst_amd.Context(0)
    t = _ragged_transducer(120_000, 24, seed=5)
    rng = np.random.default_rng(9)
    t["arcs"]["weight"] = (rng.integers(0, 2048, len(t["arcs"])).astype(np.float32) / np.float32(256.0)).astype(np.float32)
    can = to_oracle(oracle, t).shortest_path_canonical()
    assert np.isfinite(can.distance).sum() > 50_000
    d = to_device(t, ctx)
    for q in range(3):
        dist, hops = d.shortest_distance(want_hops=True)
        assert ctx.stats()["relax_kernel"] == 2 and ctx.stats()["resident_aborts"] == 0
        np.testing.assert_array_equal(dist.view(np.uint32), can.distance.view(np.uint32))
        np.testing.assert_array_equal(hops, can.hops)
        assert_flat_identical(d.shortest_path().to_flat(), can.to_flat(), f"lanes {lps}, states per group {umax}, query {q}")


@pytest.mark.parametrize("plan", ["1", "0"], ids=["through_the_mailbox_plan", "two_atomic_passes"])
def test_transpose_is_built_in_the_second_query(oracle, monkeypatch, plan):
    """The transpose for the backtrace is built inside the SECOND shortest_path query of a large FST (sssp.hip: reverse_csr):
    through the mailbox plan's regions (rev_bucket_kernel / rev_place_kernel: no global atomic) or, without a plan, by the two
    atomic passes — the same walks either way: every path bit-identical to the canonical oracle, the tied choices counted
    from the second query on; a second context, a tr_sort in between, an abandoned handle."""
    monkeypatch.setenv("WFST_SSSP_TRANSPOSE_PLAN", plan)
    unknown = rustfst_amd._lib.TIES_UNKNOWN
    ctx = rustfst_amd.Context(0)
    t = synth.make_transducer(300_000, 8, 64, 0.0, seed=41)
    o = to_oracle(oracle, t)
    can = o.shortest_path_canonical()
    d = to_device(t, ctx)
    assert_flat_identical(d.shortest_path().to_flat(), can.to_flat(), "first query (parent pass)")
    assert ctx.stats()["tied_choices"] == unknown
    for q in range(3):
        assert_flat_identical(d.shortest_path().to_flat(), can.to_flat(), f"query {q + 2}")
        assert ctx.stats()["tied_choices"] == can.n_tied_choices
    # a second context right behind a fresh handle's first query
    d2 = to_device(t, ctx)
    ctx_b = rustfst_amd.Context(0)
    import ctypes as C
    from rustfst_amd import _lib
    first = d2.shortest_path().to_flat()
    out = C.c_void_p()
    _lib.check(_lib.lib().wfst_shortest_path(ctx_b._h, d2._h, ShortestPathConfig(nshortest=1)._c(), C.byref(out)), "wfst_shortest_path")
    got = rustfst_amd.DeviceFst(out, ctx_b).to_flat()
    assert_flat_identical(first, can.to_flat(), "fresh handle, first query")
    assert_flat_identical(got, can.to_flat(), "fresh handle, second query from another context")
    assert ctx_b.stats()["tied_choices"] == can.n_tied_choices
    # tr_sort after the transpose exists: it is dropped, the next one is built for the new order
    d3 = to_device(t, ctx)
    d3.shortest_path()
    d3.shortest_path()
    d3.tr_sort(False)
    o.tr_sort(by_olabel=True)
    ref3 = o.shortest_path_canonical().to_flat()
    for q in range(3):
        assert_flat_identical(d3.shortest_path().to_flat(), ref3, f"after tr_sort, query {q}")
    d4 = to_device(t, ctx)  # a handle dropped right after the query that built its transpose
    d4.shortest_path()
    d4.shortest_path()
    del d4


@pytest.mark.parametrize("split", [False, True])
def test_shortest_path_tail_in_one_launch(gpu_ctx, oracle, monkeypatch, split):
    """Repeated queries end in ONE launch (sssp_tail_kernel: final-state search by 128 workgroups, the last one walks back
    over the transpose and writes the result header into pinned memory) or, with WFST_SSSP_SPLIT_TAIL, in the three
    kernels + copy of round 1: same FSTs — with a path, without any reachable final state, and with a path longer than
    the pinned buffer (a 270 k-state chain: the walk gives up and the parent pass takes over)."""
    if split:
        monkeypatch.setenv("WFST_SSSP_SPLIT_TAIL", "1")
    t = synth.make_transducer(50000, 8, 64, 0.05, seed=611)
    cases = [("path", t)]
    nofinal = dict(t)
    nofinal["finals"] = np.full_like(t["finals"], np.inf)
    cases.append(("no final state", nofinal))
    n = 270_000  # one arc per state: >= 2^18 arcs, so the second query builds the transpose; 270 k hops
    arcs = np.zeros(n - 1, dtype=t["arcs"].dtype)
    arcs["ilabel"] = arcs["olabel"] = 1 + (np.arange(n - 1) % 5)
    arcs["weight"] = ((np.arange(n - 1) % 7) / 4.0).astype(np.float32)
    arcs["nextstate"] = np.arange(1, n, dtype=np.uint32)
    fin = np.full(n, np.inf, dtype=np.float32)
    fin[-1] = 0.5
    chain = dict(n_states=n, start=0, offsets=np.concatenate([np.arange(n, dtype=np.uint32), [n - 1]]).astype(np.uint32), arcs=arcs,
                 finals=fin, props=0)
    cases.append(("long chain", chain))
    for name, f in cases:
        d = to_device(f)
        ref = to_oracle(oracle, f).shortest_path_canonical().to_flat()
        for q in range(3):
            assert_flat_identical(d.shortest_path().to_flat(), ref, f"{name}, query {q}, split={split}", check_props=(name != "long chain"))


def test_chain_timing_of_repeated_queries(oracle):
    """wfst_ctx_set_profiling(ctx, 2): the pre-queued sweeps of a repeated query are timed between two events on the
    solve's stream (what bench.py's roofline object uses); results are unchanged, the first query of a handle (no
    prediction yet) reports no chain, later ones report their sweep count and a plausible time."""
    ctx = rustfst_amd.Context(0)
    t = synth.make_transducer(80_000, 8, 64, 0.0, seed=91)
    d = to_device(t, ctx)
    ref = to_oracle(oracle, t).shortest_path_canonical().to_flat()
    ctx.set_profiling(2)
    seen = []
    for q in range(4):
        assert_flat_identical(d.shortest_path().to_flat(), ref, f"chain-timed query {q}")
        st = ctx.stats()
        seen.append((st["relax_launches"], st["relax_ms"]))
    ctx.set_profiling(0)
    assert seen[0][0] == 0  # nothing to predict from
    # (a repeated query queues the launches the last one needed plus one: the mailbox schedule is not exactly repeatable)
    assert seen[-1][0] in (ctx.stats()["sweeps"], ctx.stats()["sweeps"] + 1) and 0.0 < seen[-1][1] < 50.0, seen
    assert_flat_identical(d.shortest_path().to_flat(), ref, "after chain timing")


def test_async_shortest_path_matches_sync(gpu_ctx, oracle, monkeypatch):
    """wfst_shortest_path_begin/_end: same FST as the synchronous call and the oracle — on the first queries (no
    prediction, no transpose), on predicted ones (final search + backtrace queued speculatively behind the sweeps),
    and when the prediction falls short (the schedule is changed between queries so that the solve needs more
    sweeps than the previous one: the speculative tail must be redone)."""
    t = synth.make_transducer(60000, 8, 64, 0.0, seed=77)
    assert t["offsets"][-1] >= 1 << 18
    d = to_device(t)
    ref = to_oracle(oracle, t).shortest_path_canonical().to_flat()
    monkeypatch.setenv("WFST_SSSP_DELTA", "0")  # plain frontier sweeps: the fewest sweeps
    few = []
    for q in range(4):
        job = d.shortest_path_begin()
        with pytest.raises(rustfst_amd.WfstError, match="in flight"):
            d.shortest_path_begin()
        assert_flat_identical(job.finish().to_flat(), ref, f"async query {q}")
        few.append(gpu_ctx.stats()["sweeps"])
        with pytest.raises(rustfst_amd.WfstError):
            job.finish()
    monkeypatch.setenv("WFST_SSSP_DELTA", "0.5")  # narrow bands ...
    monkeypatch.setenv("WFST_SSSP_RESIDENT", "0")  # ... and a launch per level: many more sweeps than predicted
    job = d.shortest_path_begin()
    assert_flat_identical(job.finish().to_flat(), ref, "async query after the schedule change")
    many = gpu_ctx.stats()["sweeps"]
    assert many > few[-1] + 4, (few, many)
    assert_flat_identical(d.shortest_path_begin().finish().to_flat(), ref, "async query, long prediction")
    monkeypatch.setenv("WFST_SSSP_DELTA", "0")  # and back: the prediction is now too long, which is harmless
    assert_flat_identical(d.shortest_path_begin().finish().to_flat(), ref, "async query, prediction too long")
    assert_flat_identical(d.shortest_path().to_flat(), ref, "sync after async")
    del d.shortest_path_begin()._fst  # abandoned job is reclaimed
    assert_flat_identical(d.shortest_path().to_flat(), ref, "sync after an abandoned job")
    with pytest.raises(rustfst_amd.WfstError, match="unsupported"):
        d.shortest_path_begin(ShortestPathConfig(nshortest=2))


@pytest.mark.parametrize("seed", range(4))
def test_async_shortest_path_small_and_degenerate(gpu_ctx, oracle, seed):
    """begin/end on small FSTs (no transpose: the tail is queued by _end), FSTs without start / without a path."""
    rng = np.random.default_rng(8800 + seed)
    f = random_fst_flat(rng, int(rng.integers(2, 60)), 4, 3, p_eps_i=0.1, p_eps_o=0.1, p_final=0.2 if seed else 0.0)
    d = to_device(f)
    ref = to_oracle(oracle, f).shortest_path_canonical().to_flat()
    for q in range(3):
        assert_flat_identical(d.shortest_path_begin().finish().to_flat(), ref, f"small async {q}")
    empty = rustfst_amd.VectorFst()
    out = empty.to_device().shortest_path_begin().finish()
    assert out.num_states == 0


@pytest.mark.parametrize("flt", FILTERS, ids=lambda f: f.name)
@pytest.mark.parametrize("seed", range(6))
def test_compose_filters_match_oracle(gpu_ctx, oracle, flt, seed):
    """compose_with_config with every ComposeFilterEnum value on epsilon-rich, cyclic pairs (epsilons on fst1's
    output AND fst2's input side, final and non-final all-epsilon states): ids, arc order, weights, finals and the
    property word are the oracle's, with and without connect."""
    rng = np.random.default_rng(4000 + seed)
    n1, n2 = int(rng.integers(3, 30)), int(rng.integers(3, 30))
    a = random_fst_flat(rng, n1, 4, 3, p_eps_i=0.2, p_eps_o=0.45 if seed % 2 else 0.25, p_final=0.35, sort="olabel")
    b = random_fst_flat(rng, n2, 4, 3, p_eps_i=0.45 if seed % 3 else 0.25, p_eps_o=0.2, p_final=0.35, sort="ilabel")
    da, db = to_device(a), to_device(b)
    oa, ob = to_oracle(oracle, a), to_oracle(oracle, b)
    for connect in (False, True):
        ref = oa.compose(ob, connect=connect, compose_filter=flt.value)
        got = da.compose(db, ComposeConfig(flt, connect=connect))
        assert_flat_identical(got.to_flat(), ref.to_flat(), f"{flt.name} seed {seed} connect={connect}")


@pytest.mark.parametrize("flt", FILTERS, ids=lambda f: f.name)
def test_compose_filters_wide_states_and_batch(gpu_ctx, oracle, flt):
    """fan-outs beyond one wave (general search path) and the fused batch with an explicit filter"""
    rng = np.random.default_rng(77)
    a = random_fst_flat(rng, 5, 90, 6, p_eps_o=0.3, p_final=0.5, sort="olabel", min_fanout=70)
    b = random_fst_flat(rng, 6, 90, 6, p_eps_i=0.3, p_final=0.5, sort="ilabel", min_fanout=70)
    ref = to_oracle(oracle, a).compose(to_oracle(oracle, b), connect=False, compose_filter=flt.value)
    got = to_device(a).compose(to_device(b), ComposeConfig(flt, connect=False))
    assert_flat_identical(got.to_flat(), ref.to_flat(), f"{flt.name} wide")
    accs = [random_fst_flat(rng, 8, 2, 3, p_eps_o=0.3, p_final=0.4, sort="olabel", min_fanout=1, acyclic=True)
            for _ in range(5)]
    t = random_fst_flat(rng, 30, 4, 3, p_eps_i=0.3, p_final=0.3, sort="ilabel", min_fanout=1)
    outs, _ = rustfst_amd.compose_shortest_path_batch([to_device(x) for x in accs], to_device(t), ComposeConfig(flt))
    ot = to_oracle(oracle, t)
    for x, out in zip(accs, outs):
        want = to_oracle(oracle, x).compose(ot, compose_filter=flt.value).shortest_path_canonical().to_flat()
        assert_flat_identical(out.to_flat(), want, f"{flt.name} fused batch")


# ------------------------------------------------------------------ robustness of the boundary
def test_loader_rejects_damaged_files(gpu_ctx, oracle):
    """Truncated or corrupted vector / const files come back as KO with a message — never a crash, never garbage."""
    for name in ("fst_014_hcl.fst", "fst_014_g.fst"):
        data = open(os.path.join(GOLDEN, name), "rb").read()
        for cut in (0, 3, 17, 40, 66, len(data) // 2, len(data) - 1):
            with pytest.raises(rustfst_amd.WfstError):
                rustfst_amd.DeviceFst.from_bytes(data[:cut])
            with pytest.raises(oracle.OracleError):
                oracle.OracleFst.load(data[:cut])
        bad_magic = b"\x00\x00\x00\x00" + data[4:]
        with pytest.raises(rustfst_amd.WfstError):
            rustfst_amd.DeviceFst.from_bytes(bad_magic)
        wrong_type = data.replace(b"standard", b"log\x00\x00\x00\x00\x00", 1)
        with pytest.raises(rustfst_amd.WfstError):
            rustfst_amd.DeviceFst.from_bytes(wrong_type)
    # a 100-byte file whose header claims 2^31 - 2 states must be refused from the header alone (no 16-GB reservation)
    for name in ("fst_014_hcl.fst", "fst_014_g.fst"):
        data = bytearray(open(os.path.join(GOLDEN, name), "rb").read()[:100])
        hdr = data.find(b"standard") + 8 + 4 + 4 + 8 + 8  # after arc type: version, flags, properties, start -> num_states
        data[hdr:hdr + 8] = (2 ** 31 - 2).to_bytes(8, "little")
        with pytest.raises(rustfst_amd.WfstError, match="num_states exceeds"):
            rustfst_amd.DeviceFst.from_bytes(bytes(data))
    # a const file whose state records point outside the arc array
    data = bytearray(open(os.path.join(GOLDEN, "fst_014_hcl.fst"), "rb").read())
    states_at = 80  # 65 header bytes, aligned to 16 (version 1)
    assert int.from_bytes(data[states_at + 4:states_at + 8], "little") == 0  # pos of state 0
    data[states_at + 4:states_at + 8] = (10 ** 6).to_bytes(4, "little")
    with pytest.raises(rustfst_amd.WfstError):
        rustfst_amd.DeviceFst.from_bytes(bytes(data))


def test_degenerate_fsts_through_every_entry_point(gpu_ctx, oracle):
    """no states / states without arcs / no start / no final state"""
    empty = dict(n_states=0, start=None, offsets=np.zeros(1, np.uint32), arcs=np.zeros(0, rustfst_amd.TR_DTYPE),
                 finals=np.zeros(0, np.float32), props=synth.I_LABEL_SORTED | synth.O_LABEL_SORTED)
    lonely = dict(n_states=3, start=1, offsets=np.zeros(4, np.uint32), arcs=np.zeros(0, rustfst_amd.TR_DTYPE),
                  finals=np.array([np.inf, 0.5, np.inf], np.float32), props=synth.I_LABEL_SORTED | synth.O_LABEL_SORTED)
    nostart = dict(lonely, start=None)
    nofinal = dict(lonely, finals=np.full(3, np.inf, np.float32))
    t = random_fst_flat(np.random.default_rng(3), 12, 3, 3, p_final=0.3, sort="ilabel")
    for name, f in (("empty", empty), ("lonely", lonely), ("nostart", nostart), ("nofinal", nofinal)):
        d, o = to_device(f), to_oracle(oracle, f)
        assert_flat_identical(d.shortest_path().to_flat(), o.shortest_path_canonical().to_flat(), name + " shortest_path")
        d.tr_sort(False)
        o.tr_sort(by_olabel=True)
        assert_flat_identical(d.to_flat(), o.to_flat(), name + " tr_sort")
        for flt in (ComposeFilter.AUTOFILTER, ComposeFilter.MATCHFILTER):
            got = d.compose(to_device(t), ComposeConfig(flt))
            assert_flat_identical(got.to_flat(), o.compose(to_oracle(oracle, t), compose_filter=flt.value).to_flat(),
                                  name + " compose " + flt.name)
        outs, _ = rustfst_amd.compose_shortest_path_batch([d, d], to_device(t))
        want = o.compose(to_oracle(oracle, t)).shortest_path_canonical().to_flat()
        for x in outs:
            assert_flat_identical(x.to_flat(), want, name + " fused")
        assert rustfst_amd.DeviceFst.from_bytes(d.to_bytes("const")).to_bytes() == o.store()
    outs, n = rustfst_amd.compose_shortest_path_batch([], to_device(t))
    assert len(outs) == 0 and n == 0


def test_c_example_runs(gpu_ctx, tmp_path):
    """examples/decode_batch.c: the C-ABI driven from plain C, end to end on the GPU (exit status 0 = expected paths)."""
    import shutil
    import subprocess
    from rustfst_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = tmp_path / "decode_batch"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "decode_batch.c"),
                    "-L", libdir, "-lwfst_amd", f"-Wl,-rpath,{libdir}", "-Wl,--allow-shlib-undefined", "-lm", "-o", str(exe)],
                   check=True)
    env = dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "acceptor 0: path of 3 arcs, weight 1.500, output labels: 11 12 11" in r.stdout
    assert "acceptor 1: path of 2 arcs, weight 1.000, output labels: 12 12" in r.stdout


def test_config5_scale_properties():
    """BASELINE configs[4] scale (5M states / 50M arcs, 5 % epsilon arcs): n=1 and n=10 shortest paths, distances
    (Bellman condition on 2M sampled arcs, best final = path weight), a fused batch of 64 acceptors (paths read the
    acceptors' labels) and a 50M-arc tr_sort — tools/config5_scale_check.py, size-independent properties only."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "config5_scale_check.py")], capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-2000:]


def test_one_fst_queried_from_two_contexts_concurrently(gpu_ctx, oracle):
    """A resident FST is read by several contexts (host threads) at once; its lazily built caches (transpose for the
    backtrace, reverse for n-best) are built under the handle's lock.  Every result equals the oracle's."""
    import threading
    t = synth.make_transducer(60000, 8, 64, 0.02, seed=21)
    assert t["offsets"][-1] >= 1 << 18
    d = to_device(t)
    o = to_oracle(oracle, t)
    ref1 = o.shortest_path_canonical().to_flat()
    ref5 = o.shortest_path_n(5).to_flat()
    errors = []

    def work(k):
        try:
            ctx = rustfst_amd.Context(0)
            for q in range(6):
                # the handle belongs to another context: calls run on the handle's own context unless told otherwise,
                # so drive the C-ABI with this thread's context explicitly
                import ctypes as C
                from rustfst_amd import _lib
                out = C.c_void_p()
                cfg = ShortestPathConfig(nshortest=1 if (q + k) % 2 else 5)._c()
                _lib.check(_lib.lib().wfst_shortest_path(ctx._h, d._h, cfg, C.byref(out)), "wfst_shortest_path")
                got = rustfst_amd.DeviceFst(out, ctx).to_flat()
                assert_flat_identical(got, ref1 if (q + k) % 2 else ref5, f"thread {k} query {q}")
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(3)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors


def test_cpp_reference_style_tests_run(gpu_ctx, tmp_path):
    """examples/reference_style_tests.cpp: the reference's K1 / K2 / K3 known-answer tests and its error behaviour, written
    against the C++ mirror include/wfst.hpp, end to end on the GPU."""
    import shutil
    import subprocess
    from rustfst_amd import _lib
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = tmp_path / "ref_tests"
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "reference_style_tests.cpp"),
                    "-L", libdir, "-lwfst_amd", f"-Wl,-rpath,{libdir}", "-Wl,--allow-shlib-undefined", "-o", str(exe)], check=True)
    env = dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all reference-style tests passed" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("lazy", ["0", "1"], ids=["reverse_on_host", "reverse_in_hbm"])
@pytest.mark.parametrize("seed", range(8))
def test_reverse_matches_oracle(gpu_ctx, oracle, seed, lazy, monkeypatch):
    """algorithms::reverse (reverse.rs:33-87) as a public operation: states, arc order, weights, finals, start and the
    property word (the reference's mutation bookkeeping + reverse_properties) are the oracle's."""
    monkeypatch.setenv("WFST_NBEST_LAZY", lazy)
    rng = np.random.default_rng(8100 + seed)
    if seed == 0:
        flat = dict(n_states=0, start=None, offsets=np.zeros(1, np.uint32), arcs=np.zeros(0, rustfst_amd.TR_DTYPE),
                    finals=np.zeros(0, np.float32), props=0)
    elif seed == 1:  # acceptor, unweighted, acyclic: the positive property bits must survive
        flat = synth.linear_acceptor_flat([3, 1, 2])
    else:
        flat = random_fst_flat(rng, int(rng.integers(1, 300)), int(rng.integers(1, 9)), 6, p_eps_i=0.2 * (seed % 2),
                               p_eps_o=0.2 * (seed % 3 == 0), p_final=rng.random() * 0.5, sort=["ilabel", "olabel", "none"][seed % 3],
                               acyclic=bool(seed % 2), weight_grid=512 if seed % 4 else 1)
        if seed == 5:
            flat["start"] = None
    d, o = to_device(flat), to_oracle(oracle, flat)
    assert_flat_identical(d.reverse().to_flat(), o.reverse().to_flat(), f"reverse seed {seed}")
    assert_flat_identical(d.reverse().reverse().to_flat(), o.reverse().reverse().to_flat(), f"reverse twice seed {seed}")


@pytest.mark.parametrize("lazy", ["0", "1"], ids=["reverse_on_host", "reverse_in_hbm"])
def test_reverse_and_nbest_with_hub_states(gpu_ctx, oracle, lazy, monkeypatch):
    """Hub states (a final sink every state points at, a back-off state half of them point at: in-degrees of 1e5, the
    shape of LM / HCLG graphs): the in-arc segments of such states are put back into the reference's order by a segmented
    radix sort, not by the one-lane insertion sort of ordinary segments.  reverse() and the n-best search built on it stay
    bit-identical to the oracle, and quick."""
    import time
    monkeypatch.setenv("WFST_NBEST_LAZY", lazy)
    t = synth.make_transducer(120_000, 4, 32, 0.0, seed=11)
    arcs = t["arcs"].copy()
    n, f = t["n_states"], 4
    arcs["nextstate"][0::f] = 7                                    # every state -> hub 7
    arcs["nextstate"][1:n * f // 2:f] = 12345                      # half of the states -> hub 12345
    t["arcs"] = arcs
    t["finals"][:] = np.inf
    t["finals"][7] = np.float32(0.25)
    d, o = to_device(t), to_oracle(oracle, t)
    t0 = time.perf_counter()
    got = d.reverse().to_flat()
    assert time.perf_counter() - t0 < 5.0
    assert_flat_identical(got, o.reverse().to_flat(), "reverse with hub states")
    assert_flat_identical(d.shortest_path(ShortestPathConfig(nshortest=5)).to_flat(), o.shortest_path_n(5).to_flat(), "n-best with hub states")


# ------------------------------------------------------------------ the string o T kernel of the fused batch
@pytest.mark.parametrize("kernel", ["1", "0"], ids=["string_kernel", "general_kernel"])
@pytest.mark.parametrize("seed", range(10))
def test_string_batch_both_kernels_match_oracle(gpu_ctx, oracle, seed, kernel, monkeypatch):
    _string_batch_case(gpu_ctx, oracle, seed, kernel, monkeypatch)


@pytest.mark.parametrize("kernel", ["1", "0"], ids=["string_kernel", "general_kernel"])
@pytest.mark.parametrize("seed", [0, 3])
def test_string_batch_through_copy_commands(gpu_ctx, oracle, seed, kernel, monkeypatch):
    """The same cases with WFST_BATCH_COPY: descriptors, results and path arcs travel by copy commands (what large
    batches do) instead of being read from / written to pinned host memory by the kernel itself (the default when the
    whole path buffer fits there)."""
    monkeypatch.setenv("WFST_BATCH_COPY", "1")
    _string_batch_case(gpu_ctx, oracle, seed, kernel, monkeypatch)


def _string_batch_case(gpu_ctx, oracle, seed, kernel, monkeypatch):
    """Linear epsilon-free acceptors against an input-epsilon-free T: the specialised string o T kernel and the general
    kernel must both return the oracle's canonical path (ids of the untrimmed composition decide ties: small alphabets
    and integer weights make ties and wide levels frequent), the same composed-arc count, and identical property words."""
    monkeypatch.setenv("WFST_STRING_KERNEL", kernel)
    rng = np.random.default_rng(12_000 + seed)
    ties = seed % 2 == 0
    n_t, fan, sigma = int(rng.integers(2, 60)), int(rng.integers(1, 7)), int(rng.integers(1, 4))
    t = random_fst_flat(rng, n_t, fan, sigma, p_final=0.4, sort="ilabel", min_fanout=1, weight_grid=1 if ties else 512,
                        max_w=3 if ties else 2560)
    accs = []
    for k in range(6):
        length = int(rng.integers(0, 40))
        a = synth.linear_acceptor_flat(rng.integers(1, sigma + 1, length).astype(np.uint32), final_weight=0.5 * (k % 2))
        if k % 3 == 0 and length:
            a["arcs"]["weight"] = (rng.integers(0, 4, length)).astype(np.float32)  # weighted string
            a["props"] = 0x0000_0000_0001_0000 | synth.I_LABEL_SORTED | synth.O_LABEL_SORTED  # ACCEPTOR + sorted, rest unknown
        accs.append(a)
    ctx = rustfst_amd.default_context()
    dacc = rustfst_amd.DeviceFst.upload_many(accs, ctx)
    outs, n_arcs = rustfst_amd.compose_shortest_path_batch(dacc, to_device(t))
    used = ctx.stats()["string_problems"]
    assert used == (len(accs) if kernel == "1" else 0)
    ot = to_oracle(oracle, t)
    want_arcs = 0
    for a, out in zip(accs, outs):
        oc = to_oracle(oracle, a).compose(ot, connect=False)
        want_arcs += oc.num_arcs
        assert_flat_identical(out.to_flat(), oc.shortest_path_canonical().to_flat(), f"seed {seed} kernel {kernel}")
    assert n_arcs == want_arcs


@pytest.mark.parametrize("seed", range(3))
def test_string_batch_packed_workgroups(gpu_ctx, oracle, seed):
    """Batches of 16 or more strings run several waves per workgroup, every wave with its own slice of LDS sized from the
    longest acceptor; with a small alphabet some compositions outgrow their slice and are redone by the general kernel.
    Every result is the oracle's canonical path."""
    rng = np.random.default_rng(15_000 + seed)
    sigma = 2 + seed
    t = random_fst_flat(rng, 40, 5, sigma, p_final=0.3, sort="ilabel", min_fanout=1, weight_grid=512)
    accs = [synth.linear_acceptor_flat(rng.integers(1, sigma + 1, int(rng.integers(1, 90))).astype(np.uint32), final_weight=0.25 * (k % 3))
            for k in range(27)]
    ctx = rustfst_amd.default_context()
    outs, n_arcs = rustfst_amd.compose_shortest_path_batch(rustfst_amd.DeviceFst.upload_many(accs, ctx), to_device(t))
    ot = to_oracle(oracle, t)
    want_arcs = 0
    for k, (a, out) in enumerate(zip(accs, outs)):
        oc = to_oracle(oracle, a).compose(ot, connect=False)
        want_arcs += oc.num_arcs
        assert_flat_identical(out.to_flat(), oc.shortest_path_canonical().to_flat(), f"seed {seed} string {k}")
    assert n_arcs == want_arcs


@pytest.mark.parametrize("n_acc", [27, 700], ids=["one_thread", "host_threads"])
def test_fused_batch_as_packed_records(gpu_ctx, n_acc):
    """wfst_compose_shortest_path_batch_packed: the same batch with its results as one table (the record layout of
    wfst_fst_pack_paths) instead of path handles — word for word what packing the handles gives, for strings the string
    kernel takes, strings with no match in T (empty results), strings that outgrow their slice and are redone by the
    general kernel, a branching first operand, and enough results for the host threads (> 512); a record too short for a
    path is an error, not a truncation."""
    from rustfst_amd import dist
    rng = np.random.default_rng(77 + n_acc)
    sigma = 3
    t = random_fst_flat(rng, 40, 5, sigma, p_final=0.3, sort="ilabel", min_fanout=1, weight_grid=512)
    def walk(length):  # the input labels along a random walk through T: a string that matches at least that far
        s, labs = int(t["start"]), []
        for _ in range(length):
            b, e = int(t["offsets"][s]), int(t["offsets"][s + 1])
            k = int(rng.integers(b, e))
            labs.append(int(t["arcs"]["ilabel"][k]))
            s = int(t["arcs"]["nextstate"][k])
        return np.array(labs, dtype=np.uint32)

    accs = [synth.linear_acceptor_flat(walk(int(rng.integers(0, 90))) if k % 2 else rng.integers(1, sigma + 1, int(rng.integers(0, 90))).astype(np.uint32),
                                       final_weight=0.25 * (k % 3)) for k in range(n_acc - 2)]
    accs.append(synth.linear_acceptor_flat(np.array([1, 9, 1], dtype=np.uint32)))  # label 9 is not in T: no path
    accs.append(random_fst_flat(rng, 12, 2, sigma, p_final=0.4, sort="olabel"))  # not a string: the general kernel
    ctx = rustfst_amd.default_context()
    dacc, dt = rustfst_amd.HandleArray(rustfst_amd.DeviceFst.upload_many(accs, ctx)), to_device(t)
    outs, n_arcs = rustfst_amd.compose_shortest_path_batch(dacc, dt)
    want = dist.pack_device_paths(outs, 96)
    got, n_arcs_p = rustfst_amd.compose_shortest_path_batch_packed(dacc, dt, 96)
    assert n_arcs_p == n_arcs and got.shape == want.shape
    np.testing.assert_array_equal(got, want)
    assert got[-2, 2] == 0 and got[:, 2].sum() >= 3 and got[:, 0].max() > 8  # an empty record for the unmatched string; real paths
    flats = dist.unpack_paths(got[:5])
    for k in range(5):
        f = outs[k].to_flat()
        np.testing.assert_array_equal(flats[k]["arcs"], f["arcs"])
    with pytest.raises(rustfst_amd.WfstError, match="longer than the record"):
        rustfst_amd.compose_shortest_path_batch_packed(dacc, dt, 8)
    again, _ = rustfst_amd.compose_shortest_path_batch_packed(dacc, dt, 96)  # (the context is usable after the error)
    np.testing.assert_array_equal(again, want)


def test_batch_results_as_views_into_the_result_block(gpu_ctx, monkeypatch):
    """The path FSTs of a serving-size fused batch point into the batch's pinned result block until their arrays are asked for
    (wfst_fst::path_form): every way of reading one — download, pack_paths (straight from the block), the OpenFST writer,
    a second algorithm on it (upload), conversion to a VectorFst — gives exactly what the eager construction
    (WFST_BATCH_EAGER_PATHS=1) gives, results outlive later batches on the same context (each batch has a block of its own
    while results point into it), and a result nobody reads is released like any other."""
    from rustfst_amd import dist
    rng = np.random.default_rng(4242)
    t = random_fst_flat(rng, 300, 6, 5, p_final=0.2, sort="ilabel", min_fanout=2, weight_grid=512)
    def walk(length):
        s, labs = int(t["start"]), []
        for _ in range(length):
            b, e = int(t["offsets"][s]), int(t["offsets"][s + 1])
            k = int(rng.integers(b, e))
            labs.append(int(t["arcs"]["ilabel"][k]))
            s = int(t["arcs"]["nextstate"][k])
        return np.array(labs, dtype=np.uint32)
    accs = [synth.linear_acceptor_flat(walk(int(rng.integers(1, 60))), final_weight=0.5 * (k % 2)) for k in range(40)]
    accs.append(synth.linear_acceptor_flat(np.array([1, 99, 1], dtype=np.uint32)))  # no path: built eagerly (an empty FST)
    ctx = rustfst_amd.default_context()
    dacc, dt = rustfst_amd.HandleArray(rustfst_amd.DeviceFst.upload_many(accs, ctx)), to_device(t)
    monkeypatch.setenv("WFST_BATCH_EAGER_PATHS", "1")
    eager, n_e = rustfst_amd.compose_shortest_path_batch(dacc, dt)
    eager_flats = [eager[k].to_flat() for k in range(len(accs))]
    want_rec = dist.pack_device_paths(eager, 64)
    monkeypatch.delenv("WFST_BATCH_EAGER_PATHS")
    views, n_v = rustfst_amd.compose_shortest_path_batch(dacc, dt)
    assert n_v == n_e
    np.testing.assert_array_equal(dist.pack_device_paths(views, 64), want_rec)  # (read from the block: no arrays built)
    later = [rustfst_amd.compose_shortest_path_batch(dacc, dt)[0] for _ in range(3)]  # later batches: other blocks
    np.testing.assert_array_equal(dist.pack_device_paths(views, 64), want_rec)
    for k in range(len(accs)):
        assert_flat_identical(views[k].to_flat(), eager_flats[k], f"result {k}")  # download: builds the arrays
    np.testing.assert_array_equal(dist.pack_device_paths(views, 64), want_rec)  # ... and packing still agrees afterwards
    fresh = later[0]
    k = next(i for i in range(len(accs)) if eager_flats[i]["n_states"] > 3)
    # a second algorithm on a view (upload), the writer, the VectorFst conversion
    assert_flat_identical(fresh[k].shortest_path().to_flat(), eager[k].shortest_path().to_flat(), "shortest_path of a view")
    assert later[1][k].to_bytes() == eager[k].to_bytes()
    va, vb = later[2][k].to_vector_fst(), eager[k].to_vector_fst()
    assert va.num_states() == vb.num_states() and va.start() == vb.start()
    for s_ in range(va.num_states()):
        assert va.num_trs(s_) == vb.num_trs(s_) and va.final_weight(s_) == vb.final_weight(s_)
    del later, fresh, views  # (results nobody read: released with their blocks)
    again, _ = rustfst_amd.compose_shortest_path_batch(dacc, dt)
    np.testing.assert_array_equal(dist.pack_device_paths(again, 64), want_rec)
    # in-place operations and further algorithms on views: what they do to the eagerly built FST
    ops = [lambda f: f.tr_sort(False), lambda f: f.project(), lambda f: f.reverse(), lambda f: f.rm_epsilon(), lambda f: f.connect(),
           lambda f: f.compose(dt) if False else f.shortest_path()]
    for j, op in enumerate(ops):
        a, b = op(again[k + j] if k + j < 40 else again[k]), op(eager[k + j] if k + j < 40 else eager[k])
        assert_flat_identical(a.to_flat(), b.to_flat(), f"operation {j} on a view")
    # more batches with live results than the ring keeps free blocks: every batch still has a block of its own
    held = [rustfst_amd.compose_shortest_path_batch(dacc, dt)[0] for _ in range(12)]
    for h in held:
        np.testing.assert_array_equal(dist.pack_device_paths(h, 64), want_rec)
    del held


@pytest.mark.parametrize("waits", ["tickets", "hip"])
def test_completion_by_ticket_and_by_hip_wait_agree(gpu_ctx, oracle, monkeypatch, waits):
    """_end calls learn that their kernels are done from tickets the kernels store into pinned memory (behind a system-scope
    fence), and fall back to the HIP event / stream wait (long kernels, WFST_SSSP_EVENT_WAIT / WFST_BATCH_STREAM_WAIT): both
    ways, repeated asynchronous shortest_path queries overlapped with fused batches give the oracle's results every time."""
    if waits == "hip":
        monkeypatch.setenv("WFST_SSSP_EVENT_WAIT", "1")
        monkeypatch.setenv("WFST_BATCH_STREAM_WAIT", "1")
    t = synth.make_transducer(120_000, 8, 64, 0.0, seed=5)
    accs = synth.make_acceptors(t, 48, 60, seed0=77)
    ot = to_oracle(oracle, t)
    ref_sp = ot.shortest_path_canonical().to_flat()
    refs = [to_oracle(oracle, a).compose(ot).shortest_path_canonical().to_flat() for a in accs[:6]]
    ctx2 = rustfst_amd.Context(0)
    dt, dt2 = to_device(t), rustfst_amd.DeviceFst.from_arrays(t["n_states"], t["start"], t["offsets"], t["arcs"], t["finals"], t["props"], ctx2)
    dacc = rustfst_amd.HandleArray(rustfst_amd.DeviceFst.upload_many(accs, ctx2))
    for it in range(12):
        sp_job = dt.shortest_path_begin()
        job = rustfst_amd.compose_shortest_path_batch_begin(dacc, dt2, ctx=ctx2)
        outs, _ = job.finish()
        sp = sp_job.finish()
        assert_flat_identical(sp.to_flat(), ref_sp, f"{waits}: query {it}")
        for k in range(6):
            assert_flat_identical(outs[k].to_flat(), refs[k], f"{waits}: step {it} result {k}")


def test_string_kernel_falls_back_where_it_does_not_apply(gpu_ctx, oracle):
    """Levels wider than one wave, input epsilons in T, epsilons or branching in fst1, explicit non-sequence filters: the
    batch silently takes the general kernel (per problem) and still matches the oracle."""
    rng = np.random.default_rng(5)
    ctx = rustfst_amd.default_context()
    # 1. a level wider than 64 states: T fans one label out to 100 distinct states
    n = 103
    rows, offsets = [], [0]
    for s in range(n):
        if s == 0:
            rows += [(1, 1, float(k % 5), 1 + k) for k in range(100)]
        elif s <= 100:
            rows += [(1, 2, 1.0, 101)]
        elif s == 101:
            rows += [(1, 3, 0.5, 102)]
        offsets.append(len(rows))
    arcs = np.array(rows, dtype=rustfst_amd.TR_DTYPE)
    finals = np.full(n, np.inf, np.float32)
    finals[102] = 0.0
    t = dict(n_states=n, start=0, offsets=np.array(offsets, np.uint32), arcs=arcs, finals=finals,
             props=synth.I_LABEL_SORTED)
    a = synth.linear_acceptor_flat(np.array([1, 1, 1], np.uint32))
    outs, _ = rustfst_amd.compose_shortest_path_batch(rustfst_amd.DeviceFst.upload_many([a, a], ctx), to_device(t))
    assert ctx.stats()["string_problems"] == 0  # both problems overflowed the 64-state level and were redone
    want = to_oracle(oracle, a).compose(to_oracle(oracle, t)).shortest_path_canonical().to_flat()
    for o in outs:
        assert_flat_identical(o.to_flat(), want, "wide level")
    # 2. T with input epsilons -> general kernel for everybody
    t2 = random_fst_flat(rng, 30, 4, 3, p_eps_i=0.3, p_final=0.3, sort="ilabel", min_fanout=1)
    b = synth.linear_acceptor_flat(np.array([1, 2, 3, 1], np.uint32))
    outs, _ = rustfst_amd.compose_shortest_path_batch(rustfst_amd.DeviceFst.upload_many([b], ctx), to_device(t2))
    assert ctx.stats()["string_problems"] == 0
    assert_flat_identical(outs[0].to_flat(), to_oracle(oracle, b).compose(to_oracle(oracle, t2)).shortest_path_canonical().to_flat(), "T with eps")
    # 3. mixed batch: a string, a branching acceptor, a string with an epsilon label; explicit Match filter for all
    t3 = random_fst_flat(rng, 40, 4, 3, p_final=0.3, sort="ilabel", min_fanout=1)
    branching = random_fst_flat(rng, 6, 2, 3, p_final=0.5, sort="olabel", acyclic=True, min_fanout=1)
    eps_string = synth.linear_acceptor_flat(np.array([1, 2], np.uint32))
    eps_string["arcs"]["ilabel"][1] = 0
    eps_string["arcs"]["olabel"][1] = 0
    eps_string["props"] = 0x0000_0000_0001_0000 | synth.I_LABEL_SORTED | synth.O_LABEL_SORTED
    batch = [b, branching, eps_string]
    for flt, expect in ((ComposeFilter.AUTOFILTER, 1), (ComposeFilter.SEQUENCEFILTER, 1), (ComposeFilter.MATCHFILTER, 0)):
        outs, _ = rustfst_amd.compose_shortest_path_batch(rustfst_amd.DeviceFst.upload_many(batch, ctx), to_device(t3), ComposeConfig(flt))
        assert ctx.stats()["string_problems"] == expect
        for x, out in zip(batch, outs):
            want = to_oracle(oracle, x).compose(to_oracle(oracle, t3), compose_filter=flt.value).shortest_path_canonical().to_flat()
            assert_flat_identical(out.to_flat(), want, f"mixed batch {flt.name}")


# ------------------------------------------------------------------ §8 row A12 / N1: look-ahead composition
def _lookahead_pair(rng, n1, n2, acyclic=False, sigma=3, p_oeps=0.45, p_ieps=0.3):
    a = random_fst_flat(rng, n1, 3, sigma, p_eps_i=0.2, p_eps_o=p_oeps, p_final=0.3, sort="olabel", acyclic=acyclic)
    b = random_fst_flat(rng, n2, 3, sigma, p_eps_i=p_ieps, p_eps_o=0.2, p_final=0.3, sort="ilabel", acyclic=acyclic)
    return a, b


@pytest.mark.parametrize("path", ["wave", "wide"])
def test_k13_lookahead_hand_traced_known_answers(gpu_ctx, monkeypatch, path):
    """Look-ahead composition against the six answers traced by hand through the reference's source
    (tests/golden/K13_DERIVATION.md section 2, tests/golden/k13_lookahead.json): the relabelled second operand, the pruned
    dead end, pushed weights and labels, state numbering and arc order — on the single-wave kernel and on the wide driver,
    and through the batch entry point."""
    monkeypatch.setenv("WFST_LOOKAHEAD_PATH", path)
    g = golden("k13_lookahead.json")
    for case in g["cases"]:
        la = rustfst_amd.LookAhead(vbuild(case["fst1"]).to_device())  # (relabels and re-sorts its operand, as MatcherFst::new does)
        rel = la.relabel(vbuild(case["fst2"]).to_device())
        if "relabeled_fst1" in case:
            flat_matches_spec(la.fst1.to_flat(), case["relabeled_fst1"])
        if "relabeled_fst2" in case:
            flat_matches_spec(rel.to_flat(), case["relabeled_fst2"])
        flat_matches_spec(la.compose(rel).to_flat(), case["expected"])
        for o in la.compose_batch([rel, rel]):
            flat_matches_spec(o.to_flat(), case["expected"])


@pytest.mark.parametrize("path", ["wave", "wide"])
@pytest.mark.parametrize("seed", range(24))
def test_lookahead_compose_both_drivers(gpu_ctx, oracle, monkeypatch, seed, path):
    """The single-wave kernel and the level-per-launch wide path (one wave per composed state, tuples interned through
    atomicMin of their emission order) give the oracle's FST bit for bit on the same inputs."""
    monkeypatch.setenv("WFST_LOOKAHEAD_PATH", path)
    rng = np.random.default_rng(31_000 + seed)
    a, b = _lookahead_pair(rng, int(rng.integers(1, 60)), int(rng.integers(1, 40)), acyclic=(seed % 5 == 0),
                           sigma=int(rng.integers(2, 5)), p_oeps=0.5 if seed % 2 else 0.3)
    ref = to_oracle(oracle, a).compose_lookahead(to_oracle(oracle, b))
    la = rustfst_amd.LookAhead(to_device(a))
    out = la.compose(la.relabel(to_device(b)))
    assert_flat_identical(out.to_flat(), ref.to_flat(), f"look-ahead composition on the {path} path")


@pytest.mark.parametrize("seed", range(40))
def test_lookahead_compose_matches_oracle(gpu_ctx, oracle, seed, monkeypatch):
    """wfst_lookahead_create / _relabel / wfst_compose_lookahead against the oracle's restatement of the reference's
    look-ahead configuration (cmds/compose.rs:77-181): relabelled operands, state numbering, arc order, pushed weights
    and labels, finals and the property word are identical, on epsilon-rich cyclic and acyclic pairs (every other seed
    with the host precompute and relabelling forced onto several threads)."""
    if seed % 2:
        monkeypatch.setenv("WFST_HOST_THREADS", "3")
    rng = np.random.default_rng(21_000 + seed)
    a, b = _lookahead_pair(rng, int(rng.integers(1, 30)), int(rng.integers(1, 30)), acyclic=(seed % 4 == 0),
                           sigma=int(rng.integers(2, 6)))
    ref, r1, r2 = to_oracle(oracle, a).compose_lookahead(to_oracle(oracle, b), want_relabeled=True)
    la = rustfst_amd.LookAhead(to_device(a))
    assert_flat_identical(la.fst1.to_flat(), r1.to_flat(), "relabelled fst1")
    d2 = la.relabel(to_device(b))
    assert_flat_identical(d2.to_flat(), r2.to_flat(), "relabelled fst2")
    out = la.compose(d2)
    assert_flat_identical(out.to_flat(), ref.to_flat(), "look-ahead composition")
    # and it is the same weighted relation as the plain composition: same best path weight after trimming
    plain = to_device(a).compose(to_device(b))
    w1, w2 = plain.shortest_path().to_flat(), out.shortest_path().to_flat()
    tot = lambda p: None if p["n_states"] == 0 else round((float(p["arcs"]["weight"].sum()) + float(p["finals"][0])) * 1024)
    assert tot(w1) == tot(w2)


def test_lookahead_relabelling_of_large_operands(gpu_ctx, oracle):
    """Operands of more than 2^20 arcs: the host side of wfst_lookahead_create / _relabel goes through its table-driven
    relabelling and sorts the states' arcs on several host threads; relabelled fst1, relabelled fst2 (with labels fst1
    never emits) and the composition with a tiny second operand are the oracle's, bit for bit."""
    a = _swap_labels(synth.make_transducer(120_000, 9, 300, 0.1, seed=41, p_final=0.02))
    b_big = synth.make_transducer(110_000, 10, 340, 0.05, seed=42, p_final=0.02)  # labels 301..340 are new to fst1
    b_small = synth.make_transducer(3, 4, 300, 0.0, seed=43, p_final=0.5)
    assert a["offsets"][-1] >= 1 << 20 and b_big["offsets"][-1] >= 1 << 20
    oa = to_oracle(oracle, a)
    ref, r1, r2 = oa.compose_lookahead(to_oracle(oracle, b_small), want_relabeled=True)
    la = rustfst_amd.LookAhead(to_device(a))
    assert_flat_identical(la.fst1.to_flat(), r1.to_flat(), "relabelled fst1 (1.08 M arcs)")
    d2 = la.relabel(to_device(b_small))
    assert_flat_identical(d2.to_flat(), r2.to_flat(), "relabelled small fst2")
    assert_flat_identical(la.compose(d2).to_flat(), ref.to_flat(), "look-ahead composition")
    # the big second operand starts in an extra state without arcs, so the composition is one state while the relabelling
    # still rewrites and re-sorts 1.1 M arcs
    nb = b_big["n_states"]
    iso = dict(b_big)
    iso["n_states"] = nb + 1
    iso["start"] = nb
    iso["offsets"] = np.concatenate([b_big["offsets"], b_big["offsets"][-1:]]).astype(np.uint32)
    iso["finals"] = np.concatenate([b_big["finals"], np.array([np.inf], np.float32)]).astype(np.float32)
    ref_b, _, r2_big = oa.compose_lookahead(to_oracle(oracle, iso), want_relabeled=True)
    d2_big = la.relabel(to_device(iso))
    assert_flat_identical(d2_big.to_flat(), r2_big.to_flat(), "relabelled fst2 (1.1 M arcs, labels fst1 never emits)")
    assert_flat_identical(la.compose(d2_big).to_flat(), ref_b.to_flat(), "look-ahead composition from an isolated start state")


def _swap_labels(t):
    """output-epsilon version of a synthetic transducer (its epsilons sit on the input side): swap the label columns and
    re-sort by olabel"""
    arcs = t["arcs"].copy()
    arcs["ilabel"], arcs["olabel"] = t["arcs"]["olabel"].copy(), t["arcs"]["ilabel"].copy()
    off = t["offsets"]
    for s in range(t["n_states"]):
        seg = arcs[off[s]:off[s + 1]]
        arcs[off[s]:off[s + 1]] = seg[np.argsort(seg["olabel"], kind="stable")]
    out = dict(t)
    out["arcs"] = arcs
    out["props"] = synth.O_LABEL_SORTED
    return out


@pytest.mark.parametrize("n1,n2,fan2,sigma,seed", [(300, 20, 8, 8, 1), (700, 30, 10, 10, 3), (2000, 50, 12, 12, 3)])
def test_lookahead_compose_larger(gpu_ctx, oracle, n1, n2, fan2, sigma, seed):
    """Compositions of 7 k ... 120 k states: fst1 with 20 % output epsilons, fst2 with about as many arcs per state as
    there are labels, so most labels match somewhere (several arena growth retries, levels of thousands of arcs, pushed
    labels and weights on most paths)."""
    a = _swap_labels(synth.make_transducer(n1, 3, sigma, 0.2, seed=seed, p_final=0.05))
    b = synth.make_transducer(n2, fan2, sigma, 0.05, seed=100 + seed, p_final=0.05)
    ref, r1, r2 = to_oracle(oracle, a).compose_lookahead(to_oracle(oracle, b), want_relabeled=True)
    la = rustfst_amd.LookAhead(to_device(a))
    d2 = la.relabel(to_device(b))
    assert_flat_identical(la.fst1.to_flat(), r1.to_flat(), "relabelled fst1")
    assert_flat_identical(d2.to_flat(), r2.to_flat(), "relabelled fst2")
    out = la.compose(d2)
    assert out.num_states > 2048  # beyond the single-wave driver: redone on the wide path
    st = gpu_ctx.lookahead_stats()
    assert (st["items"], st["wide_items"], st["wave_answered"], st["one_limits"]) == (1, 1, 0, 1)
    assert_flat_identical(out.to_flat(), ref.to_flat(), f"look-ahead composition {n1}x{n2}")
    # the same handle serves further second operands (labels unseen so far get fresh indices, as in the reference)
    b2 = synth.make_transducer(50, 3, 40, 0.05, seed=500 + seed, p_final=0.1)
    out2 = la.compose(la.relabel(to_device(b2))).to_flat()
    assert out2["n_states"] >= 1


def test_lookahead_compose_degenerate_and_errors(gpu_ctx, oracle):
    rng = np.random.default_rng(5)
    a, b = _lookahead_pair(rng, 6, 6)
    la = rustfst_amd.LookAhead(to_device(a))
    with pytest.raises(rustfst_amd.WfstError, match="not sorted"):
        la.compose(to_device(random_fst_flat(rng, 5, 3, 3, sort="none")))
    # an operand without a start state: empty result with VectorFst::new() properties
    empty = rustfst_amd.VectorFst().to_device()
    out = la.compose(la.relabel(empty))
    assert out.num_states == 0
    ref = to_oracle(oracle, a).compose_lookahead(oracle.OracleFst()).to_flat()
    assert out.to_flat()["props"] == ref["props"]
    # fst1 without arcs / single state
    one = random_fst_flat(rng, 1, 0, 3, p_final=1.0, sort="olabel")
    la1 = rustfst_amd.LookAhead(to_device(one))
    ref1 = to_oracle(oracle, one).compose_lookahead(to_oracle(oracle, b)).to_flat()
    assert_flat_identical(la1.compose(la1.relabel(to_device(b))).to_flat(), ref1, "single-state fst1")


def test_lookahead_compose_batch(gpu_ctx, oracle):
    """wfst_compose_lookahead_batch: 40 second operands against one look-ahead handle in a single launch (one wave per
    problem) == the one-by-one calls == the oracle; a problem that outgrows the single wave is redone on the wide path,
    operands without a start state give the empty FST."""
    rng = np.random.default_rng(77)
    a = _swap_labels(synth.make_transducer(300, 3, 8, 0.2, seed=1, p_final=0.05))
    la = rustfst_amd.LookAhead(to_device(a))
    oa = to_oracle(oracle, a)
    bs = [random_fst_flat(rng, int(rng.integers(1, 12)), 3, 8, p_eps_i=0.2, p_eps_o=0.1, p_final=0.4, sort="ilabel") for _ in range(38)]
    bs.append(synth.make_transducer(20, 8, 8, 0.05, seed=101, p_final=0.05))  # 7 k composed states: wide path
    d2 = [la.relabel(to_device(b)) for b in bs] + [la.relabel(rustfst_amd.VectorFst().to_device())]
    outs = la.compose_batch(d2)
    assert len(outs) == 40 and outs[-1].num_states == 0
    assert outs[38].num_states > 2048
    st = gpu_ctx.lookahead_stats()
    assert (st["items"], st["items_no_start"], st["wave_answered"] + st["wide_items"], st["one_limits"]) == (40, 1, 39, 0)
    assert st["wide_items"] >= 1  # (outs[38] at least)
    for i, b in enumerate(bs):
        ref = oa.compose_lookahead(to_oracle(oracle, b)).to_flat()
        assert_flat_identical(outs[i].to_flat(), ref, f"batched look-ahead composition {i}")
    for i in (0, 7, 38):
        assert_flat_identical(la.compose(d2[i]).to_flat(), outs[i].to_flat(), f"single vs batch {i}")
    assert la.compose_batch([]) == []


# ------------------------------------------------------------------ §8(f) N4: project around the path
def test_project_known_answer_and_oracle(gpu_ctx, oracle):
    """wfst_fst_project against the reference's own test vectors (test_project.py:5-97) and, on random FSTs, against the
    oracle: arcs, per-state epsilon counters as seen by a following composition, and the property word."""
    from rustfst_amd import ProjectType
    g = golden("k7_project.json")
    for ptype, key in ((ProjectType.PROJECT_INPUT, "expected_input"), (ProjectType.PROJECT_OUTPUT, "expected_output")):
        got = vbuild(g["fst"]).project(ptype)
        assert got == vbuild(g[key])
    assert rustfst_amd.project(vbuild(g["fst"])) == vbuild(g["expected_input"])  # default = input projection
    # in place, like the reference (vector_fst.py:525-538 returns self): the object itself is projected, and what a later
    # composition sees agrees with what trs() shows
    f = vbuild(g["fst"])
    f.to_device()  # a cached device copy must not survive the projection unprojected (or be the only projected one)
    assert f.project(ProjectType.PROJECT_OUTPUT) is f and f == vbuild(g["expected_output"])
    assert all(tr.ilabel == tr.olabel for s in range(f.num_states()) for tr in f.trs(s))
    same = vbuild(g["expected_output"])
    same.tr_sort(False)
    f.tr_sort(False)
    other = vbuild(g["expected_output"])
    other.tr_sort(True)
    assert f.compose(other) == same.compose(other)
    rng = np.random.default_rng(2024)
    for k in range(12):
        f = random_fst_flat(rng, int(rng.integers(1, 40)), 4, 4, p_eps_i=0.3, p_eps_o=0.3, p_final=0.3,
                            sort=("ilabel", "olabel", "none")[k % 3])
        for out in (False, True):
            d = to_device(f).project(ProjectType.PROJECT_OUTPUT if out else ProjectType.PROJECT_INPUT)
            ref = to_oracle(oracle, f).project(out)
            assert_flat_identical(d.to_flat(), ref.to_flat(), f"project output={out}")
            # the recipe of rustfst/src/lib.rs:70-82: compose -> project -> shortest path (epsilon facts re-derived)
            if (d.to_flat()["props"] & synth.O_LABEL_SORTED) or (f["props"] & synth.I_LABEL_SORTED):
                b = random_fst_flat(rng, 6, 3, 4, p_eps_i=0.2, p_final=0.4, sort="ilabel")
                try:
                    refc = ref.compose(to_oracle(oracle, b))
                except oracle.OracleError:
                    continue
                assert_flat_identical(d.compose(to_device(b)).to_flat(), refc.to_flat(), "compose after project")


# ------------------------------------------------------------------ compose of one large pair: the wide driver
@pytest.mark.parametrize("flt", [ComposeFilter.AUTOFILTER] + FILTERS, ids=lambda f: f.name)
@pytest.mark.parametrize("seed", range(5))
def test_compose_wide_driver_matches_oracle(gpu_ctx, oracle, monkeypatch, flt, seed):
    """compose() pinned to the wide driver (compose_wide.hip: one wave per composed state of a BFS level, device-side
    connect) on the epsilon-rich pairs of the filter tests: ids, arc order, weights, finals, property word == oracle for
    every filter, with and without connect, including results that trim to nothing."""
    monkeypatch.setenv("WFST_COMPOSE_PATH", "wide")
    rng = np.random.default_rng(9000 + seed)
    n1, n2 = int(rng.integers(1, 40)), int(rng.integers(1, 40))
    a = random_fst_flat(rng, n1, 4, 3, p_eps_i=0.2, p_eps_o=0.45 if seed % 2 else 0.25, p_final=0.35 if seed else 0.0, sort="olabel")
    b = random_fst_flat(rng, n2, 4, 3, p_eps_i=0.45 if seed % 3 else 0.25, p_eps_o=0.2, p_final=0.35, sort="ilabel")
    da, db = to_device(a), to_device(b)
    oa, ob = to_oracle(oracle, a), to_oracle(oracle, b)
    for connect in (False, True):
        ref = oa.compose(ob, connect=connect, compose_filter=flt.value).to_flat()
        got = da.compose(db, ComposeConfig(flt, connect=connect)).to_flat()
        assert_flat_identical(got, ref, f"wide compose {flt.name} connect={connect}")


@pytest.mark.parametrize("connect", [False, True])
def test_compose_large_pair_switches_to_wide_driver(gpu_ctx, oracle, connect):
    """A 110 k-state composition through the default compose(): the wave kernel gives up after its first arenas and the
    wide driver finishes; one-side-sorted operands (forced match side) go the same way."""
    a = _swap_labels(synth.make_transducer(2000, 3, 12, 0.2, seed=3, p_final=0.05))
    b = synth.make_transducer(50, 12, 12, 0.05, seed=103, p_final=0.05)
    ref = to_oracle(oracle, a).compose(to_oracle(oracle, b), connect=connect).to_flat()
    assert ref["n_states"] > 50_000
    got = to_device(a).compose(to_device(b), ComposeConfig(connect=connect)).to_flat()
    assert_flat_identical(got, ref, f"large compose connect={connect}")
    assert gpu_ctx.stats()["compose_states"] > 50_000
    b_unsorted = dict(b)
    b_unsorted["props"] = b["props"] & ~synth.I_LABEL_SORTED | 0x0000_0000_2000_0000  # NOT_I_LABEL_SORTED: match on fst1 only
    ref2 = to_oracle(oracle, a).compose(to_oracle(oracle, b_unsorted), connect=connect).to_flat()
    got2 = to_device(a).compose(to_device(b_unsorted), ComposeConfig(connect=connect)).to_flat()
    assert_flat_identical(got2, ref2, "large compose, output-side matching only")


def test_wide_driver_grows_its_arena(gpu_ctx, oracle, monkeypatch):
    """The wide driver started from a 64-state arena: levels that hold more new tuples than the table has slots (the
    probe sequence is cut off, the attempt given up) and segments that do not fit are retried with 4x until the result
    fits — look-ahead and plain composition still equal the oracle."""
    monkeypatch.setenv("WFST_WIDE_EST_STATES", "64")
    a = _swap_labels(synth.make_transducer(300, 3, 8, 0.2, seed=1, p_final=0.05))
    b = synth.make_transducer(20, 8, 8, 0.05, seed=101, p_final=0.05)
    oa, ob = to_oracle(oracle, a), to_oracle(oracle, b)
    gpu_ctx.reset_stats()
    la = rustfst_amd.LookAhead(to_device(a))
    out = la.compose(la.relabel(to_device(b)))
    assert gpu_ctx.stats()["compose_retries"] >= 3
    assert_flat_identical(out.to_flat(), oa.compose_lookahead(ob).to_flat(), "look-ahead, grown arena")
    gpu_ctx.reset_stats()
    got = to_device(a).compose(to_device(b))
    assert gpu_ctx.stats()["compose_retries"] >= 3
    assert_flat_identical(got.to_flat(), oa.compose(ob).to_flat(), "compose, grown arena")


@pytest.mark.parametrize("group,batch,est", [("8", "1", "256"), ("8", "5", "0"), ("16", "2", "256"), ("16", "8", "0"), ("64", "3", "256"),
                                             ("8", "4", "-64"), ("16", "auto", "-256"), ("4", "1", "256"), ("4", "6", "0"), ("4", "auto", "-64"),
                                             ("2", "1", "256"), ("2", "5", "0"), ("2", "auto", "-256")])
def test_wide_driver_lane_groups_and_level_batches(gpu_ctx, oracle, monkeypatch, group, batch, est):
    """The wide driver with 2, 4, 8, 16 or 64 lanes per composed state and 1..8 levels queued per look at the control block
    (level ranges, overflow status and finished-level count live on the device), from a small arena that has to grow in
    the middle of a batch (before the level that is not going to fit, or — foresight off — after it has overflowed) and
    from the default one: plain and look-ahead composition equal the oracle — also with states
    that have more arcs than a lane group (several chunks per state) and with levels queued behind the last one."""
    monkeypatch.setenv("WFST_WIDE_GROUP", group)
    if batch != "auto":
        monkeypatch.setenv("WFST_WIDE_BATCH", batch)
    if est.startswith("-"):  # the arena is only grown AFTER a level has overflowed (in the middle of a batch)
        monkeypatch.setenv("WFST_WIDE_NO_FORESIGHT", "1")
        est = est[1:]
    if est != "0":
        monkeypatch.setenv("WFST_WIDE_EST_STATES", est)
    monkeypatch.setenv("WFST_COMPOSE_PATH", "wide")
    monkeypatch.setenv("WFST_LOOKAHEAD_PATH", "wide")
    for (n1, f1, n2, f2, sigma) in [(300, 3, 20, 8, 8), (40, 40, 12, 30, 6)]:
        a = _swap_labels(synth.make_transducer(n1, f1, sigma, 0.2, seed=1, p_final=0.05))
        b = synth.make_transducer(n2, f2, sigma, 0.05, seed=101, p_final=0.05)
        oa, ob = to_oracle(oracle, a), to_oracle(oracle, b)
        la = rustfst_amd.LookAhead(to_device(a))
        out = la.compose(la.relabel(to_device(b)))
        assert_flat_identical(out.to_flat(), oa.compose_lookahead(ob).to_flat(), f"look-ahead, group {group} batch {batch}")
        for connect in (False, True):
            got = to_device(a).compose(to_device(b), ComposeConfig(connect=connect))
            assert_flat_identical(got.to_flat(), oa.compose(ob, connect=connect).to_flat(), f"compose, group {group} batch {batch}")


def test_reference_known_answers_reverse_tr_sort_connect(gpu_ctx):
    """The reference's own vectors for the operations around the path (rustfst-python/tests/algorithms/test_reverse.py:4-57,
    test_tr_sort.py:4-97, test_connect.py:4-55) through the GPU path: reverse and tr_sort directly; connect as the trim of a
    composition with the one-state identity-free acceptor of everything (compose(x, sigma*) keeps x's structure)."""
    g = golden("k9_reverse.json")
    assert vbuild(g["fst"]).to_device().reverse().to_vector_fst() == vbuild(g["expected"])
    g = golden("k10_tr_sort.json")
    assert vbuild(g["fst"]).to_device().tr_sort(True).to_vector_fst() == vbuild(g["expected_ilabel"])
    assert vbuild(g["fst"]).to_device().tr_sort(False).to_vector_fst() == vbuild(g["expected_olabel"])
    # connect: compose with a single-state FST that reads every output label of x (olabel l -> l), so the composition is x
    # itself (ids in BFS order = 0, 1, 2 here) and connect=True trims what test_connect.py trims
    g = golden("k8_connect.json")
    x = vbuild(g["fst"])
    x.tr_sort(False)
    sig = VectorFst()
    s0 = sig.add_state()
    sig.set_start(s0)
    sig.set_final(s0, 0.0)
    for l in (2, 4, 5, 6, 8):
        sig.add_tr(s0, Tr(l, l, 0.0, s0))
    got = x.compose(sig, ComposeConfig(connect=True))
    assert got == vbuild(g["expected"])


def test_connect_known_answer_and_oracle(gpu_ctx, oracle):
    """wfst_connect: the reference's test_connect.py:4-55 vector directly, then random FSTs with inaccessible and
    non-coaccessible parts (and without start / without finals) against the oracle: survivors, stable renumbering, arc
    compaction, start state and property word."""
    g = golden("k8_connect.json")
    x = vbuild(g["fst"])
    res = x.connect()
    assert x == vbuild(g["expected"]) and res == vbuild(g["expected"])
    rng = np.random.default_rng(88)
    for k in range(30):
        f = random_fst_flat(rng, int(rng.integers(1, 80)), 3, 4, p_eps_i=0.1, p_final=(0.0, 0.05, 0.3)[k % 3],
                            sort=("ilabel", "none")[k % 2], acyclic=(k % 4 == 0))
        if k % 7 == 3:
            f = dict(f)
            f["start"] = -1
        ref = to_oracle(oracle, f)
        ref.connect()
        assert_flat_identical(to_device(f).connect().to_flat(), ref.to_flat(), f"connect {k}")
    deep = synth.make_transducer(5000, 1, 4, 0.0, seed=4, p_final=0.0005)  # a 5000-state ring: thousands of sweeps
    ref = to_oracle(oracle, deep)
    ref.connect()
    assert_flat_identical(to_device(deep).connect().to_flat(), ref.to_flat(), "connect on a ring")


def test_connect_on_a_deep_chain(gpu_ctx, oracle):
    """connect on a chain of 200 000 states (a long linear acceptor with dead-end side branches, numbered in path order and,
    a second time, in REVERSE path order): the reachability sweeps walk runs of consecutive states in path order, so the
    fixed point needs diameter / 16 sweeps at worst, not one per state.  Result identical to the oracle's."""
    import time
    n = 200_000
    for reverse_ids in (False, True):
        ids = np.arange(n, dtype=np.uint32)[::-1] if reverse_ids else np.arange(n, dtype=np.uint32)
        # state k of the path: one arc to state k + 1; every 10th also has an arc to a dead end (state n + k // 10)
        n_dead = n // 10
        src, dst = [], []
        src.append(ids[:-1]); dst.append(ids[1:])
        dead_from = ids[:n - 1:10][:n_dead]
        src.append(dead_from); dst.append(np.arange(n, n + len(dead_from), dtype=np.uint32))
        src, dst = np.concatenate(src), np.concatenate(dst)
        total = n + n_dead
        order = np.argsort(src, kind="stable")
        src, dst = src[order], dst[order]
        arcs = np.zeros(len(src), dtype=rustfst_amd.TR_DTYPE)
        arcs["ilabel"] = arcs["olabel"] = 1 + (np.arange(len(src)) % 7)
        arcs["weight"] = 0.5
        arcs["nextstate"] = dst
        offsets = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=total))]).astype(np.uint32)
        finals = np.full(total, np.inf, dtype=np.float32)
        finals[ids[-1]] = 1.0
        flat = dict(n_states=total, start=int(ids[0]), offsets=offsets, arcs=arcs, finals=finals, props=0)
        ref = to_oracle(oracle, flat)
        ref.connect()
        t0 = time.perf_counter()
        got = to_device(flat).connect().to_flat()
        assert time.perf_counter() - t0 < 20.0
        assert got["n_states"] == n
        assert_flat_identical(got, ref.to_flat(), f"connect on a chain, reverse_ids={reverse_ids}")


def test_rm_epsilon_known_answer_and_oracle(gpu_ctx, oracle):
    """wfst_rm_epsilon: the reference's test_rm_epsilon.py:4-54 vector, then epsilon-rich random FSTs (acyclic and cyclic
    epsilon structure, epsilon self-loops, states that are rewritten and states that only lose their arcs, weights on the
    1/512 grid) against the oracle's restatement: states, arc ORDER (the reference rewrites states in dependency order and
    reads the rewritten successors), combined weights, finals, property word."""
    g = golden("k11_rm_epsilon.json")
    x = vbuild(g["fst"])
    res = x.rm_epsilon()
    assert x == vbuild(g["expected"]) and res == vbuild(g["expected"])
    rng = np.random.default_rng(4711)
    for k in range(60):
        f = random_fst_flat(rng, int(rng.integers(1, 40)), 3, 3, p_eps_i=(0.3, 0.6)[k % 2], p_eps_o=(0.3, 0.6)[k % 2],
                            p_final=0.3, acyclic=(k % 3 == 0), sort=("none", "ilabel")[k % 2])
        if k % 11 == 5:
            f = dict(f)
            f["start"] = -1
        ref = to_oracle(oracle, f)
        ref.rm_epsilon()
        assert_flat_identical(to_device(f).rm_epsilon().to_flat(), ref.to_flat(), f"rm_epsilon {k}")
    big = synth.make_transducer(3000, 3, 5, 0.25, seed=12, p_final=0.02)  # a quarter of the arcs epsilon:epsilon below
    arcs = big["arcs"].copy()
    arcs["olabel"] = np.where(arcs["ilabel"] == 0, 0, arcs["olabel"])
    big = dict(big); big["arcs"] = arcs; big["props"] = 0
    ref = to_oracle(oracle, big)
    ref.rm_epsilon()
    assert_flat_identical(to_device(big).rm_epsilon().to_flat(), ref.to_flat(), "rm_epsilon on 3000 states")
    # one epsilon component of a few hundred states (every rewrite walks a closure of that size: the one-wave-per-state
    # kernel with hashed lookups; rewrites inside an epsilon cycle are sequential, in the reference's order)
    dense = synth.make_transducer(400, 4, 3, 0.6, seed=12, p_final=0.02)
    arcs = dense["arcs"].copy()
    arcs["olabel"] = np.where(arcs["ilabel"] == 0, 0, arcs["olabel"])
    dense = dict(dense); dense["arcs"] = arcs; dense["props"] = 0
    ref = to_oracle(oracle, dense)
    ref.rm_epsilon()
    assert_flat_identical(to_device(dense).rm_epsilon().to_flat(), ref.to_flat(), "rm_epsilon, one large epsilon component")


def test_rm_epsilon_closure_of_100k_states(gpu_ctx, oracle):
    """An epsilon closure of 131 071 states: a binary tree of epsilon:epsilon arcs under the start state whose inner nodes
    have no other incoming arc (so they are never rewritten themselves), 65 536 leaves with one labelled arc each to a
    final sink.  The start state's rewrite walks the whole tree depth first; its 65 536 new arcs, their order, the combined
    weights and the final weight are the oracle's (the scratch slice is regrown until closure, stack and arcs fit)."""
    depth = 16
    n_tree = 2 ** (depth + 1) - 1
    first_leaf = 2 ** depth - 1
    sink = n_tree
    n = n_tree + 1
    rng = np.random.default_rng(99)
    deg = np.zeros(n, dtype=np.uint32)
    deg[:first_leaf] = 2
    deg[first_leaf:n_tree] = 1
    offsets = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint32)
    arcs = np.zeros(int(offsets[-1]), dtype=rustfst_amd.TR_DTYPE)
    inner = np.arange(first_leaf)
    arcs["nextstate"][offsets[inner]] = 2 * inner + 1
    arcs["nextstate"][offsets[inner] + 1] = 2 * inner + 2
    leaves = np.arange(first_leaf, n_tree)
    arcs["ilabel"][offsets[leaves]] = 1 + (leaves - first_leaf) % 50000  # some labels repeat: those arcs are (+)-combined
    arcs["olabel"][offsets[leaves]] = arcs["ilabel"][offsets[leaves]]
    arcs["nextstate"][offsets[leaves]] = sink
    arcs["weight"] = (rng.integers(0, 2048, len(arcs)) / 512.0).astype(np.float32)
    finals = np.full(n, np.inf, dtype=np.float32)
    finals[sink] = 0.5
    finals[first_leaf + 7] = 1.25  # a final state inside the closure
    flat = dict(n_states=n, start=0, offsets=offsets, arcs=arcs, finals=finals, props=0)
    ref = to_oracle(oracle, flat)
    ref.rm_epsilon()
    want = ref.to_flat()
    got = to_device(flat).rm_epsilon().to_flat()
    assert want["n_states"] == 2 and len(want["arcs"]) == 50000  # start + sink survive connect
    assert_flat_identical(got, want, "rm_epsilon with a 131k-state closure")
