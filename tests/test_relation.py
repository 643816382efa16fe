"""The brute-force weighted relation (relation_ref.py): the evaluator against answers known by eye and against path
enumeration, its sensitivity to one wrong weight or target, and every restatement that runs on the CPU (the OracleFst
methods and the *_ref functions of oracle/model) against the specification of its operation.  No GPU.  A failure in
the last part means a restatement computes the wrong meaning, whatever bit-parity with the device says."""
import copy

import numpy as np
import pytest

import relation_ref as R
from helpers import _oracle_dist, enumerate_paths
from isomorphic_ref import invert as invert_ref
from oracle.model import (Unsupported, closure_ref, concat_ref, connect, determinize_ref, flat_to_fst, fold_ref,
                          fst_to_flat, minimize_ref, optimize_ref, push_ref, reweight_ref, state_sort_ref, to_flat,
                          to_oracle, top_sort_ref, tr_unique, union_ref)
from oracle.model.optimize import tr_sum
from relation_ref import EPS, INF, S

FILTER_VALUE = dict(AUTOFILTER=0, NULLFILTER=1, TRIVIALFILTER=2, SEQUENCEFILTER=3, ALTSEQUENCEFILTER=4, MATCHFILTER=5,
                    NOMATCHFILTER=6)


# ================================================================ (a) the evaluator
def test_relation_equals_path_enumeration_on_acyclic_inputs():
    def strip(t):
        return tuple(a for a in t if a)
    for fam in ("acyclic", "acceptor", "acyclic_neg", "acceptor_neg"):
        for seed in range(R.SEEDS):
            f = R.small(fam, seed)
            want = {}
            for w, il, ol in enumerate_paths(f):
                k = (strip(il), strip(ol))
                if k[0] in S and k[1] in S:
                    want[k] = min(w, want.get(k, INF))
            assert R.small_relation(fam, seed) == want, (fam, seed)
            for k in list(want)[:3] + [((1, 2, 1), (2,))]:
                assert R.weight_of(f, *k) == want.get(k, INF)
            total = min((w for w, _, _ in enumerate_paths(f)), default=INF)
            assert R.best_total(f) == total


def test_hand_built_machines():
    one = (1,)
    # an epsilon self-loop of weight 0 changes nothing
    f = R.make(2, 0, [[(0, 0, 0.0, 0), (1, 1, 0.5, 1)], []], [INF, 0.25])
    assert R.relation(f) == {(one, one): 0.75} and R.weight_of(f, one, one) == 0.75 and R.best_total(f) == 0.75
    # ... nor does one of weight 0.25: going round never helps
    f = R.make(2, 0, [[(0, 0, 0.25, 0), (1, 1, 0.5, 1)], []], [INF, 0.25])
    assert R.relation(f) == {(one, one): 0.75}
    # an output-only cycle: reads 1 once, writes 2 as often as it likes, 0.5 a turn
    f = R.make(2, 0, [[(1, 0, 1.0, 1)], [(0, 2, 0.5, 1)]], [INF, 0.0])
    assert R.relation(f) == {(one, EPS): 1.0, (one, (2,)): 1.5, (one, (2, 2)): 2.0, (one, (2, 2, 2)): 2.5}
    assert R.weight_of(f, one, (2,) * 6) == 4.0 and R.weight_of(f, one, (2, 1)) == INF
    # no start state, no states
    assert R.relation(R.make(2, None, [[(1, 1, 0.0, 1)], []], [0.0, 0.0])) == {}
    assert R.relation(R.make(0, None, [], [])) == {} and R.best_total(R.make(0, None, [], [])) == INF
    assert R.weight_of(R.make(0, None, [], []), EPS, EPS) == INF
    # a final start state
    f = R.make(1, 0, [[(2, 1, 0.25, 0)]], [1.5])
    assert R.relation(f) == {(EPS, EPS): 1.5, ((2,), one): 1.75, ((2, 2), (1, 1)): 2.0, ((2, 2, 2), (1, 1, 1)): 2.25}
    # two paths for one pair: the lighter one; a negative weight on an acyclic machine
    f = R.make(3, 0, [[(1, 2, 1.0, 2), (1, 0, 0.25, 1)], [(0, 2, -0.5, 2)], []], [INF, INF, 0.0])
    assert R.relation(f) == {(one, (2,)): -0.25} and R.best_total(f) == -0.25
    # the product by definition: a writes 3, b reads 3; a's output epsilon and b's input epsilon move alone
    a = R.make(3, 0, [[(1, 0, 0.25, 1)], [(2, 3, 0.5, 2)], []], [INF, INF, 0.0])
    b = R.make(3, 0, [[(0, 1, 1.0, 1)], [(3, 2, 0.25, 2)], []], [INF, INF, 0.5])
    assert R.relation(R.naive_product(a, b)) == {((1, 2), (1, 2)): 2.5}
    assert R.weight_of(R.Product(a, b), (1, 2), (1, 2)) == 2.5
    # the specifications' own arithmetic
    Rel = {(one, EPS): 1.0, (EPS, EPS): 0.5}
    assert R.concat_rel(Rel, Rel)[((1, 1), EPS)] == 2.0 and R.concat_rel(Rel, Rel)[(one, EPS)] == 1.5
    assert R.closure_rel(Rel, False)[((1, 1, 1), EPS)] == 3.0 and R.closure_rel(Rel, True)[(EPS, EPS)] == 0.0
    assert R.closure_rel(Rel, False)[(EPS, EPS)] == 0.5


# ================================================================ (b) sensitivity
def _mutants(f, k, dead):
    """f with arc k one grid step lighter; f with arc k retargeted to the state `dead`, which reaches no final state"""
    lighter = dict(f, arcs=f["arcs"].copy())
    lighter["arcs"]["weight"][k] -= 1.0 / R.GRID
    rows = [[tuple(a) for a in f["arcs"][f["offsets"][s]:f["offsets"][s + 1]]] for s in range(f["n_states"])] + [[]]
    away = R.make(f["n_states"] + 1, f["start"], rows, list(f["finals"]) + [INF])
    away["arcs"]["nextstate"][k] = dead
    return lighter, away


def test_one_wrong_weight_or_target_changes_the_relation():
    """On 30 seeded inputs with a non-empty relation: an arc on a best path of some pair of S x S (found by brute force:
    without the arc the relation is another) made one grid step lighter, or sent to a state that reaches no final state,
    gives another relation, every time.  This is why an equal relation means something."""
    seen = 0
    for fam in ("cyclic", "acyclic", "acceptor"):
        for seed in range(2, R.SEEDS):
            f, rel = R.small(fam, seed), R.small_relation(fam, seed)
            if not rel or seen == 30:
                continue
            on_best = []
            for k in range(len(f["arcs"])):
                if f["arcs"]["weight"][k] >= 0.25:  # (a lighter arc stays non-negative: no negative cycle)
                    gone = dict(f, arcs=f["arcs"].copy())
                    gone["arcs"]["weight"][k] = np.inf
                    if R.relation(gone) != rel:
                        on_best.append(k)
            if not on_best:
                continue
            k = on_best[seed % len(on_best)]
            lighter, away = _mutants(f, k, f["n_states"])
            assert R.relation(lighter) != rel, (fam, seed, k, "lighter")
            assert R.relation(away) != rel, (fam, seed, k, "retargeted")
            x, y = next(p for p in rel if R.relation(lighter).get(p) != rel[p])
            assert R.weight_of(lighter, x, y) < R.weight_of(f, x, y)
            seen += 1
    print(f"sensitivity: {seen} of 30 mutations seen")
    assert seen == 30


# ================================================================ the families are not vacuous
@pytest.mark.parametrize("fam", R.FAMILIES)
def test_families_are_not_vacuous(fam):
    for sort, fan in (("ilabel", 1), ("none", 1)):
        rels = [R.small_relation(fam, s, sort, fan) for s in range(R.SEEDS)]
        big, empty, epseps = R.assert_not_vacuous(rels, f"{fam} {sort}")
        print(f"{fam} ({sort}): {big:.0%} with >= 3 pairs, {empty} empty, {epseps} with (eps, eps)")
    for base in (100, 200):
        assert sum(bool(R.small_relation(fam, base + s)) for s in range(R.SEEDS)) >= R.SEEDS // 2


@pytest.mark.parametrize("fam", R._ANY)
def test_compose_pairs_are_not_vacuous(fam):
    rels = [R.relation(R.naive_product(*R.compose_pair(fam, s))) for s in range(R.SEEDS)]
    share = sum(bool(r) for r in rels) / len(rels)
    print(f"compose {fam}: {share:.0%} of the pairs have a non-empty product, {sum(len(r) >= 3 for r in rels)} with >= 3")
    assert share >= 0.5 and any(not r for r in rels) and any((EPS, EPS) in r for r in rels)


# ================================================================ (c) the restatements
def _rows(op, flat):
    fst = flat_to_fst(flat)
    op(fst)
    return fst_to_flat(fst)


def apply_ref(oracle, op, ins, extra):
    """the CPU restatement of `op`"""
    f = ins[0]
    o = lambda x: to_oracle(oracle, x)  # noqa: E731
    if op.startswith("compose_"):
        return o(ins[0]).compose(o(ins[1]), compose_filter=FILTER_VALUE[op[8:]]).to_flat()
    if op == "lookahead":
        return o(ins[0]).compose_lookahead(o(ins[1])).to_flat()
    if op == "rm_epsilon":
        return o(f).rm_epsilon().to_flat()
    if op == "reverse":
        return o(f).reverse().to_flat()
    if op in ("project_i", "project_o"):
        return o(f).project(op == "project_o").to_flat()
    if op in ("tr_sort_i", "tr_sort_o"):
        x = o(f)
        x.tr_sort(op == "tr_sort_o")
        return x.to_flat()
    if op == "connect":
        x = o(f)
        x.connect()
        assert R.relation(_rows(connect, f)) == R.relation(x.to_flat())  # (the model's connect too)
        return x.to_flat()
    if op == "tr_sum":
        return _rows(tr_sum, f)
    if op == "tr_unique":
        return _rows(tr_unique, f)
    if op == "optimize":
        return optimize_ref(f, oracle)
    if op == "top_sort":
        return fst_to_flat(top_sort_ref(flat_to_fst(f)))
    if op == "state_sort":
        return fst_to_flat(state_sort_ref(flat_to_fst(f), [int(v) for v in extra]))
    if op == "invert":
        return fst_to_flat(invert_ref(flat_to_fst(f)))
    if op == "determinize":
        ref = determinize_ref(f)
        assert R.relation(o(f).determinize_fsa().to_flat()) == R.relation(ref)  # (the C++ oracle's too)
        return ref
    if op == "minimize":
        return minimize_ref(f)
    if op in ("reweight_i", "reweight_f"):
        return to_flat(reweight_ref(f, extra, op == "reweight_f"))
    if op.startswith("push_"):
        to_final = op.startswith("push_f")
        return to_flat(push_ref(f, _oracle_dist(oracle, f, to_final), to_final, op.endswith("_total")))
    fsts = [flat_to_fst(x) for x in ins]
    if op in ("union", "union_list"):
        return fst_to_flat(fold_ref(union_ref, fsts))
    if op in ("concat", "concat_list"):
        return fst_to_flat(fold_ref(concat_ref, fsts))
    if op in ("closure_plus", "closure_star"):
        return fst_to_flat(closure_ref(copy.deepcopy(fsts[0]), 0 if op == "closure_star" else 1))
    raise KeyError(op)


@pytest.mark.parametrize("op,fam", R.CASES)
def test_restatement_computes_the_specified_relation(oracle, op, fam):
    for seed in R.seeds_for(op, fam):
        try:
            R.check_case(op, fam, seed, lambda op, ins, extra: apply_ref(oracle, op, ins, extra))
        except Unsupported as e:
            pytest.fail(f"{op} on {fam} seed {seed} is refused: {e}")


@pytest.mark.parametrize("fam", R._POS)
def test_shortest_path_and_distance_restatements(oracle, fam):
    for seed in range(R.SEEDS):
        f = R.small(fam, seed)
        R.check_shortest_path(to_oracle(oracle, f).shortest_path().to_flat(), f, f"shortest_path {fam} {seed}")
        R.check_shortest_path(to_oracle(oracle, f).shortest_path_canonical().to_flat(), f, f"canonical {fam} {seed}")
        for to_final in (True, False):  # (as push_weights asks: forward for to_final, reverse for to_initial)
            got = np.asarray(_oracle_dist(oracle, f, to_final), np.float64)
            want = R.distances(f, reverse=not to_final)
            assert np.array_equal(got, want[:len(got)]) and np.all(want[len(got):] == INF), (fam, seed, to_final)


def test_fused_string_batch_restatement(oracle):
    from oracle import oracle_py
    for seed in range(R.SEEDS):
        t = R.small("cyclic", seed, "ilabel", 2)
        strs = [x for x in S if x]
        accs = [to_oracle(oracle, R.string_acceptor(x)) for x in strs]
        outs, _, _ = oracle_py.compose_shortest_path_batch(accs, to_oracle(oracle, t))
        for x, out in zip(strs, outs):
            R.check_string_path(out.to_flat(), x, t, f"seed {seed} string {x}")
