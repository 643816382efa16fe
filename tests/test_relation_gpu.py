"""What the device returns, against the brute-force weighted relation (relation_ref.py): the same specifications as
test_relation.py checks on the CPU restatements, here on to_flat() of every device result -- the small families by
default and under every pinned route (the route read from the family's counters), the list forms with 64 items per call,
and one mid-size lattice on sampled strings that leaves the one-workgroup kernels without a knob.  Every comparison is
== on float64 (the exactness rule of relation_ref.py).  With test_relation.py green, a failure here is the kernel's.

Cases and routes as recorded on an MI355X (the shares of non-vacuous inputs are tabulated in relation_ref.py):

  every operation of relation_ref.OPS on the families listed there (95 pairs), 24 seeds each: default routes
  compose under the five filters, pinned, on cyclic / acyclic / acyclic_neg, 24 each: wave: wave_first 1, never
      switched_wide; wide: no launch of the wave kernel
  look-ahead compose, pinned, same families, 24 each: wave_answered 1 / wide_items 1
  determinize, minimize, optimize, pinned, on acceptor / acceptor_neg, 24 each: narrow: no wide level; wide: every level
  top_sort, pinned, on the four acyclic families, 24 each: narrow launches only / wide launches only
  shortest_path and shortest_path_batch on cyclic / acyclic, 24, WFST_SP1_DEVICE unset, 0, 1: n1_in_kernel 1 and 24; 0
  shortest_distance, both directions, on cyclic / acyclic, 24: no counter
  fused string batch, 24 transducers x 14 strings: cyclic (input epsilons): 28 strings by the string kernel;
      cyclic_oeps: all 336, pair levels 100 under WFST_STRING_PAIR=1 and 0 under =0
  rm_epsilon / tr_sum / tr_unique / top_sort / determinize / minimize / optimize _batch, 64 items per call: 64 of 64 in
      the batch kernel; 58 of 64 for rm_epsilon on cyclic; optimize: the acceptors (a transducer goes alone)
  compose_batch under the five filters, 64 pairs per call: 1 launch, 64 in the kernel
  union_list and concat_list, 4 calls of 64 items per family: no counter
  the lattice (647 states), 88 sampled pairs per operation, 15 operations: determinize 3 of 6 levels wide; top_sort
      widest level 300, 8 wide launches; compose switched_wide 1; minimize narrow; the others keep no counter"""
import functools

import numpy as np
import pytest

import relation_ref as R
from helpers import to_device
from relation_ref import EPS, INF, S

pytestmark = pytest.mark.gpu

BATCH = 64


def _lib():
    import rustfst_amd
    return rustfst_amd


def apply_dev(ctx, op, ins, extra):
    """`op` on the device, the result as flat arrays"""
    A = _lib()
    d = [to_device(f, ctx) for f in ins]
    f = d[0]
    if op.startswith("compose_"):
        return f.compose(d[1], A.ComposeConfig(A.ComposeFilter[op[8:]])).to_flat()
    if op == "lookahead":
        la = A.LookAhead(f)
        return la.compose(la.relabel(d[1])).to_flat()
    if op in ("rm_epsilon", "reverse", "connect", "tr_sum", "tr_unique", "optimize", "top_sort", "invert", "determinize",
              "minimize"):
        return getattr(f, op)().to_flat()
    if op in ("project_i", "project_o"):
        return f.project(A.ProjectType.PROJECT_OUTPUT if op == "project_o" else A.ProjectType.PROJECT_INPUT).to_flat()
    if op in ("tr_sort_i", "tr_sort_o"):
        return f.tr_sort(op == "tr_sort_i").to_flat()
    if op == "state_sort":
        return f.state_sort(extra).to_flat()
    if op in ("reweight_i", "reweight_f"):
        kind = A.ReweightType.REWEIGHT_TO_FINAL if op == "reweight_f" else A.ReweightType.REWEIGHT_TO_INITIAL
        return f.reweight(extra, kind).to_flat()
    if op.startswith("push_"):
        kind = A.ReweightType.REWEIGHT_TO_FINAL if op.startswith("push_f") else A.ReweightType.REWEIGHT_TO_INITIAL
        return f.push_weights(kind, A.PushWeightsConfig(remove_total_weight=op.endswith("_total"))).to_flat()
    if op == "union":
        return f.union(d[1]).to_flat()
    if op == "concat":
        return f.concat(d[1]).to_flat()
    if op == "union_list":
        return A.union_list(d).to_flat()
    if op == "concat_list":
        return A.concat_list(d).to_flat()
    if op in ("closure_plus", "closure_star"):
        return f.closure(A.ClosureType.CLOSURE_STAR if op == "closure_star" else A.ClosureType.CLOSURE_PLUS).to_flat()
    raise KeyError(op)


def run_cases(ctx, op, fam, after=None):
    for seed in R.seeds_for(op, fam):
        R.check_case(op, fam, seed, lambda op, ins, extra: apply_dev(ctx, op, ins, extra))
        if after is not None:
            after(R.inputs_of(op, fam, seed)[0])


# ================================================================ the small families, default routes
@pytest.mark.parametrize("op,fam", R.CASES)
def test_device_result_has_the_specified_relation(gpu_ctx, op, fam):
    run_cases(gpu_ctx, op, fam)


@pytest.mark.parametrize("fam", R.FAMILIES)
def test_families_are_not_vacuous(fam):
    R.assert_not_vacuous([R.small_relation(fam, s) for s in range(R.SEEDS)], fam)
    if fam in R._ANY:
        rels = [R.relation(R.naive_product(*R.compose_pair(fam, s))) for s in range(R.SEEDS)]
        assert sum(bool(r) for r in rels) >= R.SEEDS // 2 and any(not r for r in rels) and any((EPS, EPS) in r for r in rels)


# ================================================================ pinned routes
@pytest.mark.parametrize("path", ["wave", "wide"])
@pytest.mark.parametrize("fam", R._ANY)
def test_compose_pinned(gpu_ctx, monkeypatch, fam, path):
    monkeypatch.setenv("WFST_COMPOSE_PATH", path)

    def route(ins):
        # compose zeroes the counters of this family when a call begins (they describe the context's LAST call) and the
        # pinned wide driver touches none of them: no launch of the wave kernel is all that shows it ran
        st = gpu_ctx.compose_path_stats()
        wave = st["wave_first"] + st["relaunch_states"] + st["relaunch_arcs"] + st["relaunch_hash"]
        assert (wave >= 1 and st["switched_wide"] == 0) if path == "wave" else wave == 0, (path, st)
    for flt in R.COMPOSE_FILTERS:
        run_cases(gpu_ctx, "compose_" + flt, fam, route)


@pytest.mark.parametrize("path", ["wave", "wide"])
@pytest.mark.parametrize("fam", R._ANY)
def test_lookahead_pinned(gpu_ctx, monkeypatch, fam, path):
    monkeypatch.setenv("WFST_LOOKAHEAD_PATH", path)

    def route(ins):
        st = gpu_ctx.lookahead_stats()
        assert st["items"] == 1 and st["items_no_start"] == 0, st
        assert (st["wave_answered"], st["wide_items"]) == ((1, 0) if path == "wave" else (0, 1)), (path, st)
    run_cases(gpu_ctx, "lookahead", fam, route)


@pytest.mark.parametrize("path", ["narrow", "wide"])
@pytest.mark.parametrize("fam", R._ACC)
def test_determinize_and_minimize_pinned(gpu_ctx, monkeypatch, fam, path):
    monkeypatch.setenv("WFST_DETERMINIZE_PATH", path)
    monkeypatch.setenv("WFST_MINIMIZE_PATH", path)

    def det_route(ins):
        st = gpu_ctx.determinize_stats()
        assert st["levels"] >= 1, st
        assert (st["wide_levels"] == 0 and st["narrow_launches"] >= 1) if path == "narrow" else \
            (st["narrow_launches"] == 0 and st["wide_levels"] == st["levels"]), (path, st)

    ran = dict(narrow=0, wide=0)

    def min_route(ins):  # (an input that accepts nothing peels no level, and a word that holds ACYCLIC needs no cycle check)
        st = gpu_ctx.minimize_stats()
        ran["narrow"] += st["narrow_launches"] + st["check_narrow_launches"]
        ran["wide"] += st["wide_levels"] + st["check_wide_levels"]
    run_cases(gpu_ctx, "determinize", fam, det_route)
    run_cases(gpu_ctx, "minimize", fam, min_route)
    assert ran[path] >= 1 and ran["wide" if path == "narrow" else "narrow"] == 0, (path, ran)
    run_cases(gpu_ctx, "optimize", fam)


@pytest.mark.parametrize("path", ["narrow", "wide"])
@pytest.mark.parametrize("fam", R._DAG)
def test_top_sort_pinned(gpu_ctx, monkeypatch, fam, path):
    monkeypatch.setenv("WFST_TOP_SORT_PATH", path)

    def route(ins):
        st = gpu_ctx.top_sort_stats()
        assert st["levels"] >= 1 and st["cyclic"] == 0, st
        assert (st["wide_launches"] == 0 and st["narrow_launches"] >= 1) if path == "narrow" else \
            (st["narrow_launches"] == 0 and st["wide_launches"] >= 1), (path, st)
    run_cases(gpu_ctx, "top_sort", fam, route)


# ================================================================ shortest path, shortest distance
@pytest.mark.parametrize("sp1", [None, "0", "1"])
@pytest.mark.parametrize("fam", R._POS)
def test_shortest_path(gpu_ctx, monkeypatch, fam, sp1):
    """shortest_path (n = 1), alone and as a batch, by default and under WFST_SP1_DEVICE=0 / 1 (and WFST_NBEST_DEVICE with it:
    it is read for n > 1 only, which the brute force of helpers.py covers)"""
    A = _lib()
    if sp1 is not None:
        monkeypatch.setenv("WFST_SP1_DEVICE", sp1)
        monkeypatch.setenv("WFST_NBEST_DEVICE", sp1)
    flats = R.family(fam)
    devs = [to_device(f, gpu_ctx) for f in flats]
    for seed, (f, d) in enumerate(zip(flats, devs)):
        R.check_shortest_path(d.shortest_path().to_flat(), f, f"shortest_path {fam} {seed}")
        st = gpu_ctx.small_path_stats()
        assert st["n1_in_kernel"] == (0 if sp1 == "0" else 1) and st["n1_handed_back"] == 0, (sp1, st)
    outs = A.shortest_path_batch(devs)
    st = gpu_ctx.small_path_stats()
    assert st["n1_in_kernel"] == (0 if sp1 == "0" else len(devs)) and st["n1_handed_back"] == 0, (sp1, st)
    for seed, (f, o) in enumerate(zip(flats, outs)):
        R.check_shortest_path(o.to_flat(), f, f"shortest_path_batch {fam} {seed}")


@pytest.mark.parametrize("fam", R._POS)
def test_shortest_distance(gpu_ctx, fam):
    for seed, f in enumerate(R.family(fam)):
        d = to_device(f, gpu_ctx)
        assert np.array_equal(d.shortest_distance().astype(np.float64), R.distances(f)), (fam, seed, "forward")
        back = d.shortest_distance(reverse=True).astype(np.float64)
        assert np.array_equal(back, R.distances(f, reverse=True)), (fam, seed, "reverse")


# ================================================================ the fused string batch that bench.py times
@pytest.mark.parametrize("pair", ["0", "1"])
@pytest.mark.parametrize("fam", ["cyclic", "cyclic_oeps"])
def test_fused_string_batch(gpu_ctx, monkeypatch, fam, pair):
    """compose_shortest_path_batch of the 14 non-empty strings of S against every transducer of the family: input epsilons
    (cyclic) send the strings to the wave kernel, none (cyclic_oeps) to the string kernel, with its pair levels on and off"""
    A = _lib()
    monkeypatch.setenv("WFST_STRING_PAIR", pair)
    strs = [x for x in S if x]
    accs = A.DeviceFst.upload_many([R.string_acceptor(x) for x in strs], gpu_ctx)
    found = pairs = answered = 0
    for seed in range(R.SEEDS):
        t = R.small(fam, seed, "ilabel", 2)
        outs, _ = A.compose_shortest_path_batch(accs, to_device(t, gpu_ctx))
        st, pc = gpu_ctx.compose_path_stats(), gpu_ctx.string_pair_counts()
        if fam == "cyclic_oeps":
            assert st["string_answered"] + st["string_handed_back"] == len(strs), st
        elif np.any(t["arcs"]["ilabel"] == 0):
            assert st["string_answered"] == 0 and st["wave_first"] >= 1, st
        assert pair == "1" or (pc["pair_levels"] == 0 and pc["pair_splits"] == 0), pc
        pairs += pc["pair_levels"]
        answered += st["string_answered"]
        for x, o in zip(strs, outs):
            found += R.check_string_path(o.to_flat(), x, t, f"{fam} seed {seed} string {x}")
    print(f"fused batch {fam} WFST_STRING_PAIR={pair}: {found} of {R.SEEDS * len(strs)} strings accepted, "
          f"{answered} by the string kernel, {pairs} pair levels")
    assert found >= R.SEEDS * len(strs) // 4
    if fam == "cyclic_oeps":
        assert answered > 0
        assert (pairs > 0) == (pair == "1"), f"WFST_STRING_PAIR={pair}: {pairs} pair levels over the family"


# ================================================================ the list forms, 64 items per call
def _batch_inputs(op, fam):
    seeds = R.seeds_for(op, fam, BATCH)
    return [R.inputs_of(op, fam, s) for s in seeds]


def _check_items(op, fam, cases, outs):
    wants = []
    for k, ((ins, _), out) in enumerate(zip(cases, outs)):
        got, want = R.relation(out.to_flat()), R.expected(op, ins)
        assert got == want, f"{op}_batch on {fam} item {k}: " + R.diff(got, want)
        R.postconditions(op, ins, out.to_flat())
        wants.append(want)
    # the 64 seeds of a list are more than the 24 the family test looks at: the same conditions on what was compared
    if op.startswith("compose_"):
        assert sum(bool(w) for w in wants) >= len(wants) // 2 and any(not w for w in wants), f"{op}_batch on {fam}: vacuous"
    else:  # (optimize refuses the transducer families' one member that accepts nothing: see relation_ref.supported)
        transducers = op == "optimize" and fam in ("acyclic", "acyclic_neg")
        R.assert_not_vacuous(wants, f"{op}_batch on {fam}", need_empty=not transducers)


BATCH_CASES = [(op, fam) for op in ("rm_epsilon", "tr_sum", "tr_unique", "optimize", "top_sort", "determinize", "minimize")
               for fam in R.OPS[op]]


@pytest.mark.parametrize("op,fam", BATCH_CASES)
def test_batch_forms(gpu_ctx, op, fam):
    A = _lib()
    cases = _batch_inputs(op, fam)
    devs = [to_device(ins[0], gpu_ctx) for ins, _ in cases]
    outs, flags = getattr(A, op + "_batch")(devs, **{("want_flags" if op == "determinize" else "return_in_kernel"): True})
    assert len(outs) == BATCH
    print(f"{op}_batch {fam}: {int(np.sum(flags))} of {BATCH} items in the batch kernel")
    if op == "optimize" and fam in ("acyclic", "acyclic_neg"):  # (a transducer takes the label encoding of the single call)
        assert not any(flag for (ins, _), flag in zip(cases, flags) if not ins[0]["props"] & R.ACCEPTOR)
    else:  # (rm_epsilon on the cyclic family: an epsilon cycle sends an item through the single call, a few of the 64)
        assert int(np.sum(flags)) >= BATCH // 2
    _check_items(op, fam, cases, outs)


@pytest.mark.parametrize("fam", R._ANY)
def test_compose_batch(gpu_ctx, fam):
    A = _lib()
    for flt in R.COMPOSE_FILTERS:
        cases = _batch_inputs("compose_" + flt, fam)
        d1 = [to_device(ins[0], gpu_ctx) for ins, _ in cases]
        d2 = [to_device(ins[1], gpu_ctx) for ins, _ in cases]
        outs, flags = A.compose_batch(d1, d2, A.ComposeConfig(A.ComposeFilter[flt]), return_in_kernel=True)
        st = A.compose_batch_stats(gpu_ctx)
        print(f"compose_batch {fam} {flt}: {st}")
        assert st["items_in_kernel"] == int(np.sum(flags)) == BATCH and st["launches"] >= 1, st
        _check_items("compose_" + flt, fam, cases, outs)


@pytest.mark.parametrize("fam", R._ANY)
def test_union_list_and_concat_list_of_64(gpu_ctx, fam):
    """union_list of 64 family members; concat_list of 64 items, three of them as the family draws them and the others
    with a final start state, so that short strings survive 63 concatenations"""
    A = _lib()
    for call in range(4):
        items = [R.small(fam, 0), R.small(fam, 1)] + [R.small(fam, 300 + 62 * call + k) for k in range(BATCH - 2)]
        got = R.relation(A.union_list([to_device(f, gpu_ctx) for f in items]).to_flat())
        R.assert_not_vacuous([R.relation(f) for f in items], f"union_list {fam} call {call}")
        want = R.union_rel(*[R.relation(f) for f in items])
        assert got == want and len(want) >= 3, f"union_list {fam} call {call}: " + R.diff(got, want)
        rng = np.random.default_rng(call)
        plain = set(rng.choice(BATCH, 3, replace=False).tolist())
        items = [f if k in plain else
                 dict(f, finals=np.where(np.arange(f["n_states"]) == f["start"], np.float32(0.25), f["finals"]))
                 for k, f in enumerate(items)]
        items = [R.with_word(dict(f), fam != "cyclic") for f in items]
        got = R.relation(A.concat_list([to_device(f, gpu_ctx) for f in items]).to_flat())
        want = functools.reduce(R.concat_rel, [R.relation(f) for f in items])
        assert got == want, f"concat_list {fam} call {call}: " + R.diff(got, want)
        print(f"concat_list {fam} call {call}: {len(want)} pairs")


# ================================================================ the mid-size family, on sampled strings
def _mid():
    L, L2, Lt, T = R.lattice(0), R.lattice(1), R.lattice(0, acceptor=False), R.mid_transducer()
    return L, L2, Lt, T


def _pairs(seed, machines):
    return R.sample_pairs(np.random.default_rng(seed), machines)


def _same_on(pairs, got, want_fn, what, key=lambda p: p, unkey=lambda p: p):
    """weight_of on both sides for `pairs` (read off the specification's machines) and for 24 more read off successful
    walks of the result itself, which a result that accepts too much would show; (x', y') = key((x, y)) is the result's
    pair for the specification's (x, y), unkey its inverse"""
    got = R.as_machine(got)
    rng = np.random.default_rng(len(pairs))
    pairs = list(pairs) + [unkey(p) for p in R.sample_pairs(rng, [got], n_walks=24, n_random=0)]
    finite = 0
    for p in pairs:
        w, g = want_fn(*p), R.weight_of(got, *key(p))
        assert g == w, f"{what}: {p} has weight {w}, the result gives {g}"
        finite += w != INF
    assert finite >= 48, f"{what}: only {finite} sampled pairs are accepted"
    assert finite < len(pairs), f"{what}: no sampled pair is rejected"


@pytest.mark.parametrize("op", ["rm_epsilon", "tr_sum", "tr_unique", "tr_sort", "optimize", "determinize", "top_sort",
                                "connect"])
def test_lattice_relation_is_kept(gpu_ctx, op):
    L = R.lattice(0)
    ML = R.Machine(L)
    out = getattr(to_device(L, gpu_ctx), op)().to_flat()
    _same_on(_pairs(1, [ML]), out, lambda x, y: R.weight_of(ML, x, y), op)
    R.postconditions(op, [L], out)
    # (tr_sum, tr_unique and tr_sort keep no route counter: that the 300-arc state is above their rank limit of 256 is the
    # family's own assertion in relation_ref.lattice, nothing the device reports)
    if op == "top_sort":
        st = gpu_ctx.top_sort_stats()
        print("top_sort of the lattice:", st)
        assert st["max_level_width"] > 256 and st["wide_launches"] >= 1, st
    if op == "determinize":
        st = gpu_ctx.determinize_stats()
        print("determinize of the lattice:", st)
        assert st["wide_levels"] >= 1, st
        mini = to_device(out, gpu_ctx).minimize().to_flat()
        print("minimize of its result:", gpu_ctx.minimize_stats(), out["n_states"], "->", mini["n_states"])
        _same_on(_pairs(2, [ML]), mini, lambda x, y: R.weight_of(ML, x, y), "minimize(determinize)")
        R.postconditions("minimize", [out], mini)


def test_lattice_reverse_union_concat(gpu_ctx):
    L, L2, _, _ = _mid()
    ML, ML2 = R.Machine(L), R.Machine(L2)
    d, d2 = to_device(L, gpu_ctx), to_device(L2, gpu_ctx)
    _same_on(_pairs(3, [ML]), d.reverse().to_flat(), lambda x, y: R.weight_of(ML, x, y), "reverse",
             key=lambda p: (p[0][::-1], p[1][::-1]), unkey=lambda p: (p[0][::-1], p[1][::-1]))
    u = d.union(d2).to_flat()
    assert u["n_states"] > 2 * 256 and len(u["arcs"]) > 2 * 256
    _same_on(_pairs(4, [ML, ML2]), u, lambda x, y: min(R.weight_of(ML, x, y), R.weight_of(ML2, x, y)), "union")
    # concat: a walk of the first then a walk of the second; both are acceptors, so a split of (x, x) is a split of x
    rng = np.random.default_rng(5)
    heads, tails = R.sample_pairs(rng, [ML]), R.sample_pairs(rng, [ML2])
    pairs = [(h[0] + t[0], h[1] + t[1]) for h, t in zip(heads, tails)]

    def want(x, y):
        if x != y:
            return INF
        return min(R.weight_of(ML, x[:i], x[:i]) + R.weight_of(ML2, x[i:], x[i:]) for i in range(len(x) + 1))
    _same_on(pairs, d.concat(d2).to_flat(), want, "concat")


def test_lattice_project(gpu_ctx):
    A = _lib()
    _, _, Lt, _ = _mid()
    for output in (False, True):
        blind = dict(Lt, arcs=Lt["arcs"].copy())
        blind["arcs"]["ilabel" if output else "olabel"] = 0  # the tape that is minimised over, ignored
        MB = R.Machine(blind)
        pairs = [(p[1], p[1]) if output else (p[0], p[0]) for p in _pairs(6, [R.Machine(Lt)])]
        pairs += [(p[0], p[0][:-1] + (p[0][-1] % R.LATTICE_SIGMA + 1,)) for p in pairs[:8] if p[0]]  # off the diagonal
        kind = A.ProjectType.PROJECT_OUTPUT if output else A.ProjectType.PROJECT_INPUT
        out = to_device(Lt, gpu_ctx).project(kind).to_flat()

        def want(x, y):
            if x != y:
                return INF
            return R.weight_of(MB, EPS, x) if output else R.weight_of(MB, x, EPS)
        _same_on(pairs, out, want, "project output" if output else "project input")


def test_lattice_compose(gpu_ctx):
    L, _, _, T = _mid()
    prod = R.Product(L, T)
    out = to_device(L, gpu_ctx).compose(to_device(T, gpu_ctx)).to_flat()
    st = gpu_ctx.compose_path_stats()
    print("compose of the lattice:", out["n_states"], "states;", st)
    assert st["switched_wide"] == 1 and st["wave_first"] == 0, st  # the wide driver answered, without a knob
    MC = R.Machine(out)
    _same_on(_pairs(7, [prod, MC]), MC, lambda x, y: R.weight_of(prod, x, y), "compose")
