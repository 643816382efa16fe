"""One long-lived device handle across in-place edits, cached derived data and the ways a handle is born.

A device handle carries a dozen lazily built derivatives of its arcs (host mirror, reversed CSR, transpose, reversed handle,
region plans, the string o T arrays, is_string, the weight statistics, the launch predictions, the parked scratch of its
context).  tr_sort, project and set_start edit a handle in place and each keeps its own list of what to drop; a forgotten
reset returns a well-formed answer for the FST as it was BEFORE the edit.  The tests here drive one resident handle
through (fill a cache, edit, observe) and compare every observation, bit for bit and property word included, with the
oracle's answer on a FRESH FST built from a model of the handle's content:

  * the pairwise table: every ordered triple (observation Oa, edit M, observation Ob) on small inputs (kept host mirror, the
    one-wave kernels), on 6000-state inputs (no host mirror) and on a 40000-state transducer (transpose, plans, parked scratch);
  * seeded random walks of edits and observations;
  * a handle owned by one context, observed from another;
  * producers x consumers: the result handle of every operation observed as returned and after download + fresh upload;
  * without a GPU: the proof that the table CAN fail — every (edit, observation) pair changes the oracle's answer on at
    least one of its inputs — and that the triple generator emits the full product.
"""
import functools
import itertools

import numpy as np
import pytest

import rustfst_amd
from rustfst_amd import (ClosureType, ComposeConfig, DeviceFst, ProjectType, PushWeightsConfig, ReweightType,
                         ShortestPathConfig, synth)
from oracle import model
from oracle.model import push_ref, reverse_len_rule
from helpers import (_oracle_dist, assert_flat_identical, linear_transducer_flat, one_sided_eps_transducer,
                     random_fst_flat, to_device, to_oracle, walk_labels)
import minimize_cases as mc

ACCEPTOR = model.ACCEPTOR
NOT_I_SORTED, NOT_O_SORTED = model.NOT_I_LABEL_SORTED, model.NOT_O_LABEL_SORTED
SIGMA = 5

# ------------------------------------------------------------------ edits
EDITS = ("tr_sort_ilabel", "tr_sort_olabel", "project_input", "project_output", "set_start")


def edit_device(h, edit, state=None):
    if edit == "tr_sort_ilabel":
        h.tr_sort(True)
    elif edit == "tr_sort_olabel":
        h.tr_sort(False)
    elif edit == "project_input":
        h.project(ProjectType.PROJECT_INPUT)
    elif edit == "project_output":
        h.project(ProjectType.PROJECT_OUTPUT)
    else:
        h.set_start(state)


class Model:
    """What the handle must hold: a flat dict.  Edits go through the oracle (tr_sort, project, set_start, then to_flat(),
    property word included); every observation is answered from a fresh OracleFst of the current flat."""

    def __init__(self, oracle, flat, key=None):
        self.oracle = oracle
        self.flat = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in flat.items()}
        self.home = flat["start"]
        self.history = ()
        self.key = key  # names the input in the answer cache (None: answers are not cached)

    def fresh(self):
        return to_oracle(self.oracle, self.flat)

    def edit(self, edit, state=None):
        o = self.fresh()
        if edit == "tr_sort_ilabel":
            o.tr_sort(by_olabel=False)
        elif edit == "tr_sort_olabel":
            o.tr_sort(by_olabel=True)
        elif edit == "project_input":
            o.project(False)
        elif edit == "project_output":
            o.project(True)
        else:
            o.set_start(state)
        self.flat = o.to_flat()
        self.history += ((edit, state),)

    @property
    def nonneg(self):
        w = self.flat["arcs"]["weight"]
        return not (np.any(w < 0) or np.any(self.flat["finals"] < 0))


# ------------------------------------------------------------------ items: what an observation returns
def canon(item):
    if isinstance(item, dict):
        return ("fst", item["n_states"], item["start"], item["offsets"].tobytes(), item["arcs"].tobytes(),
                item["finals"].tobytes(), int(item["props"]))
    if isinstance(item, np.ndarray):
        return ("arr", str(item.dtype), item.tobytes())
    return item


def same_items(a, b):
    return len(a) == len(b) and all(canon(x) == canon(y) for x, y in zip(a, b))


def check_items(got, exp, what):
    assert len(got) == len(exp), f"{what}: {len(got)} items, expected {len(exp)}"
    for k, (g, e) in enumerate(zip(got, exp)):
        if canon(g) == canon(e):
            continue
        if isinstance(g, dict) and isinstance(e, dict):
            assert_flat_identical(g, e, f"{what}, item {k}")
        if isinstance(g, np.ndarray) and isinstance(e, np.ndarray) and g.shape == e.shape:
            bad = np.nonzero(g.view(np.uint32) != e.view(np.uint32))[0]
            raise AssertionError(f"{what}, item {k}: {bad.size} entries differ, first at {bad[:5]}: {g[bad[:5]]} != {e[bad[:5]]}")
        raise AssertionError(f"{what}, item {k}: {g!r} != {e!r}")


def _err_kind(exc):
    msg = str(exc)
    # compose without a usable sortedness bit: the pair of bits unknown (fst.rs:166-176, "Properties are not known"; the device
    # words it "... properties are not known (sort?)") or known and negative on both sides (compose_fst_op.rs:194, "(sort?)")
    for kind in ("not known", "sort?", "expected acceptor"):
        if kind in msg:
            return ("err", kind)
    return ("err", msg)


def dev_try(fn):
    try:
        return fn()
    except rustfst_amd.WfstError as e:
        return _err_kind(e)


def ora_try(oracle, fn):
    try:
        return fn()
    except oracle.OracleError as e:
        return _err_kind(e)


# ------------------------------------------------------------------ observations: (device side, model side)
# Each takes the input record `inp` (fixed partners and strings of the input, made once from its ORIGINAL content, so that
# an answer changes only because the handle's content did).
def dev_O1(h, inp, mp):  # three queries in a row: parent pass; transpose + final list; re-armed scratch; predictions
    return [h.shortest_path().to_flat() for _ in range(3)]


def ora_O1(m, inp):
    return [m.fresh().shortest_path_canonical().to_flat()] * 3


def dev_O2(h, inp, mp):  # rev_host
    out = [dev_try(lambda: h.shortest_path(ShortestPathConfig(nshortest=4)).to_flat())]
    if inp["unique"]:
        out.append(dev_try(lambda: h.shortest_path(ShortestPathConfig(nshortest=4, unique=True)).to_flat()))
    return out


def ora_O2(m, inp):
    out = [ora_try(m.oracle, lambda: m.fresh().shortest_path_n(4).to_flat())]
    if inp["unique"]:
        out.append(ora_try(m.oracle, lambda: m.fresh().shortest_path_n(4, unique=True).to_flat()))
    return out


def dev_O3(h, inp, mp):  # rev_fst, plans
    dist, hops = h.shortest_distance(want_hops=True)
    rdist, ln = h.shortest_distance_with_len(reverse=True)
    return [dist, hops, rdist, ("len", ln)]


def ora_O3(m, inp):
    can = m.fresh().shortest_path_canonical()
    rdist = m.fresh().reverse().shortest_distance()[1:]
    return [can.distance, can.hops, rdist, ("len", reverse_len_rule(m.flat))]


PUSHES = ((ReweightType.REWEIGHT_TO_INITIAL, False), (ReweightType.REWEIGHT_TO_FINAL, True))


def dev_O4(h, inp, mp):  # rev_fst, structural searches
    return [h.push_weights(rt, PushWeightsConfig(remove_total_weight=rm)).to_flat() for rt, rm in PUSHES]


def ora_O4(m, inp):  # the restatement of oracle/model/push.py on the oracle's distances
    out = []
    for rt, rm in PUSHES:
        to_final = rt == ReweightType.REWEIGHT_TO_FINAL
        out.append(model.to_flat(push_ref(m.flat, _oracle_dist(m.oracle, m.flat, to_final), to_final, rm)))
    return out


def dev_O5(h, inp, mp):  # srec, noeps, wn, property word
    out = []
    for name in ("x_sorted", "x_other"):
        x = to_device(inp[name], h.ctx)
        for connect in (True, False):
            out.append(dev_try(lambda: x.compose(h, ComposeConfig(connect=connect)).to_flat()))
    for name in ("y_sorted", "y_other"):
        y = to_device(inp[name], h.ctx)
        for connect in (True, False):
            out.append(dev_try(lambda: h.compose(y, ComposeConfig(connect=connect)).to_flat()))
    return out


def ora_O5(m, inp):
    out = []
    for name in ("x_sorted", "x_other"):
        for connect in (True, False):
            out.append(ora_try(m.oracle, lambda: to_oracle(m.oracle, inp[name]).compose(m.fresh(), connect=connect).to_flat()))
    for name in ("y_sorted", "y_other"):
        for connect in (True, False):
            out.append(ora_try(m.oracle, lambda: m.fresh().compose(to_oracle(m.oracle, inp[name]), connect=connect).to_flat()))
    return out


def _batch_items(accs, t):
    def run():
        outs, n_arcs = rustfst_amd.compose_shortest_path_batch(accs, t, ctx=t.ctx)
        return [outs[k].to_flat() for k in range(len(accs))] + [("composed arcs", int(n_arcs))]
    got = dev_try(run)
    return got if isinstance(got, list) else [got]


def _ora_batch_items(oracle, accs, ot):
    def run():
        out, tot = [], 0
        for a in accs:
            oc = a.compose(ot, connect=False)  # (ids of the untrimmed composition decide ties)
            tot += oc.num_arcs
            out.append(oc.shortest_path_canonical().to_flat())
        return out + [("composed arcs", tot)]
    got = ora_try(oracle, run)
    return got if isinstance(got, list) else [got]


def dev_O6(h, inp, mp):  # anext, ieps_state: the handle as T of >= 16 string acceptors, both kernels
    accs = DeviceFst.upload_many(inp["strings"], h.ctx)
    mp.delenv("WFST_STRING_KERNEL", raising=False)
    default = _batch_items(accs, h)
    mp.setenv("WFST_STRING_KERNEL", "0")
    general = _batch_items(accs, h)
    mp.delenv("WFST_STRING_KERNEL")
    check_items(default, general, "string kernel at its default vs pinned to 0")
    return default


def ora_O6(m, inp):
    return _ora_batch_items(m.oracle, [to_oracle(m.oracle, a) for a in inp["strings"]], m.fresh())


def dev_O7(h, inp, mp):  # host mirror, rev_host
    return [h.reverse().to_flat(), h.connect().to_flat(), h.rm_epsilon().to_flat(), h.to_flat()]


def ora_O7(m, inp):
    c, r = m.fresh(), m.fresh()
    c.connect()
    r.rm_epsilon()
    return [m.fresh().reverse().to_flat(), c.to_flat(), r.to_flat(), m.flat]


def dev_O8(h, inp, mp):  # is_string: the handle as one of the first operands of a fused batch
    t = to_device(inp["t8"], h.ctx)
    return _batch_items([h] + DeviceFst.upload_many(inp["strings8"], h.ctx), t)


def ora_O8(m, inp):
    return _ora_batch_items(m.oracle, [m.fresh()] + [to_oracle(m.oracle, a) for a in inp["strings8"]],
                            to_oracle(m.oracle, inp["t8"]))


OBS = {"O1": (dev_O1, ora_O1), "O2": (dev_O2, ora_O2), "O3": (dev_O3, ora_O3), "O4": (dev_O4, ora_O4),
       "O5": (dev_O5, ora_O5), "O6": (dev_O6, ora_O6), "O7": (dev_O7, ora_O7), "O8": (dev_O8, ora_O8)}
ALL_OBS = tuple(OBS)

_answers = {}


def answer(m, inp, ob):
    """the model's answer to observation `ob`; cached per (input, edit history): the table asks for each many times"""
    if m.key is None:
        return OBS[ob][1](m, inp)
    key = (m.key, m.history, ob)
    if key not in _answers:
        _answers[key] = OBS[ob][1](m, inp)
    return _answers[key]


def observe(h, m, inp, ob, mp, what):
    check_items(OBS[ob][0](h, inp, mp), answer(m, inp, ob), f"{what}: {ob}")


# ------------------------------------------------------------------ inputs
def _partners(seed):
    """Small compose partners over the same alphabet: sorted on the side the composition matches on (always composable),
    and sorted on the OTHER side only, known not sorted on the matching side (composable only if the handle's own
    property word says it is sorted: else the reference's "(sort?)" error)."""
    rng = np.random.default_rng(50_000 + seed)
    out = {}
    for name, sort, need in (("x_sorted", "olabel", 0), ("x_other", "ilabel", NOT_O_SORTED), ("y_sorted", "ilabel", 0),
                             ("y_other", "olabel", NOT_I_SORTED)):
        while True:
            f = random_fst_flat(rng, 6, 3, SIGMA, p_eps_i=0.15, p_eps_o=0.15, p_final=0.4, sort=sort, min_fanout=1)
            if f["props"] & need == need:
                break
        out[name] = f
    return out


def _alt_start(oracle, flat):
    """a reachable, coaccessible state other than the start state with at least two arcs: the nearest one (smallest id on ties)"""
    o = to_oracle(oracle, flat)
    fwd = o.shortest_path_canonical().distance
    rev = o.reverse().shortest_distance()[1:]
    deg = np.diff(flat["offsets"].astype(np.int64))
    ok = np.isfinite(fwd) & np.isfinite(rev) & (deg >= min(2, deg.max()))
    ok[flat["start"]] = False
    cand = np.nonzero(ok)[0]
    assert cand.size, "input without a second source state: change its seed"
    return int(cand[np.lexsort((cand, fwd[cand]))[0]])


def _finish_input(oracle, key, flat, obs, seed, unique=False, alt=None):
    rng = np.random.default_rng(60_000 + seed)
    alt = _alt_start(oracle, flat) if alt is None else alt
    inp = dict(key=key, flat=flat, obs=tuple(obs), unique=unique, alt=alt, **_partners(seed))
    # 16 strings for the handle as T: walks over its input and its output labels, from both start states it will have
    labs = [walk_labels(rng, flat, s, side, int(rng.integers(1, 9))) for s, side, n in
            ((flat["start"], "ilabel", 6), (flat["start"], "olabel", 4), (alt, "ilabel", 3), (alt, "olabel", 3)) for _ in range(n)]
    inp["strings"] = [synth.linear_acceptor_flat(l, final_weight=0.5 * (k % 2)) for k, l in enumerate(labs)]
    # the handle as a first operand: a fixed epsilon-free, ilabel-sorted T and 15 strings it accepts
    t8 = random_fst_flat(rng, 30, 4, SIGMA, p_final=0.4, sort="ilabel", min_fanout=1)
    inp["t8"] = t8
    inp["strings8"] = [synth.linear_acceptor_flat(walk_labels(rng, t8, 0, "ilabel", int(rng.integers(1, 12)))) for _ in range(15)]
    return inp


S_SEEDS = (12, 16, 21)  # (seeds whose canonical shortest path has >= 4 arcs and a unique optimum)
M_SEEDS = (24, 25)
L_SEED = 300


def _s_flat(seed, acceptor=False):
    rng = np.random.default_rng(40_000 + seed)
    f = random_fst_flat(rng, int(rng.integers(20, 61)), 4, SIGMA, p_eps_i=0.15, p_eps_o=0.15, p_final=0.06, sort="none",
                        min_fanout=1, acyclic=acceptor)
    if acceptor:  # (acyclic: the unique leg determinizes reverse(fst), which need not end on a cyclic weighted acceptor)
        f["arcs"]["olabel"] = f["arcs"]["ilabel"]
        f["props"] = (f["props"] & (NOT_I_SORTED | NOT_O_SORTED)) | ACCEPTOR
    return f


@functools.lru_cache(maxsize=None)
def _small_inputs_cached(oracle):
    inps = [_finish_input(oracle, f"S{seed}", _s_flat(seed), ALL_OBS, seed) for seed in S_SEEDS]
    inps.append(_finish_input(oracle, "S-acc", _s_flat(17, acceptor=True), ALL_OBS, 14, unique=True))
    lin = ("O1", "O6", "O7", "O8")
    inps.append(_finish_input(oracle, "S-str", synth.linear_acceptor_flat(np.random.default_rng(15).integers(1, SIGMA + 1, 12)),
                              lin, 15, alt=3))
    inps.append(_finish_input(oracle, "S-lin", linear_transducer_flat(np.random.default_rng(16), 12, SIGMA), lin, 16, alt=3))
    tobs = ("O1", "O5", "O6", "O7")
    inps.append(_finish_input(oracle, "S-T", one_sided_eps_transducer(np.random.default_rng(17), 40, 4, SIGMA, "olabel"), tobs, 17))
    inps.append(_finish_input(oracle, "S-Tm", one_sided_eps_transducer(np.random.default_rng(18), 40, 4, SIGMA, "ilabel"), tobs, 18))
    return {i["key"]: i for i in inps}


@functools.lru_cache(maxsize=None)
def _medium_inputs_cached(oracle):
    out = {}
    for seed in M_SEEDS:  # beyond the 4096 limits: no host mirror, n > 1 on the host-heap path
        rng = np.random.default_rng(40_000 + seed)
        f = random_fst_flat(rng, 6000, 4, 8, p_eps_i=0.1, p_eps_o=0.1, p_final=0.003, sort="none", min_fanout=1)
        out[f"M{seed}"] = _finish_input(oracle, f"M{seed}", f, ("O1", "O2", "O3", "O4", "O7"), seed)
    return out


@functools.lru_cache(maxsize=None)
def _large_inputs_cached(oracle):
    t = synth.make_transducer(40000, 8, 64, 0.05, seed=L_SEED)  # >= 2^18 arcs: the size at which the transpose is built
    assert t["offsets"][-1] >= 1 << 18
    o = to_oracle(oracle, t)
    o.tr_sort(by_olabel=True)  # the same content in olabel order: the input on which tr_sort by ilabel moves arcs
    return {"L": _finish_input(oracle, "L", t, ("O1", "O3"), L_SEED), "L-o": _finish_input(oracle, "L-o", o.to_flat(), ("O1", "O3"), L_SEED)}


INPUTS = {"small": _small_inputs_cached, "medium": _medium_inputs_cached, "large": _large_inputs_cached}
# (what the generator below reads: the applicable observations per input, without building anything)
APPLICABLE = {"small": {**{f"S{s}": ALL_OBS for s in S_SEEDS}, "S-acc": ALL_OBS, "S-str": ("O1", "O6", "O7", "O8"),
                        "S-lin": ("O1", "O6", "O7", "O8"), "S-T": ("O1", "O5", "O6", "O7"), "S-Tm": ("O1", "O5", "O6", "O7")},
              "medium": {f"M{s}": ("O1", "O2", "O3", "O4", "O7") for s in M_SEEDS},
              "large": {"L": ("O1", "O3"), "L-o": ("O1", "O3")}}


def triples(size):
    """every ordered (input, edit, Oa, Ob) of a size class"""
    for key, obs in APPLICABLE[size].items():
        for edit, oa, ob in itertools.product(EDITS, obs, obs):
            yield key, edit, oa, ob


def run_triple(oracle, ctx, mp, inp, edit, oa, ob):
    """fresh handle: Oa, the edit on the handle and on the model, Ob, Oa again; set_start goes there AND back again"""
    what = f"input {inp['key']}, fill {oa}, edit {edit}, observe {ob}"
    h = to_device(inp["flat"], ctx)
    m = Model(oracle, inp["flat"], inp["key"])
    observe(h, m, inp, oa, mp, f"{what}: fresh")
    for state in ((inp["alt"], m.home) if edit == "set_start" else (None,)):
        edit_device(h, edit, state)
        m.edit(edit, state)
        tag = f"{what}: after {edit}" + (f"({state})" if state is not None else "")
        observe(h, m, inp, ob, mp, tag)
        observe(h, m, inp, oa, mp, tag + ", again")
    check_items([h.to_flat()], [m.flat], f"{what}: content at the end")


def run_table(oracle, ctx, mp, size, edit, oa):
    inputs = INPUTS[size](oracle)
    n = 0
    for key, e, a, ob in triples(size):
        if e == edit and a == oa:
            run_triple(oracle, ctx, mp, inputs[key], edit, oa, ob)
            n += 1
    assert n, "no triple for this (edit, Oa): the generator lost a row"


# ================================================================ without a GPU
def _tight_states(oracle, flat):
    """states on a shortest path (the canonical one where the optimum is unique): forward + reverse distance = the optimum,
    exact on the weight grid"""
    o = to_oracle(oracle, flat)
    can = o.shortest_path_canonical()
    rev = o.reverse().shortest_distance()[1:]
    with np.errstate(invalid="ignore"):
        return np.nonzero(can.distance + rev == np.float32(can.total_weight))[0], can.n_tied_choices


def _positions_changed(before, after, states):
    """does some arc of one of `states` sit at another position within its state?"""
    off = before["offsets"]
    return any(before["arcs"][off[s]:off[s + 1]].tobytes() != after["arcs"][off[s]:off[s + 1]].tobytes() for s in states)


LABEL_FREE = {("project_input", "O3"), ("project_output", "O3")}


def test_triple_generator_emits_the_full_product():
    for size, per_input in APPLICABLE.items():
        got = list(triples(size))
        assert len(got) == len(set(got))
        want = {(k, e, a, b) for k, obs in per_input.items() for e in EDITS for a in obs for b in obs}
        assert set(got) == want
    small = set(triples("small"))
    for e, a, b in itertools.product(EDITS, ALL_OBS, ALL_OBS):  # the S table: every pair of observations on some input
        assert any((k, e, a, b) in small for k in APPLICABLE["small"]), (e, a, b)
    assert {k for k, *_ in triples("small")} >= {f"S{s}" for s in S_SEEDS} | {"S-acc", "S-str", "S-lin", "S-T", "S-Tm"}
    for s in S_SEEDS:  # three seeds carry the whole 8 x 8 table
        assert sum(1 for k, *_ in small if k == f"S{s}") == len(EDITS) * len(ALL_OBS) ** 2
    assert {ob for _, _, a, b in triples("medium") for ob in (a, b)} == {"O1", "O2", "O3", "O4", "O7"}
    assert {ob for _, _, a, b in triples("large") for ob in (a, b)} == {"O1", "O3"}
    assert ("L", "set_start", "O1", "O1") in set(triples("large"))  # three queries on each side of the round trip
    assert {e for _, e, _, _ in triples("large")} == set(EDITS)


def test_inputs_are_what_the_table_needs(oracle):
    small = _small_inputs_cached(oracle)
    for seed in S_SEEDS:
        f = small[f"S{seed}"]["flat"]
        a = f["arcs"]
        assert 20 <= f["n_states"] <= 60 and np.diff(f["offsets"].astype(np.int64)).max() <= 4
        assert f["props"] & NOT_I_SORTED and f["props"] & NOT_O_SORTED  # not sorted on either side at upload
        assert np.any(a["ilabel"] == 0) and np.any(a["olabel"] == 0)  # both epsilon kinds
        assert np.mean(a["ilabel"] != a["olabel"]) > 0.5
        assert _has_cycle(f)
        can = to_oracle(oracle, f).shortest_path_canonical()
        assert can.num_arcs >= 4 and can.n_tied_choices == 0
    acc = small["S-acc"]["flat"]
    assert np.array_equal(acc["arcs"]["ilabel"], acc["arcs"]["olabel"]) and acc["props"] & ACCEPTOR
    st, stm = small["S-T"]["flat"]["arcs"], small["S-Tm"]["flat"]["arcs"]
    assert not np.any(st["ilabel"] == 0) and np.any(st["olabel"] == 0)
    assert not np.any(stm["olabel"] == 0) and np.any(stm["ilabel"] == 0)
    for key in ("S-str", "S-lin"):
        f = small[key]["flat"]
        assert f["n_states"] == 13 and small[key]["alt"] == 3 and len(small[key]["strings"]) >= 16
    assert np.all(small["S-lin"]["flat"]["arcs"]["ilabel"] != small["S-lin"]["flat"]["arcs"]["olabel"])


def _has_cycle(flat):
    n, off, nxt = flat["n_states"], flat["offsets"], flat["arcs"]["nextstate"]
    color = np.zeros(n, np.uint8)
    for root in range(n):
        if color[root]:
            continue
        stack = [(root, int(off[root]))]
        color[root] = 1
        while stack:
            s, k = stack.pop()
            if k < off[s + 1]:
                stack.append((s, k + 1))
                t = int(nxt[k])
                if color[t] == 1:
                    return True
                if color[t] == 0:
                    color[t] = 1
                    stack.append((t, int(off[t])))
            else:
                color[s] = 2
    return False


def test_every_edit_changes_every_observation_somewhere(oracle, capsys):
    """A stale cache shows only if the edit changes the answer.  For every (edit, observation) pair and at least one of its
    inputs of the S table, with the oracle alone: project and set_start change Ob's answer; tr_sort moves an arc of Ob's
    answer, or of a state on the canonical shortest path, to another position within its state (or changes the answer
    outright).  The one pair this cannot hold for is (project, O3): distances, hops and the reversed length do not read
    labels, so for it the test asserts the opposite — the answer is the same on every input — instead of exempting it
    silently.  Prints, per pair, on how many of its inputs the answer changed."""
    inputs = _small_inputs_cached(oracle)
    counts, moved = {}, {}
    for key, inp in inputs.items():
        base = Model(oracle, inp["flat"], key)
        tight, tied = _tight_states(oracle, inp["flat"])
        for edit in EDITS:
            after = Model(oracle, inp["flat"], key)
            after.edit(edit, inp["alt"] if edit == "set_start" else None)
            pos = tied == 0 and _positions_changed(base.flat, after.flat, tight)
            for ob in inp["obs"]:
                differs = not same_items(answer(base, inp, ob), answer(after, inp, ob))
                counts.setdefault((edit, ob), []).append(differs)
                moved.setdefault((edit, ob), []).append(bool(pos))
                if (edit, ob) in LABEL_FREE:
                    assert not differs, f"{edit} changed {ob} on {key}: distances read labels?"
    with capsys.disabled():
        print("\nsensitivity (inputs on which the oracle's answer changes / inputs the pair runs on):")
        for edit in EDITS:
            print("  %-15s" % edit + "  ".join(f"{ob} {sum(counts[(edit, ob)])}/{len(counts[(edit, ob)])}" + (
                f" (arcs moved on {sum(moved[(edit, ob)])})" if edit.startswith("tr_sort") else "") for ob in ALL_OBS))
    for edit, ob in itertools.product(EDITS, ALL_OBS):
        assert (edit, ob) in counts, f"no input runs ({edit}, {ob})"
        if (edit, ob) in LABEL_FREE:
            continue
        if edit.startswith("tr_sort"):
            assert any(counts[(edit, ob)]) or any(moved[(edit, ob)]), f"({edit}, {ob}) cannot fail on any input"
        else:
            assert any(counts[(edit, ob)]), f"({edit}, {ob}) cannot fail on any input"


def test_medium_and_large_rows_are_sensitive_too(oracle):
    """the same proof for the M and L rows, per (edit, observation) pair on at least one input of the row (tr_sort by ilabel
    is the identity on L as generated: L-o, the same transducer sorted by olabel before the upload, is where it bites)"""
    for size in ("medium", "large"):
        hit = {}
        for key, inp in INPUTS[size](oracle).items():
            base = Model(oracle, inp["flat"], key)
            tight, tied = _tight_states(oracle, inp["flat"])
            assert tied == 0
            for edit in EDITS:
                after = Model(oracle, inp["flat"], key)
                after.edit(edit, inp["alt"] if edit == "set_start" else None)
                moved = edit.startswith("tr_sort") and _positions_changed(base.flat, after.flat, tight)
                for ob in inp["obs"]:
                    if size == "medium" and ob == "O4":  # (its restatement is slow at this size: the S table proves the pair)
                        continue
                    differs = not same_items(answer(base, inp, ob), answer(after, inp, ob))
                    hit[(edit, ob)] = hit.get((edit, ob), False) or differs or moved
        for pair, ok in hit.items():
            assert ok or pair in LABEL_FREE, f"{size} row: {pair} cannot fail on any input"


# ================================================================ on the GPU
@pytest.mark.gpu
@pytest.mark.parametrize("oa", ALL_OBS)
@pytest.mark.parametrize("edit", EDITS)
def test_table_small(gpu_ctx, oracle, monkeypatch, edit, oa):
    run_table(oracle, gpu_ctx, monkeypatch, "small", edit, oa)


@pytest.mark.gpu
@pytest.mark.parametrize("oa", ("O1", "O2", "O3", "O4", "O7"))
@pytest.mark.parametrize("edit", EDITS)
def test_table_medium(gpu_ctx, oracle, monkeypatch, edit, oa):
    run_table(oracle, gpu_ctx, monkeypatch, "medium", edit, oa)


@pytest.mark.gpu
@pytest.mark.parametrize("oa", ("O1", "O3"))
@pytest.mark.parametrize("edit", EDITS)
def test_table_large(gpu_ctx, oracle, monkeypatch, edit, oa):
    run_table(oracle, gpu_ctx, monkeypatch, "large", edit, oa)


@pytest.mark.gpu
def test_set_start_turns_the_string_kernel_off_for_the_handle(gpu_ctx, oracle, monkeypatch):
    """S-str from state 3 is linear from there but not a string acceptor by the kernel's definition (start 0): the fused batch
    must take the general kernel for it, and the answer is the oracle's either way."""
    monkeypatch.delenv("WFST_STRING_KERNEL", raising=False)
    inp = _small_inputs_cached(oracle)["S-str"]
    h, m = to_device(inp["flat"], gpu_ctx), Model(oracle, inp["flat"], "S-str")
    observe(h, m, inp, "O8", monkeypatch, "fresh")
    assert gpu_ctx.stats()["string_problems"] == 1 + len(inp["strings8"])
    edit_device(h, "set_start", 3)
    m.edit("set_start", 3)
    observe(h, m, inp, "O8", monkeypatch, "from state 3")
    assert gpu_ctx.stats()["string_problems"] == len(inp["strings8"])


@pytest.mark.gpu
def test_project_output_flips_the_input_epsilon_fact_between_two_string_batches(gpu_ctx, oracle, monkeypatch):
    """S-T has no input epsilons but output epsilons: the string kernel runs the first batch, project(OUTPUT) copies the
    epsilons to the input side and the second batch must take the general kernel.  S-Tm is the mirror image: input epsilons
    only, which project(OUTPUT) removes, so the string kernel runs the second batch only."""
    monkeypatch.delenv("WFST_STRING_KERNEL", raising=False)
    inputs = _small_inputs_cached(oracle)
    for key, first, second in (("S-T", len(inputs["S-T"]["strings"]), 0), ("S-Tm", 0, len(inputs["S-Tm"]["strings"]))):
        inp = inputs[key]
        h, m = to_device(inp["flat"], gpu_ctx), Model(oracle, inp["flat"], key)
        accs = DeviceFst.upload_many(inp["strings"], gpu_ctx)
        for used, edit in ((first, "project_output"), (second, None)):
            check_items(_batch_items(accs, h), answer(m, inp, "O6"), f"{key}: string batch")
            assert gpu_ctx.stats()["string_problems"] == used, f"{key}: string kernel use"
            if edit:
                edit_device(h, edit)
                m.edit(edit)


# ------------------------------------------------------------------ seeded random walks
def run_walk(oracle, ctx, mp, inp, seed, steps):
    rng = np.random.default_rng(seed)
    h, m = to_device(inp["flat"], ctx), Model(oracle, inp["flat"], inp["key"])
    log = []
    for step in range(steps):
        if rng.random() < 0.45:
            edit = EDITS[int(rng.integers(len(EDITS)))]
            state = None
            if edit == "set_start":
                state = inp["alt"] if m.flat["start"] == m.home else m.home
            log.append(f"{edit}({state})" if state is not None else edit)
            edit_device(h, edit, state)
            m.edit(edit, state)
        else:
            ob = inp["obs"][int(rng.integers(len(inp["obs"])))]
            log.append(ob)
            observe(h, m, inp, ob, mp, f"walk seed {seed} on {inp['key']}, step {step} of {log}")
    check_items([h.to_flat()], [m.flat], f"walk seed {seed} on {inp['key']}, content after {log}")


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(4))
def test_random_walk_small(gpu_ctx, oracle, monkeypatch, seed):
    inputs = _small_inputs_cached(oracle)
    run_walk(oracle, gpu_ctx, monkeypatch, inputs[([f"S{s}" for s in S_SEEDS] + ["S-acc"])[seed]], 7000 + seed, 30)


@pytest.mark.gpu
def test_random_walk_large(gpu_ctx, oracle, monkeypatch):
    run_walk(oracle, gpu_ctx, monkeypatch, _large_inputs_cached(oracle)["L"], 7100, 12)


# ------------------------------------------------------------------ two contexts, one thread
@pytest.mark.gpu
@pytest.mark.parametrize("size,key", [("small", f"S{S_SEEDS[0]}"), ("large", "L")])
def test_caches_built_from_another_context_follow_the_edits(oracle, monkeypatch, size, key):
    """ctx2 observes a handle that ctx1 owns (the caches are built from ctx2, with buffers of the owner's pool), ctx1 edits it,
    both observe again."""
    ctx1, ctx2 = rustfst_amd.Context(0), rustfst_amd.Context(0)
    inp = INPUTS[size](oracle)[key]
    for edit in EDITS:
        h = to_device(inp["flat"], ctx1)
        view = DeviceFst(h._h, ctx2, owner=h)  # the same handle, its calls on ctx2
        m = Model(oracle, inp["flat"], key)
        for ob in ("O1", "O3"):
            observe(view, m, inp, ob, monkeypatch, f"{key}: ctx2, fresh")
        edit_device(h, edit, inp["alt"])
        m.edit(edit, inp["alt"] if edit == "set_start" else None)
        for who, hh in (("ctx2", view), ("ctx1", h), ("ctx2 again", view)):
            for ob in ("O1", "O3"):
                observe(hh, m, inp, ob, monkeypatch, f"{key}: {who} after {edit}")
        del view, h


# ------------------------------------------------------------------ producers x consumers
def _acyclic_acceptor(rng, n=30, sort="none"):
    f = random_fst_flat(rng, n, 3, 4, p_final=0.3, acyclic=True, min_fanout=1, sort=sort)
    f["arcs"]["olabel"] = f["arcs"]["ilabel"]
    f["props"] = ACCEPTOR
    return f


def _negative_potentials(flat):
    """potentials that push some arc weights below zero: every other state is 2.5 dearer to leave"""
    return np.where(np.arange(flat["n_states"]) % 2 == 0, 0.0, 2.5).astype(np.float32)


def _producers(ctx, oracle, mp):
    """(name, result handle) of every way a handle is born; S-sized inputs, acyclic acceptors where the producer needs them"""
    small = _small_inputs_cached(oracle)
    s, s2 = small[f"S{S_SEEDS[0]}"]["flat"], small[f"S{S_SEEDS[1]}"]["flat"]
    rng = np.random.default_rng(90_000)
    acc = [_acyclic_acceptor(rng) for _ in range(4)]
    tries = [mc.trie_flat(rng, 12, 4, 6) for _ in range(3)]
    x, y = small[f"S{S_SEEDS[0]}"]["x_sorted"], small[f"S{S_SEEDS[0]}"]["y_sorted"]
    dev = lambda f: to_device(f, ctx)  # noqa: E731
    mp.setenv("WFST_COMPOSE_PATH", "wave")
    yield "compose (wave kernel)", dev(x).compose(dev(s))
    mp.setenv("WFST_COMPOSE_PATH", "wide")
    yield "compose (wide driver)", dev(s).compose(dev(y))
    mp.delenv("WFST_COMPOSE_PATH")
    yield "rm_epsilon", dev(s).rm_epsilon()
    yield "connect", dev(s2).connect()
    yield "reverse", dev(s).reverse()
    yield "reweight to initial, negative arcs", dev(s).reweight(_negative_potentials(s), ReweightType.REWEIGHT_TO_INITIAL)
    yield "reweight to final, negative arcs", dev(acc[0]).reweight(_negative_potentials(acc[0]), ReweightType.REWEIGHT_TO_FINAL)
    yield "push_weights to initial", dev(s).push_weights(ReweightType.REWEIGHT_TO_INITIAL)
    yield "push_weights to final", dev(s2).push_weights(ReweightType.REWEIGHT_TO_FINAL, PushWeightsConfig(remove_total_weight=True))
    det = dev(acc[1]).determinize()
    yield "determinize", det
    yield "minimize", dev(tries[0]).minimize()
    yield "tr_sum", dev(s).tr_sum()
    yield "union", dev(s).union(dev(s2))
    yield "concat", dev(acc[2]).concat(dev(s2))
    yield "closure", dev(s2).closure(ClosureType.CLOSURE_PLUS)
    for k, r in enumerate(rustfst_amd.determinize_batch([dev(a) for a in acc], ctx=ctx)):
        yield f"determinize_batch[{k}]", r
    for k, r in enumerate(rustfst_amd.minimize_batch([dev(t) for t in tries], ctx=ctx)):
        yield f"minimize_batch[{k}]", r
    neg = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in acc[3].items()}
    neg["arcs"]["weight"][::3] -= np.float32(1.5)
    for k, r in enumerate(DeviceFst.upload_many([s, acc[0], neg, small["S-str"]["flat"]], ctx)):
        yield f"upload_many[{k}]", r
    yield "shortest_path (n = 1)", dev(s).shortest_path()
    outs, _ = rustfst_amd.compose_shortest_path_batch(DeviceFst.upload_many(small["S-T"]["strings"], ctx), dev(small["S-T"]["flat"]), ctx=ctx)
    k = max(range(len(outs)), key=lambda i: outs[i].num_arcs)
    assert outs[k].num_arcs > 0
    yield "path_form item of a fused batch", outs[k]
    no_final = dict(s, finals=np.full(s["n_states"], np.inf, np.float32))
    yield "empty result", dev(no_final).shortest_path()


def _consumer_obs(flat):
    obs = ["O1", "O2", "O3", "O4", "O5", "O6", "O7"]
    if flat["n_states"] == 0 or flat["start"] is None:
        obs = ["O1", "O2", "O5", "O7"]  # (distances and pushes of an FST without states: covered by the degenerate-input tests)
    return obs


def _consumer_input(oracle, name, flat):
    rng = np.random.default_rng(91_000)
    inp = dict(key=None, flat=flat, unique=bool(flat["props"] & ACCEPTOR and flat["props"] & synth.ACYCLIC), **_partners(77))
    if flat["n_states"] and flat["start"] is not None:
        labs = [walk_labels(rng, flat, flat["start"], "ilabel", int(rng.integers(1, 9))) for _ in range(16)]
    else:
        labs = [np.array([1 + k % SIGMA], np.uint32) for k in range(16)]
    inp["strings"] = [synth.linear_acceptor_flat(l) for l in labs]
    return inp


@pytest.mark.gpu
def test_result_handles_answer_like_fresh_uploads_of_their_content(gpu_ctx, oracle, monkeypatch):
    """Every result handle, (a) as returned and (b) downloaded and uploaded afresh, through O1-O7: (a) = (b) item for item,
    and (b) = the oracle on that content (O1 and O3 only where no weight is negative: the canonical rule's domain)."""
    for name, res in _producers(gpu_ctx, oracle, monkeypatch):
        flat = res.to_flat()  # (the next test observes result handles nothing was read from)
        inp = _consumer_input(oracle, name, flat)
        fresh = to_device(flat, gpu_ctx)
        m = Model(oracle, flat)
        for ob in _consumer_obs(flat):
            a = OBS[ob][0](res, inp, monkeypatch)
            b = OBS[ob][0](fresh, inp, monkeypatch)
            check_items(a, b, f"{name}: {ob}, as returned vs uploaded afresh")
            if ob in ("O1", "O3", "O4") and not m.nonneg:
                continue
            check_items(b, answer(m, inp, ob), f"{name}: {ob}, uploaded afresh vs the oracle")


@pytest.mark.gpu
def test_first_use_of_a_result_handle_is_each_observation(gpu_ctx, oracle, monkeypatch):
    """The same, with a NEW result handle per observation and nothing read from it before (no download first): the path a
    host-resident or path_form result takes to the device on its first use."""
    names = ("shortest_path (n = 1)", "path_form item of a fused batch", "empty result", "upload_many[2]", "minimize_batch[0]",
             "determinize_batch[0]", "reweight to initial, negative arcs")
    ref = {name: res.to_flat() for name, res in _producers(gpu_ctx, oracle, monkeypatch) if name in names}
    assert set(ref) == set(names)
    for ob in ("O1", "O2", "O3", "O5", "O6", "O7"):
        for name, res in _producers(gpu_ctx, oracle, monkeypatch):
            if name not in names or ob not in _consumer_obs(ref[name]):
                continue
            inp = _consumer_input(oracle, name, ref[name])
            check_items(OBS[ob][0](res, inp, monkeypatch), OBS[ob][0](to_device(ref[name], gpu_ctx), inp, monkeypatch),
                        f"{name}: {ob} as the first use")


@pytest.mark.gpu
def test_negative_arc_weight_same_answers_however_the_handle_was_born(gpu_ctx, oracle):
    """has_negative keeps the one-wave searches (n-best batch kernel, n = 1 batch kernel) and the early tail off an input
    with a negative arc weight; every producer must work it out.  An acyclic acceptor with negative arcs, born by upload,
    by upload_many, as the output of reweight and as an item of minimize_batch: the same n-best and n = 1 answers, single
    call and batch call, equal to the oracle's n-best (reference mode) and to brute force over its paths."""
    from helpers import check_nbest_against_brute_force
    rng = np.random.default_rng(92_000)
    base = _acyclic_acceptor(rng, 24)
    neg = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
    neg["arcs"]["weight"][::2] -= np.float32(3.0)
    assert np.any(neg["arcs"]["weight"] < 0)
    other = _acyclic_acceptor(rng, 10)
    born = {"upload": to_device(neg, gpu_ctx),
            "upload_many": DeviceFst.upload_many([other, neg, other], gpu_ctx)[1],
            "upload_many, alone": DeviceFst.upload_many([neg], gpu_ctx)[0]}
    cfg4, cfg1 = ShortestPathConfig(nshortest=4), ShortestPathConfig(nshortest=1)
    want4 = to_oracle(oracle, neg).shortest_path_n(4).to_flat()
    check_nbest_against_brute_force(want4, neg, 4, "oracle")
    want1 = born["upload"].shortest_path().to_flat()
    check_nbest_against_brute_force(want1, neg, 1, "n = 1")
    pad = [to_device(other, gpu_ctx), to_device(other, gpu_ctx)]
    for name, h in born.items():
        assert_flat_identical(h.shortest_path(cfg4).to_flat(), want4, f"{name}: n = 4")
        assert_flat_identical(h.shortest_path().to_flat(), want1, f"{name}: n = 1")
        assert_flat_identical(rustfst_amd.shortest_path_batch(pad + [h], cfg4, ctx=gpu_ctx)[2].to_flat(), want4, f"{name}: n = 4 in a batch")
        assert_flat_identical(rustfst_amd.shortest_path_batch(pad + [h], cfg1, ctx=gpu_ctx)[2].to_flat(), want1, f"{name}: n = 1 in a batch")
    # reweight makes the negative arcs on the device: the result as returned and its content uploaded afresh
    pot = _negative_potentials(base)
    r = to_device(base, gpu_ctx).reweight(pot, ReweightType.REWEIGHT_TO_INITIAL)
    rf = r.to_flat()
    assert np.any(rf["arcs"]["weight"] < 0)
    r2 = to_device(base, gpu_ctx).reweight(pot, ReweightType.REWEIGHT_TO_INITIAL)  # (nothing read from it before its first search)
    for cfg, n in ((cfg4, 4), (cfg1, 1)):
        want = to_device(rf, gpu_ctx).shortest_path(cfg).to_flat()
        check_nbest_against_brute_force(want, rf, n, f"reweight output, n = {n}")
        assert_flat_identical(r2.shortest_path(cfg).to_flat(), want, f"reweight output as returned, n = {n}")
        assert_flat_identical(rustfst_amd.shortest_path_batch(pad + [r], cfg, ctx=gpu_ctx)[2].to_flat(), want, f"reweight output in a batch, n = {n}")


@pytest.mark.gpu
def test_negative_weights_beyond_the_one_wave_sizes_born_by_upload_many(gpu_ctx, oracle):
    """the same at 6000 states (the relaxation's regimes read has_negative): an acyclic FST with negative arcs answers alike
    born by upload and by upload_many, and its best weight is the reference-mode oracle's"""
    rng = np.random.default_rng(93_000)
    f = random_fst_flat(rng, 6000, 4, 8, p_final=0.01, acyclic=True, min_fanout=1)
    f["arcs"]["weight"][::5] -= np.float32(2.0)
    a, b = to_device(f, gpu_ctx), DeviceFst.upload_many([synth.linear_acceptor_flat([1, 2]), f], gpu_ctx)[1]
    want = a.shortest_path().to_flat()
    ref = to_oracle(oracle, f).shortest_path()
    assert want["n_states"] > 1 and abs(float(model.F32(0) + sum(want["arcs"]["weight"][::-1].astype(np.float64)) + want["finals"][0]) - ref.total_weight) <= 1e-3
    for q in range(3):
        assert_flat_identical(b.shortest_path().to_flat(), want, f"upload_many, query {q}")
    np.testing.assert_array_equal(b.shortest_distance().view(np.uint32), a.shortest_distance().view(np.uint32))
    cfg = ShortestPathConfig(nshortest=3)
    assert_flat_identical(b.shortest_path(cfg).to_flat(), a.shortest_path(cfg).to_flat(), "n = 3")
    assert_flat_identical(b.shortest_path(cfg).to_flat(), to_oracle(oracle, f).shortest_path_n(3).to_flat(), "n = 3 vs the oracle")
