"""The solo query: once three queries in a row have been ended by the bounded head and the cleaned scratch is parked on the
context, a repeated single-shortest-path query is ONE launch of one workgroup that searches, walks the path back and puts
every key it wrote back to +inf (sssp_solo.h).  WFST_SSSP_SOLO=0 switches the route off, =2 tries it whatever the streak and
raises, after the query, with the reason unless the solo kernel answered; WFST_SSSP_SOLO_LOG caps the kernel's log.  Every
result is compared bit for bit with the CPU oracle's canonical path, tied_choices with the oracle's count, and the parked keys
are counted after every query: none may differ from +inf."""
import gc

import numpy as np
import pytest

import rustfst_amd
from rustfst_amd import reach, synth
from helpers import assert_flat_identical, to_device, to_oracle

pytestmark = pytest.mark.gpu

N = 70_000  # the fixture of test_bounded_head.py: the smallest shape with mailbox sweeps, the transpose and the fused tail
KNOB = "WFST_SSSP_SOLO"


@pytest.fixture(scope="module")
def base(oracle):
    t = synth.make_transducer(N, 8, 64, 0.0, seed=9)
    can = to_oracle(oracle, t).shortest_path_canonical()
    dist = np.asarray(can.distance, dtype=np.float32)
    assert dist.shape[0] == N and np.isfinite(dist).all()
    model = reach.head_reach(t)
    assert model["engaged"] and model["levels"] == 8 and model["expanded"] == 67
    return t, dist, can, can.to_flat()


def _canonical(oracle, t):
    can = to_oracle(oracle, t).shortest_path_canonical()
    return can, can.to_flat()


def _counters(ctx):
    return dict(solo=ctx.solo_query(), bounded=ctx.bounded_stats(), rearm=ctx.rearm_stats())


def _query(d, ctx, can, want, what, run=None):
    """One query; the result and tied_choices are the oracle's.  Returns the counters' change."""
    before = _counters(ctx)
    got = (run() if run else d.shortest_path()).to_flat()
    assert_flat_identical(got, want, what)
    assert ctx.stats()["tied_choices"] == can.n_tied_choices, (what, ctx.stats()["tied_choices"], can.n_tied_choices)
    after = _counters(ctx)
    return {fam: {k: after[fam][k] - before[fam][k] for k in after[fam] if isinstance(after[fam][k], int)} for fam in after}


def _solo(d, ctx, can, want, what, run=None):
    """One query that the solo kernel answers: every counter reads as after the bounded stop it replaces."""
    ch = _query(d, ctx, can, want, what, run)
    assert ch["solo"]["attempts"] == 1 and ch["solo"]["answered"] == 1 and ch["solo"]["aborted"] == 0, (what, ch)
    assert ctx.stats()["sweeps"] == 1, (what, ctx.stats()["sweeps"])
    assert ch["bounded"]["stops"] == 1 and ch["bounded"]["full_solves"] == 0, (what, ch)
    assert ch["rearm"]["adopted"] == 1 and ch["rearm"]["armed"] == 1 and ch["rearm"]["dropped"] == 0, (what, ch)
    assert ctx.parked_key_check() == 0, what
    return ch


def _ordinary(d, ctx, can, want, what, run=None):
    ch = _query(d, ctx, can, want, what, run)
    assert ch["solo"]["attempts"] == 0, (what, ch)
    return ch


def _until_solo(d, ctx, can, want, what, run=None, stops=0):
    """Default queries: ordinary ones until three have stopped in a row (`stops` of them already have), then a solo one."""
    for q in range(8):
        ch = _query(d, ctx, can, want, f"{what}: query {q}", run)
        if ch["solo"]["attempts"]:
            assert stops >= 3, (what, q, "solo resumed after fewer than three stops in a row")
            assert ch["solo"]["answered"] == 1 and ctx.parked_key_check() == 0, (what, ch)
            return
        stops = stops + 1 if ch["bounded"]["stops"] else 0
    raise AssertionError(f"{what}: the solo route did not resume")


def _warm(t, want, monkeypatch, what, ctx=None):
    """A handle after the two warm-up queries: the transpose and the list exist, the solve is predicted, its scratch parked."""
    monkeypatch.delenv(KNOB, raising=False)
    ctx = ctx or rustfst_amd.Context(0)
    d = to_device(t, ctx)
    for q in range(2):
        assert_flat_identical(d.shortest_path().to_flat(), want, f"{what}: warm-up {q}")
    return ctx, d


def test_repeats(base, monkeypatch):
    t, _, can, want = base
    ctx, d = _warm(t, want, monkeypatch, "repeats")
    stops = ctx.bounded_stats()["stops"]
    answered = 0
    for q in range(12):
        if stops >= 3:
            _solo(d, ctx, can, want, f"query {q}")
            answered += 1
        else:
            ch = _ordinary(d, ctx, can, want, f"query {q}")
            assert ch["bounded"]["stops"] == 1 and ctx.stats()["sweeps"] == 1, (q, ch)
            assert ctx.parked_key_check() == 0, q
        stops += 1
    assert answered >= 9 and ctx.solo_query()["answered"] == answered


def test_async_route(base, monkeypatch):
    """The bench's order at the smallest size: the query begun, a fused batch of 16 strings begun on a second context, the
    query finished, the batch finished."""
    t, _, can, want = base
    ctx, d = _warm(t, want, monkeypatch, "async")
    ctx_b = rustfst_amd.Context(0)
    strings = rustfst_amd.DeviceFst.upload_many(synth.make_acceptors(t, 16, 20, seed0=1000, mark_finals=False), ctx_b)
    first = None

    def run():
        nonlocal first
        job = d.shortest_path_begin()
        batch = rustfst_amd.compose_shortest_path_batch_begin(strings, d, ctx=ctx_b)
        out = job.finish()
        outs = batch.finish()[0]
        flats = [o.to_flat() for o in outs]
        if first is None:
            first = flats
        for a, b in zip(flats, first):
            assert_flat_identical(a, b, "the batch beside the query")
        return out

    stops = ctx.bounded_stats()["stops"]
    for q in range(8):
        if stops >= 3:
            _solo(d, ctx, can, want, f"async query {q}", run)
        else:
            _ordinary(d, ctx, can, want, f"async query {q}", run)
        stops += 1
    assert ctx.solo_query()["answered"] >= 5


def test_knob_2_and_0(base, monkeypatch):
    t, _, can, want = base
    ctx, d = _warm(t, want, monkeypatch, "knob")
    monkeypatch.setenv(KNOB, "2")
    _solo(d, ctx, can, want, "=2 on a fresh handle: answered at once")
    monkeypatch.setenv(KNOB, "0")
    for q in range(5):
        _ordinary(d, ctx, can, want, f"=0, query {q}")
    monkeypatch.delenv(KNOB)
    _solo(d, ctx, can, want, "the default behind them")


def _aborts_clean_up(t, oracle, monkeypatch, why, reason, what, env=()):
    """Under =2 the query raises with its reason and leaves the parked keys clean; the next default query is right, and so is a
    full solve that must adopt the scratch the solo kernel cleaned."""
    can, want = _canonical(oracle, t)
    for k, v in env:
        monkeypatch.setenv(k, v)
    ctx, d = _warm(t, want, monkeypatch, what)
    assert ctx.parked_key_check() == 0, what
    monkeypatch.setenv(KNOB, "2")
    before = ctx.solo_query()
    with pytest.raises(rustfst_amd.WfstError, match=why):
        d.shortest_path()
    after = ctx.solo_query()
    assert after["attempts"] == before["attempts"] + 1 and after["aborted"] == before["aborted"] + 1, (what, after)
    assert after["last_abort"] == reason and after["answered"] == before["answered"], (what, after)
    assert ctx.parked_key_check() == 0, what
    monkeypatch.delenv(KNOB)
    _ordinary(d, ctx, can, want, f"{what}: the next default query")
    monkeypatch.setenv("WFST_SSSP_BOUNDED", "0")
    monkeypatch.setenv("WFST_SSSP_REARM", "2")
    adopted = ctx.rearm_stats()["adopted"]
    _ordinary(d, ctx, can, want, f"{what}: a full solve on the scratch the solo kernel cleaned")
    assert ctx.rearm_stats()["adopted"] == adopted + 1 and ctx.stats()["sweeps"] > 1, what
    monkeypatch.delenv("WFST_SSSP_BOUNDED")
    monkeypatch.delenv("WFST_SSSP_REARM")
    return can


def test_abort_best_total_beyond_the_band(base, oracle, monkeypatch):
    t = dict(base[0], start=N // 3)
    model = reach.head_reach(t)
    assert not model["engaged"] and model["B"] > model["tau0"]
    _aborts_clean_up(t, oracle, monkeypatch, "gave the query up", "BAND", "start N // 3")


def test_abort_no_final_state_within_reach(base, oracle, monkeypatch):
    t, dist = base[0], base[1]
    fin = np.full(N, np.inf, dtype=np.float32)
    fin[int(np.argmax(dist))] = 0.5
    _aborts_clean_up(dict(t, finals=fin), oracle, monkeypatch, "gave the query up", "BAND", "farthest state")


def test_abort_log_full(base, oracle, monkeypatch):
    """67 listings overflow a log of 32 entries: every key is cleaned, not only the logged ones."""
    t = base[0]
    _aborts_clean_up(t, oracle, monkeypatch, "log of written keys is full", "LOG", "log of 32", env=(("WFST_SSSP_SOLO_LOG", "32"),))


def test_abort_outgrown(base, oracle, monkeypatch):
    """The input of test_bounded_head.py::test_outgrown: a first band of twice the default and one final state at distance 11 —
    some level of the states at or below B is wider than NW_GROW."""
    t, dist = base[0], base[1]
    order = np.argsort(dist, kind="stable")
    f = int(order[np.searchsorted(dist[order], 11.0)])
    fin = np.full(N, np.inf, dtype=np.float32)
    fin[f] = 0.0
    assert dist[f] <= reach.first_band(t, 2.0)
    model = reach.head_reach(dict(t, finals=fin), tau0_mult=2.0)
    assert not model["engaged"] and "NW_GROW" in model["why"]
    _aborts_clean_up(dict(t, finals=fin), oracle, monkeypatch, "outgrew its workgroup", "GREW", "outgrown",
                     env=(("WFST_SSSP_TAU0_MULT", "2"),))


def test_tie_found_only_at_b(base, oracle, monkeypatch):
    """The construction of test_bounded_head.py: a tie found only AT B by expanding a state AT B, plus a second final state at
    the same total: answered solo, the ties counted as the oracle counts them."""
    t, dist = base[0], base[1]
    f1 = int(np.argmin(dist + t["finals"]))
    b = dist[f1]
    assert 0 < b < reach.first_band(t)
    arcs = t["arcs"].copy()
    row = np.arange(t["offsets"][f1], t["offsets"][f1 + 1])
    k = int(row[np.argmax(dist[arcs["nextstate"][row]])])
    g = int(arcs["nextstate"][k])
    assert dist[g] > b and g != f1
    arcs["weight"][k] = 0.0
    other = [s for s in np.flatnonzero((dist > 0) & (dist < b)) if s not in (f1, g)]
    h = int(other[len(other) // 2])
    fin = np.full(N, np.inf, dtype=np.float32)
    fin[f1] = 0.0
    fin[g] = 0.0
    fin[h] = np.float32(b - dist[h])
    assert np.float32(dist[h] + fin[h]) == b
    t2 = dict(t, arcs=arcs, finals=fin)
    assert reach.head_reach(t2)["engaged"]
    can, want = _canonical(oracle, t2)
    assert can.n_tied_choices >= 1
    ctx, d = _warm(t2, want, monkeypatch, "tie at B")
    monkeypatch.setenv(KNOB, "2")
    for q in range(3):
        _solo(d, ctx, can, want, f"tie at B, query {q}")


def test_start_state_final_with_weight_0(base, oracle, monkeypatch):
    """B = 0 from the start: level 0 follows nothing but zero-weight arcs and the search stops there."""
    t = base[0]
    fin = t["finals"].copy()
    fin[0] = 0.0
    t2 = dict(t, finals=fin)
    can, want = _canonical(oracle, t2)
    assert want["n_states"] == 1
    ctx, d = _warm(t2, want, monkeypatch, "start final")
    monkeypatch.setenv(KNOB, "2")
    ch = _solo(d, ctx, can, want, "start final")
    assert ctx.solo_query()["cleaned"] >= 1 and ch["solo"]["answered"] == 1


def test_start_state_without_arcs(base, oracle, monkeypatch):
    """A start state without arcs that is not final: the solo kernel gives up (no total at all) and the empty result comes by
    the ordinary route."""
    t = base[0]
    s = N - 1  # (the last state's row moves nothing else)
    off = t["offsets"].copy()
    arcs = t["arcs"][: off[s]].copy()
    off[s + 1] = off[s]
    fin = t["finals"].copy()
    fin[s] = np.inf
    t2 = dict(t, offsets=off, arcs=arcs, finals=fin)
    can, want = _canonical(oracle, t2)
    ctx, d = _warm(t2, want, monkeypatch, "arcless state")  # (from state 0: the scratch is parked for this plan)
    d.set_start(s)
    can_s, want_s = _canonical(oracle, dict(t2, start=s))
    assert want_s["n_states"] == 0
    monkeypatch.setenv(KNOB, "2")
    before = ctx.solo_query()
    with pytest.raises(rustfst_amd.WfstError, match="gave the query up"):
        d.shortest_path()
    after = ctx.solo_query()
    assert after["aborted"] == before["aborted"] + 1 and after["last_abort"] == "BAND" and ctx.parked_key_check() == 0
    monkeypatch.delenv(KNOB)
    _ordinary(d, ctx, can_s, want_s, "the empty result by the ordinary route")


def test_invalidation(base, oracle, monkeypatch):
    """Between solo queries: another start and back, a knob change, profiling, a query from a second context, a second handle
    of another size on the same context, the handle freed while its scratch is parked.  After each: right results, no raise,
    and the solo route resumes only after three stops in a row."""
    t, _, can, want = base
    ctx, d = _warm(t, want, monkeypatch, "invalidation")
    _until_solo(d, ctx, can, want, "at first", stops=ctx.bounded_stats()["stops"])
    _solo(d, ctx, can, want, "steady")

    can3, want3 = _canonical(oracle, dict(t, start=N // 3))
    d.set_start(N // 3)
    _ordinary(d, ctx, can3, want3, "another start")
    d.set_start(0)
    _until_solo(d, ctx, can, want, "the start moved and back")

    monkeypatch.setenv("WFST_SSSP_BOUNDED", "0")
    _ordinary(d, ctx, can, want, "WFST_SSSP_BOUNDED=0")
    monkeypatch.delenv("WFST_SSSP_BOUNDED")
    _until_solo(d, ctx, can, want, "a knob changed and back")

    ctx.set_profiling(2)
    try:
        _ordinary(d, ctx, can, want, "set_profiling(2)")
    finally:
        ctx.set_profiling(False)
    _until_solo(d, ctx, can, want, "profiling and back")

    ctx2 = rustfst_amd.Context(0)
    got = d.shortest_path_begin(ctx=ctx2).finish().to_flat()
    assert_flat_identical(got, want, "the same handle from a second context")
    assert ctx2.solo_query()["attempts"] == 0
    _until_solo(d, ctx, can, want, "a query from a second context")

    t_small = synth.make_transducer(66_000, 8, 64, 0.0, seed=7)
    can_s, want_s = _canonical(oracle, t_small)
    _, d_small = _warm(t_small, want_s, monkeypatch, "a second handle of another size", ctx=ctx)
    assert ctx.solo_query()["attempts"] == ctx.solo_query()["answered"]
    _ordinary(d_small, ctx, can_s, want_s, "a second handle of another size, third query")
    _until_solo(d, ctx, can, want, "a second handle on the same context")

    assert reach.head_reach(t_small)["engaged"]
    del d  # (its scratch is parked on ctx: the record keeps the plan, never the handle)
    gc.collect()
    _until_solo(d_small, ctx, can_s, want_s, "another handle behind the freed one")


def test_dropped_candidates(base, oracle, monkeypatch):
    """A candidate the old head could only have made wait: the first arc of state 27419 (a level-1 successor of the start,
    expanded at d = 3.732) goes to state 20487 in block 5 with weight tau0 + 1, and no arc of block 0 enters block 5 any
    longer, so the region (0 -> 5) has no room for a message.  The solo kernel drops it: the key stays clean."""
    t = base[0]
    tau0 = np.float32(reach.first_band(t))
    arcs = t["arcs"].copy()
    lo, hi = int(t["offsets"][0]), int(t["offsets"][4096])
    nxt = arcs["nextstate"][lo:hi]
    into5 = (nxt >> 12) == 5
    nxt[into5] += 4096
    arcs["nextstate"][lo:hi] = nxt
    k = int(t["offsets"][27419])
    arcs["nextstate"][k] = 20487
    arcs["weight"][k] = np.float32(tau0 + np.float32(1.0))
    t2 = dict(t, arcs=arcs)
    model = reach.head_reach(t2)
    assert model["engaged"] and model["B"] == 6.138671875 and model["levels"] == 10 and model["expanded"] == 76
    assert np.isclose(model["dist"][27419], 3.732, atol=1e-3) and np.isinf(model["dist"][20487])
    # (the candidate: 3.732 + (9.362 + 1) = 14.09, beyond the band whatever B is)
    assert np.isclose(np.float32(model["dist"][27419]) + arcs["weight"][k], 14.09, atol=1e-2) and 14.09 > tau0 > model["B"]
    can, want = _canonical(oracle, t2)
    ctx, d = _warm(t2, want, monkeypatch, "dropped candidate")
    monkeypatch.setenv(KNOB, "2")
    for q in range(2):
        _solo(d, ctx, can, want, f"dropped candidate, query {q}")
