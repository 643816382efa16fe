"""The bounded head of a repeated shortest-path query: launch 0 tracks B, the best total it has seen, follows by min(tau0, B)
and ends the search once everything at or below B is settled and nothing pending can come in at or below B; the ordinary tail
over the list of final states then returns what it returns after the full solve.  WFST_SSSP_BOUNDED=0 switches the stop off,
=2 raises (after the solve, with the reason) unless the stop ended the query.  Every result is compared bit for bit with the
CPU oracle's canonical path, and tied_choices with the oracle's count; every case first runs two warm-up queries."""
import numpy as np
import pytest

import rustfst_amd
from rustfst_amd import reach, synth
from helpers import assert_flat_identical, to_device, to_oracle

pytestmark = pytest.mark.gpu

N = 70_000  # the smallest shape with mailbox sweeps (>= 65 536 states), the transpose (>= 2^18 arcs) and the fused tail
KNOB = "WFST_SSSP_BOUNDED"


@pytest.fixture(scope="module")
def base(oracle):
    """T (the fixture shape of test_early_tail.py) and its distances from state 0."""
    t = synth.make_transducer(N, 8, 64, 0.0, seed=9)
    dist = np.asarray(to_oracle(oracle, t).shortest_path_canonical().distance, dtype=np.float32)
    assert dist.shape[0] == N and np.isfinite(dist).all()
    return t, dist


def _canonical(oracle, t):
    can = to_oracle(oracle, t).shortest_path_canonical()
    return can, can.to_flat()


def _query(d, ctx, monkeypatch, mode):
    if mode is None:
        monkeypatch.delenv(KNOB, raising=False)
    else:
        monkeypatch.setenv(KNOB, mode)
    got = d.shortest_path().to_flat()
    return got, ctx.stats()["tied_choices"]


def _warm_up(d, want, monkeypatch, what):
    """Two queries with the default: the transpose and the list exist and the solve is predicted from the second query on."""
    monkeypatch.delenv(KNOB, raising=False)
    for q in range(2):
        assert_flat_identical(d.shortest_path().to_flat(), want, f"{what}: warm-up {q}")


def _stops_in_every_mode(t, oracle, monkeypatch, what):
    """Knobs 0 / 1 / 2 / default: identical results; 1, 2 and the default end in launch 0 (stops counted, one launch), 0 does not."""
    model = reach.head_reach(t)
    assert model["engaged"], (what, model["why"])
    can, want = _canonical(oracle, t)
    ctx = rustfst_amd.Context(0)
    d = to_device(t, ctx)
    _warm_up(d, want, monkeypatch, what)
    for mode in ("1", "2", "0", "2", None):
        before = ctx.bounded_stats()
        got, ties = _query(d, ctx, monkeypatch, mode)
        after = ctx.bounded_stats()
        assert_flat_identical(got, want, f"{what}: {KNOB}={mode}")
        assert ties == can.n_tied_choices, (what, mode, ties, can.n_tied_choices)
        if mode == "0":
            assert after["stops"] == before["stops"] and after["full_solves"] == before["full_solves"] + 1
            assert "switched off" in after["last_reason"] and ctx.stats()["sweeps"] > 1
        else:
            assert after["stops"] == before["stops"] + 1, (what, mode, after)
            assert ctx.stats()["sweeps"] == 1, (what, mode, ctx.stats()["sweeps"])
    return can


def _default_matches_and_2_raises(t, oracle, monkeypatch, why, what, env=()):
    """The default and 0 return the oracle's path; =2 raises with the reason; the handle is good afterwards."""
    can, want = _canonical(oracle, t)
    ctx = rustfst_amd.Context(0)
    d = to_device(t, ctx)
    for k, v in env:
        monkeypatch.setenv(k, v)
    _warm_up(d, want, monkeypatch, what)
    stops = ctx.bounded_stats()["stops"]
    for mode in (None, "1", "0"):
        got, ties = _query(d, ctx, monkeypatch, mode)
        assert_flat_identical(got, want, f"{what}: {KNOB}={mode}")
        assert ties == can.n_tied_choices, (what, mode, ties, can.n_tied_choices)
    monkeypatch.setenv(KNOB, "2")
    with pytest.raises(rustfst_amd.WfstError, match=why):
        d.shortest_path()
    assert ctx.bounded_stats()["stops"] == stops, what
    got, ties = _query(d, ctx, monkeypatch, None)
    assert_flat_identical(got, want, f"{what}: after the error")
    assert ties == can.n_tied_choices
    return can


def test_stops(base, oracle, monkeypatch):
    """From state 0 the best total (6.1387) lies inside the first band (9.362): 8 levels, 67 expansions on the CPU model."""
    t = base[0]
    model = reach.head_reach(t)
    assert model["levels"] == 8 and max(model["sizes"]) == 13 and model["expanded"] == 67
    assert model["B"] < model["tau0"] and model["B"] < model["least_not_followed"]
    _stops_in_every_mode(t, oracle, monkeypatch, "start 0")


def test_best_total_beyond_the_band(base, oracle, monkeypatch):
    """From state N // 3 the best total (12.85) is beyond the first band: the head behaves as before."""
    t = dict(base[0], start=N // 3)
    model = reach.head_reach(t)
    assert not model["engaged"] and model["B"] > model["tau0"]
    _default_matches_and_2_raises(t, oracle, monkeypatch, "no total at or below the first band", "start N // 3")


def test_no_final_state_within_reach(base, oracle, monkeypatch):
    t, dist = base
    fin = np.full(N, np.inf, dtype=np.float32)
    fin[int(np.argmax(dist))] = 0.5
    _default_matches_and_2_raises(dict(t, finals=fin), oracle, monkeypatch, "no total at or below the first band", "farthest state")


def test_tie_found_only_at_b(base, oracle, monkeypatch):
    """The optimum's final state f1 (final weight 0) has a zero-weight arc to a state that is final with weight 0: that state is
    found only AT B, by expanding a state AT B — the threshold is inclusive.  A second final state on another branch attains
    the same total.  The ties are counted as the oracle counts them."""
    t, dist = base
    f1 = int(np.argmin(dist + t["finals"]))
    b = dist[f1]
    assert 0 < b < reach.first_band(t)
    arcs = t["arcs"].copy()
    row = np.arange(t["offsets"][f1], t["offsets"][f1 + 1])
    k = int(row[np.argmax(dist[arcs["nextstate"][row]])])  # (an arc to a state that no shorter path reaches)
    g = int(arcs["nextstate"][k])
    assert dist[g] > b and g != f1
    arcs["weight"][k] = 0.0
    other = [s for s in np.flatnonzero((dist > 0) & (dist < b)) if s not in (f1, g)]
    h = int(other[len(other) // 2])
    fin = np.full(N, np.inf, dtype=np.float32)
    fin[f1] = 0.0
    fin[g] = 0.0
    fin[h] = np.float32(b - dist[h])
    assert np.float32(dist[h] + fin[h]) == b  # (weights on the 1/512 grid: exact)
    t2 = dict(t, arcs=arcs, finals=fin)
    can = _stops_in_every_mode(t2, oracle, monkeypatch, "tie at B")
    assert can.n_tied_choices >= 1
    d2 = np.asarray(can.distance, dtype=np.float32)
    assert d2[g] == b and d2[f1] == b and d2[h] == dist[h]


def test_start_state_final(base, oracle, monkeypatch):
    t = base[0]
    row = t["arcs"]["weight"][t["offsets"][0]:t["offsets"][1]]
    assert row.min() > 0
    fin = t["finals"].copy()
    fin[0] = np.float32(row.min() / 2)  # below every arc of the start state: a one-state path
    can = _stops_in_every_mode(dict(t, finals=fin), oracle, monkeypatch, "start final, light")
    assert can.to_flat()["n_states"] == 1
    fin[0] = 40.0  # beyond the band: the search goes on and finds T's own best final state
    can = _stops_in_every_mode(dict(t, finals=fin), oracle, monkeypatch, "start final, heavy")
    assert can.to_flat()["n_states"] > 1


def test_outgrown(base, oracle, monkeypatch):
    """A first band of twice the default and a single final state at distance 11: B <= tau0, but some hop level of the states at
    or below B is wider than NW_GROW, so the head hands over to the WIDE levels."""
    t, dist = base
    order = np.argsort(dist, kind="stable")
    f = int(order[np.searchsorted(dist[order], 11.0)])
    b = dist[f]
    fin = np.full(N, np.inf, dtype=np.float32)
    fin[f] = 0.0
    assert b <= reach.first_band(t, 2.0)
    # hop levels of the states at or below B over the tight arcs (d[s] + w == d[t]): the head lists at least these
    off, nxt, w = t["offsets"].astype(np.int64), t["arcs"]["nextstate"].astype(np.int64), t["arcs"]["weight"]
    seen = np.zeros(N, dtype=bool)
    seen[0] = True
    cur, widest = np.array([0]), 1
    while cur.size:
        idx = (off[cur][:, None] + np.arange(8)[None, :]).ravel()
        src = np.repeat(cur, 8)
        tg = nxt[idx]
        tight = ((dist[src] + w[idx]).astype(np.float32) == dist[tg]) & (dist[tg] <= b) & ~seen[tg]
        cur = np.unique(tg[tight])
        seen[cur] = True
        widest = max(widest, int(cur.size))
    assert widest > reach.NW_GROW, widest
    model = reach.head_reach(dict(t, finals=fin), tau0_mult=2.0)
    assert not model["engaged"] and "NW_GROW" in model["why"]
    _default_matches_and_2_raises(dict(t, finals=fin), oracle, monkeypatch, "outgrew", "outgrown", env=(("WFST_SSSP_TAU0_MULT", "2"),))


def test_moving_the_start(base, oracle, monkeypatch):
    """One handle, the start alternating between a source that stops bounded and one that does not: every answer is the oracle's,
    through the shortened predicted chain and the extended one."""
    t = base[0]
    monkeypatch.delenv(KNOB, raising=False)
    cans = {s: _canonical(oracle, dict(t, start=s)) for s in (0, N // 3)}
    ctx = rustfst_amd.Context(0)
    d = to_device(t, ctx)
    _warm_up(d, cans[0][1], monkeypatch, "start 0")
    for rnd in range(3):
        for s in (N // 3, 0):
            d.set_start(s)
            stops = ctx.bounded_stats()["stops"]
            for q in range(2):
                got, ties = _query(d, ctx, monkeypatch, None)
                assert_flat_identical(got, cans[s][1], f"round {rnd}, start {s}, query {q}")
                assert ties == cans[s][0].n_tied_choices
            assert ctx.bounded_stats()["stops"] == stops + (2 if s == 0 else 0), (rnd, s)


def test_scratch_after_a_bounded_stop(base, oracle, monkeypatch):
    """The head's far messages and waits stay behind: shortest_distance on the same handle equals the oracle everywhere, a
    full solve after a bounded one is the oracle's, and the re-armed scratch keeps being adopted."""
    t, dist = base
    can, want = _canonical(oracle, t)
    ctx = rustfst_amd.Context(0)
    d = to_device(t, ctx)
    _warm_up(d, want, monkeypatch, "scratch")
    got, _ = _query(d, ctx, monkeypatch, "2")
    assert_flat_identical(got, want, "bounded")
    np.testing.assert_array_equal(np.asarray(d.shortest_distance(), dtype=np.float32).view(np.uint32), dist.view(np.uint32))
    got, _ = _query(d, ctx, monkeypatch, "2")
    assert_flat_identical(got, want, "bounded again")
    adopted = ctx.rearm_stats()["adopted"]
    got, ties = _query(d, ctx, monkeypatch, "0")
    assert_flat_identical(got, want, "full solve behind a bounded one")
    assert ties == can.n_tied_choices
    assert ctx.rearm_stats()["adopted"] == adopted + 1
    for q in range(3):  # (the full solve outran the chain predicted from the bounded one and parked nothing: a set-up launch, then adopted again)
        got, _ = _query(d, ctx, monkeypatch, "2")
        assert_flat_identical(got, want, f"bounded behind a full solve, query {q}")
    assert ctx.rearm_stats()["adopted"] >= adopted + 3
    np.testing.assert_array_equal(np.asarray(d.shortest_distance(), dtype=np.float32).view(np.uint32), dist.view(np.uint32))


def test_not_eligible_negative_final_weight(base, oracle, monkeypatch):
    t = base[0]
    fin = t["finals"].copy()
    fin[int(np.flatnonzero(np.isfinite(fin))[-1])] = -0.25
    _default_matches_and_2_raises(dict(t, finals=fin), oracle, monkeypatch, "not eligible", "negative final weight")


def test_not_eligible_without_a_list(base, oracle, monkeypatch):
    """More than 65 536 final states: the handle gets no list and the tail scans."""
    t = base[0]
    rng = np.random.default_rng(4)
    fin = np.full(N, np.inf, dtype=np.float32)
    fin[1: 65_536 + 64] = (rng.integers(0, 5120, 65_536 + 63) / 512.0).astype(np.float32)
    _default_matches_and_2_raises(dict(t, finals=fin), oracle, monkeypatch, "not eligible", "no list")


def test_not_eligible_blocks_of_8192_states(base, oracle, monkeypatch):
    _default_matches_and_2_raises(base[0], oracle, monkeypatch, "not eligible", "LOG13", env=(("WFST_SSSP_LOG13", "1"),))


def test_not_eligible_early_tail_required(base, oracle, monkeypatch):
    """WFST_SSSP_EARLY_TAIL=2 demands the stage of the solve that the stop skips: the full solve runs (and that knob is content)."""
    t = base[0]
    can, want = _canonical(oracle, t)
    ctx = rustfst_amd.Context(0)
    d = to_device(t, ctx)
    _warm_up(d, want, monkeypatch, "early tail required")
    monkeypatch.setenv("WFST_SSSP_EARLY_TAIL", "2")
    stops = ctx.bounded_stats()["stops"]
    got, ties = _query(d, ctx, monkeypatch, None)
    assert_flat_identical(got, want, "EARLY_TAIL=2")
    assert ties == can.n_tied_choices and ctx.bounded_stats()["stops"] == stops
    monkeypatch.setenv(KNOB, "2")
    with pytest.raises(rustfst_amd.WfstError, match="not eligible"):
        d.shortest_path()
    monkeypatch.delenv("WFST_SSSP_EARLY_TAIL")
    got, _ = _query(d, ctx, monkeypatch, "2")
    assert_flat_identical(got, want, "after the error")


def test_not_eligible_under_profiling(base, oracle, monkeypatch):
    t = base[0]
    can, want = _canonical(oracle, t)
    ctx = rustfst_amd.Context(0)
    d = to_device(t, ctx)
    _warm_up(d, want, monkeypatch, "profiling")
    for level in (True, 2):
        ctx.set_profiling(level)
        try:
            stops = ctx.bounded_stats()["stops"]
            got, ties = _query(d, ctx, monkeypatch, None)
            assert_flat_identical(got, want, f"profiling {level}")
            assert ties == can.n_tied_choices and ctx.bounded_stats()["stops"] == stops
            assert ctx.stats()["sweeps"] > 1
            monkeypatch.setenv(KNOB, "2")
            with pytest.raises(rustfst_amd.WfstError, match="not eligible"):
                d.shortest_path()
        finally:
            ctx.set_profiling(False)
    got, _ = _query(d, ctx, monkeypatch, "2")
    assert_flat_identical(got, want, "after profiling")
