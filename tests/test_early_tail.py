"""The early tail of a repeated shortest-path query: the search over the final states and the walk back run in an extra
workgroup of the NARROW launch that drains the relaxation, and sssp_tail_kernel keeps that result only when the launch
certifies it (its flag is CLEAN and every key it lowered went above the best total).  WFST_SSSP_EARLY_TAIL=0 switches the
early tail off, =2 raises unless its result was the one returned.  Every result is compared bit for bit with the CPU oracle."""
import numpy as np
import pytest

import rustfst_amd
from rustfst_amd import synth
from helpers import assert_flat_identical, to_device, to_oracle

pytestmark = pytest.mark.gpu

N = 70_000  # the smallest shape with mailbox sweeps (>= 65 536 states), the transpose (>= 2^18 arcs) and the fused tail
KNOB = "WFST_SSSP_EARLY_TAIL"


@pytest.fixture(scope="module")
def base(oracle):
    """T, its distances from state 0, the state of greatest finite distance and a state next to the start."""
    t = synth.make_transducer(N, 8, 64, 0.0, seed=9)
    assert t["arcs"].shape[0] >= 1 << 18
    dist = np.asarray(to_oracle(oracle, t).shortest_path_canonical().distance, dtype=np.float32)
    assert dist.shape[0] == N and np.isfinite(dist).all()  # (the ring backbone reaches every state)
    far = int(np.argmax(dist))
    pos = np.where(dist > 0, dist, np.inf)
    near = int(np.argmin(pos))
    assert near != far and dist[near] < dist[far]
    return t, dist, far, near


def _last_busy_launch_is_narrow(t, ctx):
    """A profiled solve (one launch per level) of a handle of its own: the last launch that relaxed anything is a NARROW one."""
    d = to_device(t, ctx)
    d.shortest_path()
    ctx.reset_stats(); ctx.set_profiling(True); d.shortest_path(); ctx.set_profiling(False)
    _, _, states = ctx.sweep_trace()
    modes = ctx.sweep_modes()
    busy = np.flatnonzero(states > 0)
    assert busy.size and modes[busy[-1]] == 2, (modes, states)


def _warm_up(d, want, monkeypatch, what):
    """Two queries with the default: the transpose and the list exist and the solve is predicted from the third query on."""
    monkeypatch.delenv(KNOB, raising=False)
    for q in range(2):
        assert_flat_identical(d.shortest_path().to_flat(), want, f"{what}: warm-up {q}")


def _query(d, ctx, monkeypatch, mode):
    if mode is None:
        monkeypatch.delenv(KNOB, raising=False)
    else:
        monkeypatch.setenv(KNOB, mode)
    got = d.shortest_path().to_flat()
    return got, ctx.stats()["tied_choices"]


def _default_matches_and_2_raises(t, oracle, monkeypatch, why, what):
    ctx = rustfst_amd.Context(0)
    d = to_device(t, ctx)
    can = to_oracle(oracle, t).shortest_path_canonical()
    want = can.to_flat()
    assert want["n_states"] > 1
    _warm_up(d, want, monkeypatch, what)
    for mode in (None, "1", "0"):
        got, ties = _query(d, ctx, monkeypatch, mode)
        assert_flat_identical(got, want, f"{what}: {KNOB}={mode}")
        assert ties == can.n_tied_choices, (mode, ties, can.n_tied_choices)
    monkeypatch.setenv(KNOB, "2")
    with pytest.raises(rustfst_amd.WfstError, match=why):
        d.shortest_path()
    got, ties = _query(d, ctx, monkeypatch, None)  # (the handle is as good as before)
    assert_flat_identical(got, want, f"{what}: after the error")
    assert ties == can.n_tied_choices
    return can


def test_certified(base, oracle, monkeypatch):
    """Sparse random final states with weights >= 0: queries 3-6 return the canonical path with the oracle's count of tied
    choices whether the early tail is off (0), on (1) or required (2, which does not raise), from two start states."""
    t = base[0]
    fin = t["finals"]
    assert 100 < np.isfinite(fin).sum() < N // 8 and (fin[np.isfinite(fin)] >= 0).all()
    ctx = rustfst_amd.Context(0)
    _last_busy_launch_is_narrow(t, ctx)
    d = to_device(t, ctx)
    for start in (0, N // 3):
        if start:
            d.set_start(start)
        can = to_oracle(oracle, dict(t, start=start)).shortest_path_canonical()
        want = can.to_flat()
        assert want["n_states"] > 1
        _warm_up(d, want, monkeypatch, f"from {start}")
        flats = {}
        for mode in ("1", "2", "0", "2"):
            got, ties = _query(d, ctx, monkeypatch, mode)
            assert_flat_identical(got, want, f"{KNOB}={mode} from {start}")
            assert ties == can.n_tied_choices, (mode, start, ties, can.n_tied_choices)
            flats[mode] = got
        assert_flat_identical(flats["0"], flats["1"], f"0 vs 1 from {start}")
        assert_flat_identical(flats["0"], flats["2"], f"0 vs 2 from {start}")


def test_refuted(base, oracle, monkeypatch):
    """The only final state is the state of greatest distance: whatever the last launch writes is at or below the best total."""
    t, dist, far, _ = base
    fin = np.full(N, np.inf, dtype=np.float32)
    fin[far] = 0.5
    _default_matches_and_2_raises(dict(t, finals=fin), oracle, monkeypatch, "refuted", "refuted")


def test_tie_across_the_boundary(base, oracle, monkeypatch):
    """The far state with final weight 0 and a state next to the start whose final weight makes the totals equal: a write AT
    the best total can make a tie, so the certificate is strict and the ordinary tail counts the tie."""
    t, dist, far, near = base
    fin = np.full(N, np.inf, dtype=np.float32)
    fin[far] = 0.0
    fin[near] = np.float32(dist[far] - dist[near])
    assert np.float32(dist[near] + fin[near]) == dist[far]  # (weights on the 1/512 grid: exact)
    can = _default_matches_and_2_raises(dict(t, finals=fin), oracle, monkeypatch, "early tail", "tie")
    assert can.n_tied_choices >= 1


def test_not_eligible_negative_final_weight(base, oracle, monkeypatch):
    t = base[0]
    fin = t["finals"].copy()
    fin[int(np.flatnonzero(np.isfinite(fin))[-1])] = -0.25
    _default_matches_and_2_raises(dict(t, finals=fin), oracle, monkeypatch, "not eligible", "negative final weight")


def test_not_eligible_without_a_list(base, oracle, monkeypatch):
    """More than 65 536 final states: the handle gets no list, the tail scans, the early tail does not run."""
    t = base[0]
    rng = np.random.default_rng(4)
    fin = np.full(N, np.inf, dtype=np.float32)
    fin[1: 65_536 + 64] = (rng.integers(0, 5120, 65_536 + 63) / 512.0).astype(np.float32)  # (not the start state: a path with arcs)
    _default_matches_and_2_raises(dict(t, finals=fin), oracle, monkeypatch, "not eligible", "no list")


def test_blocks_of_8192_states(oracle, monkeypatch):
    """WFST_SSSP_LOG13=1 at 140 000 states: every launch is a resident one; the result is the oracle's with or without an early
    tail in that kernel."""
    monkeypatch.setenv("WFST_SSSP_LOG13", "1")
    monkeypatch.delenv(KNOB, raising=False)
    t = synth.make_transducer(140_000, 8, 64, 0.0, seed=9)
    can = to_oracle(oracle, t).shortest_path_canonical()
    want = can.to_flat()
    ctx = rustfst_amd.Context(0)
    d = to_device(t, ctx)
    for q in range(5):
        assert_flat_identical(d.shortest_path().to_flat(), want, f"query {q}")
    assert ctx.stats()["tied_choices"] == can.n_tied_choices
    monkeypatch.setenv(KNOB, "0")
    assert_flat_identical(d.shortest_path().to_flat(), want, "early tail off")
