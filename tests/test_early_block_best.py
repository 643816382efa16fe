"""The early tail's arg-min from the resident launch: on its COLLECT exit every workgroup of sssp_mbox_resident_kernel leaves the
best final state of its block (its keys are in LDS there), and the extra workgroup of the NARROW launch behind it merges those
words instead of searching the handle's list of final states.  WFST_SSSP_EARLY_BEST=0 switches that off, =2 raises unless the
returned result came from those words.  Every result is compared bit for bit with the CPU oracle's canonical path, and
`tied_choices` with the oracle's count.

Shape: T(70 000, 8, 64) — the smallest with mailbox sweeps, the transpose and the fused tail: 18 blocks of 4096 states, the last
one holding 368; it takes a resident launch by default (stats()["relax_kernel"] == 2)."""
import numpy as np
import pytest

import rustfst_amd
from rustfst_amd import synth
from helpers import assert_flat_identical, to_device, to_oracle

pytestmark = pytest.mark.gpu

N = 70_000
B = 4096
LAST = (N // B) * B  # 69 632: first state of the last, partial block
KNOB = "WFST_SSSP_EARLY_BEST"


@pytest.fixture(scope="module")
def base(oracle):
    """T and its distances from state 0 (computed once, never modified)."""
    t = synth.make_transducer(N, 8, 64, 0.0, seed=9)
    assert t["arcs"].shape[0] >= 1 << 18 and N - LAST == 368
    dist = np.asarray(to_oracle(oracle, t).shortest_path_canonical().distance, dtype=np.float32)
    assert dist.shape[0] == N and np.isfinite(dist).all()  # (the ring backbone reaches every state)
    dist.setflags(write=False)
    return t, dist


def _finals(pairs):
    fin = np.full(N, np.inf, dtype=np.float32)
    for s, w in pairs:
        fin[s] = np.float32(w)
    return fin


def _query(d, ctx, monkeypatch, mode):
    if mode is None:
        monkeypatch.delenv(KNOB, raising=False)
    else:
        monkeypatch.setenv(KNOB, mode)
    got = d.shortest_path().to_flat()
    return got, ctx.stats()["tied_choices"]


def _warm_up(d, ctx, want, monkeypatch, what, resident=True):
    """Two queries with the default: the transpose and the list exist and the solve is predicted from the third query on."""
    monkeypatch.delenv(KNOB, raising=False)
    for q in range(2):
        assert_flat_identical(d.shortest_path().to_flat(), want, f"{what}: warm-up {q}")
    if resident:
        assert ctx.stats()["relax_kernel"] == 2, ctx.stats()["relax_kernel"]


def _same_under_every_knob(t, oracle, monkeypatch, what):
    """Queries 3-6 with the knob at 1, 2, 0, 2: the oracle's path and tie count each time, and 2 does not raise."""
    ctx = rustfst_amd.Context(0)
    d = to_device(t, ctx)
    can = to_oracle(oracle, t).shortest_path_canonical()
    want = can.to_flat()
    assert want["n_states"] > 1
    _warm_up(d, ctx, want, monkeypatch, what)
    for mode in ("1", "2", "0", "2"):
        got, ties = _query(d, ctx, monkeypatch, mode)
        assert_flat_identical(got, want, f"{what}: {KNOB}={mode}")
        assert ties == can.n_tied_choices, (what, mode, ties, can.n_tied_choices)
    return can


def test_partials_used(base, oracle, monkeypatch):
    """Sparse random final states, two start states on one handle: 1, 2, 0, 2 return the same flat arrays, 2 does not raise, and
    the second start does not see what the first solve's resident launch left."""
    t = base[0]
    fin = t["finals"]
    assert 100 < np.isfinite(fin).sum() < N // 8 and (fin[np.isfinite(fin)] >= 0).all()
    ctx = rustfst_amd.Context(0)
    d = to_device(t, ctx)
    for start in (0, N // 3):
        if start:
            d.set_start(start)
        can = to_oracle(oracle, dict(t, start=start)).shortest_path_canonical()
        want = can.to_flat()
        assert want["n_states"] > 1
        _warm_up(d, ctx, want, monkeypatch, f"from {start}")
        flats = {}
        for q, mode in enumerate(("1", "2", "0", "2")):
            got, ties = _query(d, ctx, monkeypatch, mode)
            assert_flat_identical(got, want, f"{KNOB}={mode} from {start}")
            assert ties == can.n_tied_choices, (mode, start, ties, can.n_tied_choices)
            flats[q] = got
        for q in (1, 2, 3):
            assert_flat_identical(flats[0], flats[q], f"query {3 + q} vs query 3 from {start}")


def test_without_resident_launches(base, oracle, monkeypatch):
    """WFST_SSSP_RESIDENT=0: one launch per level, nobody leaves the blocks' words: the early workgroup searches the list."""
    t = base[0]
    monkeypatch.setenv("WFST_SSSP_RESIDENT", "0")
    ctx = rustfst_amd.Context(0)
    d = to_device(t, ctx)
    can = to_oracle(oracle, t).shortest_path_canonical()
    want = can.to_flat()
    _warm_up(d, ctx, want, monkeypatch, "no resident launch", resident=False)
    assert ctx.stats()["relax_kernel"] == 1
    got, ties = _query(d, ctx, monkeypatch, None)
    assert_flat_identical(got, want, "default")
    assert ties == can.n_tied_choices
    monkeypatch.setenv(KNOB, "2")
    with pytest.raises(rustfst_amd.WfstError, match="no resident hand-over"):
        d.shortest_path()
    got, ties = _query(d, ctx, monkeypatch, None)  # (the handle is as good as before)
    assert_flat_identical(got, want, "after the error")
    assert ties == can.n_tied_choices


def test_final_states_only_in_the_partial_block(base, oracle, monkeypatch):
    """Every final state lies in the last block (368 states): the other seventeen words are `none`.  Nearer than the median state,
    so that the launch that drains the far end of the search certifies the result."""
    t, dist = base
    near = LAST + np.flatnonzero(dist[LAST:] < np.median(dist))
    assert near.size >= 8
    pick = near[:: max(1, near.size // 8)][:8]
    fin = _finals((int(s), (int(s) % 7) * 0.25) for s in pick)
    assert np.isfinite(fin[:LAST]).sum() == 0 and np.isfinite(fin[LAST:]).sum() == pick.size
    _same_under_every_knob(dict(t, finals=fin), oracle, monkeypatch, "finals in the partial block")


def test_one_final_state(base, oracle, monkeypatch):
    """Exactly one final state in the whole machine, in the partial block."""
    t, dist = base
    s = LAST + int(np.argmin(dist[LAST:]))
    assert dist[s] < np.median(dist)
    fin = _finals([(s, 0.25)])
    assert np.isfinite(fin).sum() == 1
    _same_under_every_knob(dict(t, finals=fin), oracle, monkeypatch, "one final state")


def test_tie_across_two_blocks(base, oracle, monkeypatch):
    """Two final states, the last state of one block and the first of the next, with equal totals: the merge of two blocks'
    words keeps the lower state and the tie, as the oracle does."""
    t, dist = base
    bounds = np.arange(B, N, B)
    k = int(bounds[np.argmin(np.maximum(dist[bounds - 1], dist[bounds]))])
    a, b = k - 1, k
    total = np.float32(max(dist[a], dist[b]))
    assert total < np.median(dist)
    fin = _finals([(a, total - dist[a]), (b, total - dist[b])])
    assert fin[a] >= 0 and fin[b] >= 0
    assert np.float32(dist[a] + fin[a]) == np.float32(dist[b] + fin[b]) == total  # (weights on the 1/512 grid: exact)
    assert a // B + 1 == b // B
    can = _same_under_every_knob(dict(t, finals=fin), oracle, monkeypatch, "tie across two blocks")
    assert can.n_tied_choices >= 1


def test_refuted(base, oracle, monkeypatch):
    """The only final state is the state of greatest distance: whatever the last launch writes is at or below the best total."""
    t, dist = base
    far = int(np.argmax(dist))
    t = dict(t, finals=_finals([(far, 0.5)]))
    ctx = rustfst_amd.Context(0)
    d = to_device(t, ctx)
    can = to_oracle(oracle, t).shortest_path_canonical()
    want = can.to_flat()
    assert want["n_states"] > 1
    _warm_up(d, ctx, want, monkeypatch, "refuted")
    for mode in (None, "1", "0"):
        got, ties = _query(d, ctx, monkeypatch, mode)
        assert_flat_identical(got, want, f"refuted: {KNOB}={mode}")
        assert ties == can.n_tied_choices, (mode, ties, can.n_tied_choices)
    monkeypatch.setenv(KNOB, "2")
    with pytest.raises(rustfst_amd.WfstError, match="refuted"):
        d.shortest_path()
    got, ties = _query(d, ctx, monkeypatch, None)
    assert_flat_identical(got, want, "refuted: after the error")
    assert ties == can.n_tied_choices


def test_blocks_of_8192_states(oracle, monkeypatch):
    """WFST_SSSP_LOG13=1 at 140 000 states: the resident kernel runs the NARROW launches itself, there is no extra workgroup and
    nothing is left for one: the oracle's result with the knob at 0 and at 1."""
    monkeypatch.setenv("WFST_SSSP_LOG13", "1")
    t = synth.make_transducer(140_000, 8, 64, 0.0, seed=9)
    can = to_oracle(oracle, t).shortest_path_canonical()
    want = can.to_flat()
    ctx = rustfst_amd.Context(0)
    d = to_device(t, ctx)
    _warm_up(d, ctx, want, monkeypatch, "8192-state blocks")
    for mode in ("0", "1"):
        got, ties = _query(d, ctx, monkeypatch, mode)
        assert_flat_identical(got, want, f"8192-state blocks: {KNOB}={mode}")
        assert ties == can.n_tied_choices


def test_without_an_early_tail(base, oracle, monkeypatch):
    """WFST_SSSP_EARLY_TAIL=0 with WFST_SSSP_EARLY_BEST=1: the resident launch's epilogue does not disturb a solve without an
    early tail."""
    t = base[0]
    ctx = rustfst_amd.Context(0)
    d = to_device(t, ctx)
    can = to_oracle(oracle, t).shortest_path_canonical()
    want = can.to_flat()
    _warm_up(d, ctx, want, monkeypatch, "no early tail")
    monkeypatch.setenv("WFST_SSSP_EARLY_TAIL", "0")
    for q in range(2):
        got, ties = _query(d, ctx, monkeypatch, "1")
        assert_flat_identical(got, want, f"no early tail: query {q}")
        assert ties == can.n_tied_choices
