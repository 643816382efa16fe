"""Re-armed relaxation scratch: a predicted mailbox solve has its scratch cleaned on the device BEHIND its result
(sssp_mbox_rearm_kernel, on the fused tail's verdict) and parks it on the context; the next solve with the same plan and schedule
adopts it, queues no set-up launch, and launch 0 seeds the start state itself.  WFST_SSSP_REARM=0 is the behaviour without any
of it, =2 raises (after the solve) unless the solve started from adopted scratch, and says why.  Context.rearm_stats() counts
armed / adopted / dropped per context.  Every path is compared bit for bit with the CPU oracle's canonical path, and
`tied_choices` with the oracle's count.

Shape: T(70 000, 8, 64), as tests/test_early_block_best.py: the smallest with mailbox sweeps, a resident launch, the transpose and
the fused tail — 18 blocks of 4096 states, the last one holding 368.  Queries 1-3 of a handle run with the default: the 2nd
builds the transpose, the 3rd is the first predicted one and arms."""
import gc

import numpy as np
import pytest

import rustfst_amd
from rustfst_amd import synth
from helpers import assert_flat_identical, to_device, to_oracle

pytestmark = pytest.mark.gpu

N = 70_000
B = 4096
LAST = (N // B) * B  # 69 632: first state of the last, partial block
KNOB = "WFST_SSSP_REARM"
PATH_PINNED = 4096  # arcs of a path that the tail writes straight into pinned memory (sssp.hip)


def _oracle_of(oracle, t):
    can = to_oracle(oracle, t).shortest_path_canonical()
    return can.to_flat(), can.n_tied_choices


@pytest.fixture(scope="module")
def base(oracle):
    """T, a second T of the same size (another seed: another plan), and their oracle results from state 0 (computed once)."""
    t = synth.make_transducer(N, 8, 64, 0.0, seed=9)
    t2 = synth.make_transducer(N, 8, 64, 0.0, seed=10)
    assert N - LAST == 368
    return t, _oracle_of(oracle, t), t2, _oracle_of(oracle, t2)


def _query(d, ctx, monkeypatch, mode, exp, what, ties=True):
    """One query under WFST_SSSP_REARM=mode (None: unset), compared with the oracle's (flat, tied choices).  ties=False: a query
    whose tail does not count them (the first two of a handle: no transpose yet; a path beyond the pinned buffer)."""
    if mode is None:
        monkeypatch.delenv(KNOB, raising=False)
    else:
        monkeypatch.setenv(KNOB, mode)
    got = d.shortest_path().to_flat()
    assert_flat_identical(got, exp[0], f"{what}: {KNOB}={mode}, {ctx.rearm_stats()}")
    if ties:
        assert ctx.stats()["tied_choices"] == exp[1], (what, mode, ctx.stats()["tied_choices"], exp[1], ctx.rearm_stats())


def _prime(d, ctx, monkeypatch, exp, what):
    """Queries 1-3 with the default; the third is predicted and parks its scratch."""
    for q in range(2):
        _query(d, ctx, monkeypatch, None, exp, f"{what}: query {q + 1}", ties=False)
    before = ctx.rearm_stats()["armed"]
    _query(d, ctx, monkeypatch, None, exp, f"{what}: query 3")
    assert ctx.rearm_stats()["armed"] == before + 1, (what, ctx.rearm_stats())


def _raises(d, monkeypatch, match):
    monkeypatch.setenv(KNOB, "2")
    with pytest.raises(rustfst_amd.WfstError, match=match):
        d.shortest_path()
    monkeypatch.delenv(KNOB)


def test_repeated_query(base, monkeypatch):
    """Queries 4-9 with the knob at 1, 2, 0, 2, 1, 2: the first 2 does not raise, the 2 straight after the 0 raises "nothing
    parked" (the 0 gave the scratch back), and `adopted` rises by exactly the number of adopting solves."""
    t, exp = base[0], base[1]
    ctx = rustfst_amd.Context(0)
    d = to_device(t, ctx)
    _prime(d, ctx, monkeypatch, exp, "repeated")
    assert ctx.stats()["relax_kernel"] == 2
    s0 = ctx.rearm_stats()
    _query(d, ctx, monkeypatch, "1", exp, "query 4")
    _query(d, ctx, monkeypatch, "2", exp, "query 5")
    assert ctx.rearm_stats()["adopted"] == s0["adopted"] + 2
    _query(d, ctx, monkeypatch, "0", exp, "query 6")
    s = ctx.rearm_stats()
    assert s["adopted"] == s0["adopted"] + 2 and s["dropped"] == s0["dropped"] + 1 and s["armed"] == s0["armed"] + 2, (s0, s)
    _raises(d, monkeypatch, "nothing parked")  # query 7: solved to its end, and parked again
    _query(d, ctx, monkeypatch, "1", exp, "query 8")
    _query(d, ctx, monkeypatch, "2", exp, "query 9")
    assert ctx.rearm_stats()["adopted"] == s0["adopted"] + 4, (s0, ctx.rearm_stats())


def _without_arcs_of(t, s):
    """A copy of T in which state s has no arcs and is the start state."""
    off = t["offsets"].astype(np.int64)
    keep = np.ones(t["arcs"].shape[0], dtype=bool)
    keep[off[s]:off[s + 1]] = False
    deg = np.diff(off)
    deg[s] = 0
    offsets = np.concatenate(([0], np.cumsum(deg))).astype(np.uint32)
    props = t["props"] & ~(synth.ACCESSIBLE | synth.INITIAL_CYCLIC)  # (no longer known)
    return dict(t, start=int(s), offsets=offsets, arcs=t["arcs"][keep].copy(), props=props)


def test_start_states(base, oracle, monkeypatch):
    """One handle, three start states (block 0, a middle block, the partial last block) with set_start between them, knob 1
    throughout: launch 0 seeds whatever start the query has.  A fresh handle agrees; a start state without arcs returns the
    oracle's result twice in a row."""
    t = base[0]
    monkeypatch.setenv(KNOB, "1")
    ctx = rustfst_amd.Context(0)
    d = to_device(t, ctx)
    starts = (0, N // 3, LAST + 100)
    exps = {}
    for start in starts:
        if start:
            d.set_start(start)
        exps[start] = base[1] if start == 0 else _oracle_of(oracle, dict(t, start=start))
        assert exps[start][0]["n_states"] > 1
        for q in range(4):
            _query(d, ctx, monkeypatch, "1", exps[start], f"from {start}, query {q + 1}", ties=start != 0 or q >= 2)
    assert ctx.rearm_stats()["adopted"] >= 3, ctx.rearm_stats()  # (at least the repeats of every start)
    ctx2 = rustfst_amd.Context(0)
    fresh = to_device(dict(t, start=starts[2]), ctx2)
    _query(fresh, ctx2, monkeypatch, "1", exps[starts[2]], "fresh handle", ties=False)
    # a start state without out-arcs: final (a path of one state) and not final (the empty FST)
    fin = np.flatnonzero(np.isfinite(t["finals"]))
    non = np.flatnonzero(~np.isfinite(t["finals"]))
    for s in (int(fin[fin > B][0]), int(non[non > B][0])):
        ts = _without_arcs_of(t, s)
        exp = _oracle_of(oracle, ts)
        assert exp[0]["n_states"] == (1 if np.isfinite(t["finals"][s]) else 0)
        ds = to_device(ts, ctx)
        for q in range(4):  # (the 3rd is predicted and arms, the 4th seeds an entry without arcs)
            _query(ds, ctx, monkeypatch, "1", exp, f"start {s} without arcs, query {q + 1}", ties=q >= 2)


def test_two_handles_alternating(base, monkeypatch):
    """Two handles of equal size on one context (different seeds: different plans), A, B, A, B, A, B: nobody adopts the other's
    scratch; then A, A adopts."""
    t, exp, t2, exp2 = base
    ctx = rustfst_amd.Context(0)
    a, b = to_device(t, ctx), to_device(t2, ctx)
    _prime(a, ctx, monkeypatch, exp, "A")
    _prime(b, ctx, monkeypatch, exp2, "B")
    adopted = ctx.rearm_stats()["adopted"]
    for r in range(3):
        _query(a, ctx, monkeypatch, None, exp, f"A, round {r}")
        _query(b, ctx, monkeypatch, None, exp2, f"B, round {r}")
        assert ctx.rearm_stats()["adopted"] == adopted, (r, ctx.rearm_stats())
    _query(a, ctx, monkeypatch, None, exp, "A after B")
    _query(a, ctx, monkeypatch, "2", exp, "A after A")
    assert ctx.rearm_stats()["adopted"] == adopted + 1, ctx.rearm_stats()


def test_handle_address_reuse(base, monkeypatch):
    """Arm on A, destroy A, create B of the same size: B never starts from A's scratch, wherever its handle lies."""
    t, exp, t2, exp2 = base
    ctx = rustfst_amd.Context(0)
    a = to_device(t, ctx)
    _prime(a, ctx, monkeypatch, exp, "A")
    del a
    gc.collect()
    b = to_device(t2, ctx)
    adopted = ctx.rearm_stats()["adopted"]
    _raises(b, monkeypatch, "parked for another plan|nothing parked")
    assert ctx.rearm_stats()["adopted"] == adopted
    _query(b, ctx, monkeypatch, None, exp2, "B", ties=False)
    _query(b, ctx, monkeypatch, None, exp2, "B again")


def test_two_contexts_one_handle(base, monkeypatch):
    """One handle queried from two contexts at once (each on half the device, so that both solves are resident ones side by
    side): every context parks and adopts its own scratch."""
    t, exp = base[0], base[1]
    monkeypatch.delenv(KNOB, raising=False)
    ctxs = [rustfst_amd.Context(0), rustfst_amd.Context(0)]
    for c in ctxs:
        c.set_resident_share(1)
    d = to_device(t, ctxs[0])
    for q in range(3):
        for c in ctxs:
            got = d.shortest_path_begin(ctx=c).finish().to_flat()
            assert_flat_identical(got, exp[0], f"priming query {q + 1}")
    for r in range(3):
        before = [c.rearm_stats()["adopted"] for c in ctxs]
        jobs = [d.shortest_path_begin(ctx=c) for c in ctxs]
        for k, (c, job) in enumerate(zip(ctxs, jobs)):
            assert_flat_identical(job.finish().to_flat(), exp[0], f"round {r}, context {k}: {c.rearm_stats()}")
            assert c.stats()["tied_choices"] == exp[1]
        for k, c in enumerate(ctxs):
            assert c.rearm_stats()["adopted"] == before[k] + 1, (r, k, c.rearm_stats())


@pytest.mark.parametrize("knob, value, n", [("WFST_SSSP_RESIDENT", "0", N), ("WFST_SSSP_TAU0_MULT", "0.5", N),
                                             ("WFST_SSSP_NARROW", "0", N), ("WFST_SSSP_LOG13", "1", 140_000),
                                             ("WFST_SSSP_MAILBOX", "0", N)])
def test_knobs_that_change_the_solve(base, oracle, monkeypatch, knob, value, n):
    """A knob that changes the solve's shape between an arming solve and the next: that solve does not adopt (the scratch is
    dropped) and is right; the solve after returning to the default arms again."""
    if n == N:
        t, exp = base[0], base[1]
    else:
        t = synth.make_transducer(n, 8, 64, 0.0, seed=9)
        exp = _oracle_of(oracle, t)
    ctx = rustfst_amd.Context(0)
    d = to_device(t, ctx)
    _prime(d, ctx, monkeypatch, exp, knob)
    _query(d, ctx, monkeypatch, "2", exp, f"{knob}: armed")
    s0 = ctx.rearm_stats()
    monkeypatch.setenv(knob, value)
    _query(d, ctx, monkeypatch, None, exp, f"{knob}={value}")
    s1 = ctx.rearm_stats()
    assert s1["adopted"] == s0["adopted"] and s1["dropped"] == s0["dropped"] + 1, (s0, s1)
    monkeypatch.delenv(knob)
    _query(d, ctx, monkeypatch, None, exp, f"{knob}: back to the default")
    s2 = ctx.rearm_stats()
    assert s2["armed"] == s1["armed"] + 1, (s1, s2)


def test_solve_that_outruns_its_prediction(base, monkeypatch):
    """WFST_SSSP_RES_LEVELS=2 after arming: the resident launch hands over early and the batch is extended.  Nothing is parked
    after such a solve; two queries later adoption is back."""
    t, exp = base[0], base[1]
    ctx = rustfst_amd.Context(0)
    d = to_device(t, ctx)
    _prime(d, ctx, monkeypatch, exp, "outrun")
    monkeypatch.setenv("WFST_SSSP_RES_LEVELS", "2")
    armed = ctx.rearm_stats()["armed"]
    _query(d, ctx, monkeypatch, None, exp, "RES_LEVELS=2")
    assert ctx.rearm_stats()["armed"] == armed, ctx.rearm_stats()
    monkeypatch.delenv("WFST_SSSP_RES_LEVELS")
    _raises(d, monkeypatch, "nothing parked")
    _query(d, ctx, monkeypatch, "2", exp, "two queries later")


def test_keys_needed_after_the_tail(oracle, monkeypatch):
    """A chain i -> i + 1 with two arcs per state (1/512 and 8), the only final state 6000 steps from the start: the best path
    has more arcs than the pinned buffer holds, the tail raises pad & 8 and the host reads the keys again in the parent pass —
    the case the tail's verdict guards.  Whether the solve is predicted within 64 launches depends on the device; the results
    are the oracle's either way."""
    n = N
    src = np.repeat(np.arange(n, dtype=np.uint32), 2)
    arcs = np.empty(2 * n, dtype=synth.TR_DTYPE)
    arcs["ilabel"] = np.tile(np.array([1, 2], dtype=np.uint32), n)
    arcs["olabel"] = np.tile(np.array([2, 1], dtype=np.uint32), n)
    arcs["weight"] = np.tile(np.array([1.0 / 512.0, 8.0], dtype=np.float32), n)
    arcs["nextstate"] = (src + 1) % n
    finals = np.full(n, np.inf, dtype=np.float32)
    finals[6000] = 0.0
    props = synth.make_transducer(16, 2, 4, 0.0, seed=1)["props"]  # (the same facts hold here)
    t = dict(n_states=n, start=0, offsets=(np.arange(n + 1, dtype=np.uint32) * 2), arcs=arcs, finals=finals, props=props)
    exp = _oracle_of(oracle, t)
    assert exp[0]["arcs"].shape[0] == 6000 > PATH_PINNED
    monkeypatch.delenv(KNOB, raising=False)
    ctx = rustfst_amd.Context(0)
    d = to_device(t, ctx)
    for q in range(6):
        _query(d, ctx, monkeypatch, None, exp, f"long path, query {q + 1}", ties=False)


def test_pool_under_pressure(base, monkeypatch):
    """The pool's trim (what an allocation that fails does first) frees parked scratch: the next solve finds it gone."""
    t, exp = base[0], base[1]
    ctx = rustfst_amd.Context(0)
    d = to_device(t, ctx)
    _prime(d, ctx, monkeypatch, exp, "trim")
    ctx.trim_pool()
    _raises(d, monkeypatch, "blocks reclaimed")
    _query(d, ctx, monkeypatch, None, exp, "after the trim")
    _query(d, ctx, monkeypatch, "2", exp, "armed again")


def test_knob_zero_is_the_parent(base, monkeypatch):
    """WFST_SSSP_REARM=0 for a whole context's life: nothing is ever parked or adopted."""
    t, exp = base[0], base[1]
    monkeypatch.setenv(KNOB, "0")
    ctx = rustfst_amd.Context(0)
    d = to_device(t, ctx)
    for q in range(5):
        _query(d, ctx, monkeypatch, "0", exp, f"query {q + 1}", ties=q >= 2)
    s = ctx.rearm_stats()
    assert s["armed"] == 0 and s["adopted"] == 0, s
