"""wfst_rm_epsilon at every scratch limit, kernel hand-over and cycle order.

Without a GPU: the C-ABI and Python surface of wfst_ctx_get_rm_epsilon_stats, a plain Python restatement of the reference's
rewrite for inputs whose epsilon graph is acyclic (checked against the oracle), and the needs (closure states, stack
entries, arcs) of every input family below, so that a family that stops hitting its edge fails here.

On the device: every case bit-exact against the oracle, property word included, and for epsilon-acyclic cases the counters
of the call (which kernel ran, how often, how many states finished where) against what the restatement predicts from the
needs and the retry ladder.  Result parity alone cannot see a capacity comparison that is off by one: only the number of
retries changes.  Weights are on the 1/512 grid, where the exact minimum the kernels compute is the reference's distance."""
import ctypes as C
import functools
import inspect

import numpy as np
import pytest

from rustfst_amd import synth as P

import helpers
from helpers import assert_flat_identical, random_fst_flat, to_device, to_oracle
from rm_epsilon_cases import (Builder, STAT_KEYS, chain, expected_stats, fan, par, props_hand_made, props_random_inputs,
                              rm_epsilon_model, value_cases, wide)

WAVE_COMPONENT = 64  # members of an epsilon component larger than this go straight to the wave kernel (`closure_hint > 64`)


# ---------------------------------------------------------------- inputs
def ladder(length):
    """a chain 1 -> 2 -> ... -> length of cheap epsilon arcs, every chain state with one labelled arc, and one expensive
    epsilon arc from the root to every chain state but the first, which it reaches by a cheap one: (length + 1, length,
    length).  The root's arcs list the chain backwards, so the closure is discovered farthest state first and every
    distance improves one hop per label-correcting round whichever way a round sweeps the closure."""
    b = Builder()
    root = b.state()
    states = [b.state() for _ in range(length)]
    sink = b.state(final=256)
    for i in range(length - 1, 0, -1):
        b.eps(root, 2048, states[i])
    b.eps(root, 1, states[0])
    for i, q in enumerate(states):
        if i + 1 < length:
            b.eps(q, 1, states[i + 1])
        b.arc(q, i + 1, i + 1, (i * 13) % 97, sink)
    return b.flat()


FAMILIES = {"fan": fan, "chain": chain, "par": par, "wide": wide, "ladder": ladder}
FAMILY_CASES = ([("chain", c - 1, (c, 1, 1)) for c in (16, 17, 64, 65, 1024, 1025)]
                + [("par", p, (2, p, 1)) for p in (32, 33, 128, 129, 1024, 1025)]
                + [("wide", a, (2, 1, a)) for a in (32, 33, 128, 129, 1024, 1025)]
                + [("fan", m, (m + 1, m, m)) for m in (15, 16, 63, 64, 1023, 1024)]
                + [("ladder", n, (n + 1, n, n)) for n in (14, 60, 200, 1100)])
FAMILY_IDS = ["%s-%d" % (name, size) for name, size, _ in FAMILY_CASES]


@functools.lru_cache(maxsize=None)
def family(name, size):
    flat = FAMILIES[name](size)
    return flat, rm_epsilon_model(flat)


DUP_POSITIONS = (3, 67, 129)
CHUNK_CASES = [(a, m, a == 130) for a in (130, 192, 193) for m in DUP_POSITIONS]  # (130 - 3 arcs fit the thread kernel)


def chunk_case(a, min_at, force_wave):
    """wide(a) whose arcs 3, 67 and 129 share one (ilabel, olabel, nextstate), the smallest weight at `min_at`; arcs 10
    and 20 share a second key inside one chunk of 64; a second closure state, walked first, holds the keys of arcs 5
    (cheaper there) and 100 (cheaper here).  force_wave: 129 parallel epsilon arcs send the rewrite to the wave kernel."""
    b = Builder()
    root, w, v, sink = b.state(), b.state(), b.state(), b.state(final=256)
    for i in range(129 if force_wave else 1):
        b.eps(root, 5 + i, w)
    b.eps(root, 3, v)  # (pushed last: popped and walked first)
    for i in range(a):
        if i in DUP_POSITIONS:
            b.arc(w, 7777, 7777, 10 if i == min_at else 50 + i, sink)
        elif i in (10, 20):
            b.arc(w, 8888, 8889, 60 - i, sink)
        else:
            b.arc(w, i + 1, i + 1, 100 + (i * 37) % 64, sink)
    b.arc(v, 6, 6, 20, sink)
    b.arc(v, 101, 101, 900, sink)
    return b.flat()


def push_case():
    """under the root one state with 100 arcs, 70 of them epsilon arcs to distinct unvisited targets (the 64th arc lies
    between them); some targets also reach the next one, which is then walked before its own stack entry comes up"""
    b = Builder()
    root, x = b.state(), b.state()
    b.eps(root, 2, x)
    targets = [b.state(final=(40 + j if j % 9 == 0 else None)) for j in range(70)]
    sink = b.state(final=256)
    j = 0
    for i in range(100):
        if i % 10 < 7:
            b.eps(x, (i * 5) % 31, targets[j])
            j += 1
        else:
            b.arc(x, 500 + i, 500 + i, i, sink)
    for j, t in enumerate(targets):
        b.arc(t, 200 + j % 60, 200 + j % 60, (j * 13) % 97, sink)  # (the last ten repeat keys of the first ten)
        if j % 5 == 0 and j + 1 < len(targets):
            b.eps(t, 1, targets[j + 1])
    return b.flat()


def arena_case():
    """states that read rewritten successors out of the arenas of earlier attempts:
    q  (depth 0) 210 arcs, 200 distinct: finishes in the wave kernel
    r  (depth 1) an epsilon arc to q: 201 arcs, the wave kernel reads q from its arena; r1 beside it has a closure of two
       and finishes in the first thread launch of the same batch
    q2 (depth 1) 129 parallel epsilon arcs to a state with 20 arcs: the wave kernel, 20 arcs
    r2 (depth 2) an epsilon arc to q2: the thread kernel reads q2 from the arena of a wave attempt
    r3 (depth 2) epsilon arcs to r and q2: the wave kernel reads both, and q2's keys are twenty of those r took from q"""
    b = Builder()
    hub, q, r, r1, z, q2, z2, r2, r3 = (b.state() for _ in range(9))
    sink = b.state(final=256)
    for i, s in enumerate((q, r, r1, q2, r2, r3)):
        b.arc(hub, 900 + i, 900 + i, 3 * i, s)
    for i in range(210):
        k = i - 200 if i >= 200 else i  # the last ten repeat the first ten keys
        b.arc(q, k + 1, k + 1, (i * 29) % 113, sink)
    b.eps(r, 4, q)
    b.arc(r, 300, 300, 1, sink)
    b.eps(r1, 6, z)
    for i in range(3):
        b.arc(z, 10 + i, 20 + i, i, sink)
    for i in range(129):
        b.eps(q2, 1 + (i * 7) % 129, z2)
    for i in range(20):
        b.arc(z2, 40 + i, 40 + i, (i * 5) % 17, sink)
    b.eps(r2, 8, q2)
    b.arc(r2, 301, 301, 2, sink)
    b.eps(r3, 2, r)
    b.eps(r3, 1, q2)
    return b.flat()


MIXED_ARCS = (5, 100, 500, 1025, 0)  # first / second thread size, first / second wave size, no arcs


def mixed_case():
    """one depth-0 batch of fifteen states in interleaved id order, three each of MIXED_ARCS (plus the hub and the sink),
    and above every one a depth-1 state that reads it"""
    b = Builder()
    hub = b.state()
    sink = b.state(final=256)
    for i in range(15):
        n_arcs = MIXED_ARCS[i % 5]
        item = b.state(final=None if n_arcs else 7 + i)
        upper = b.state()
        b.arc(hub, 2000 + i, 2000 + i, i, item)
        b.arc(hub, 3000 + i, 3000 + i, i, upper)
        for k in range(n_arcs):
            b.arc(item, k + 1, k + 1, (k * 13 + i) % 97, sink)
        b.eps(upper, 1 + i, item)
        b.arc(upper, 4000, 4000, 3, sink)
    return b.flat()


def ring(k, seed=None, hub_every=1, two=False):
    """a ring of k epsilon arcs, a labelled arc out of every member to the sink, a start hub with labelled arcs into every
    hub_every-th member (through one more hub per 100 members, so that no hub outgrows the thread kernel).  seed: ids
    permuted.  two: a second ring one epsilon depth up, joined by an epsilon arc.
    Returns (flat, number of rewritten ring members, number of rewritten states outside the rings)."""
    b = Builder()
    hub = b.state()
    rings = [[b.state() for _ in range(k)] for _ in range(2 if two else 1)]
    rewritten, hubs = 0, []
    for ri, members in enumerate(rings):
        for i, s in enumerate(members):
            b.eps(s, 1 + (i * 3 + ri) % 5, members[(i + 1) % k])
            if i % hub_every == 0:
                if rewritten % 100 == 0:
                    hubs.append(b.state())
                    b.arc(hub, 5000 + len(hubs), 5000 + len(hubs), len(hubs), hubs[-1])
                b.arc(hubs[-1], 1000 * (ri + 1) + i, 7, i % 11, s)
                rewritten += 1
    sink = b.state(final=256)
    for ri, members in enumerate(rings):
        for i, s in enumerate(members):
            b.arc(s, 1 + i, 1 + i + ri, (i * 13) % 97, sink)
    if two:
        b.eps(rings[1][0], 2, rings[0][3 % k])
    perm = None
    if seed is not None:
        perm = np.arange(len(b.trs))
        ids = perm[1:-1].copy()
        np.random.default_rng(seed).shuffle(ids)
        perm[1:-1] = ids
    return b.flat(perm=perm), rewritten, len(hubs) + 2


# ================================================================ no GPU
def test_stats_symbol_declared_exported_and_bound(wfst_lib):
    import rustfst_amd
    helpers.check_counter_getter(wfst_lib, "wfst_ctx_get_rm_epsilon_stats", STAT_KEYS, rustfst_amd.rm_epsilon_stats)


def test_stats_null_context_is_ko(wfst_lib):
    assert "null" in helpers.ko_message(wfst_lib.wfst_ctx_get_rm_epsilon_stats(None, None, None, None, None, None, None))
    vals = [C.c_uint64(7) for _ in STAT_KEYS]
    assert "null" in helpers.ko_message(wfst_lib.wfst_ctx_get_rm_epsilon_stats(None, *[C.byref(v) for v in vals]))
    assert [v.value for v in vals] == [7] * len(STAT_KEYS)


def test_python_surface():
    import rustfst_amd
    assert "rm_epsilon_stats" in rustfst_amd.__all__ and hasattr(rustfst_amd, "rm_epsilon_stats")
    p = inspect.signature(rustfst_amd.rm_epsilon_stats).parameters
    assert list(p) == ["ctx"] and p["ctx"].default is None


def assert_model_is_oracle(oracle, flat, what):
    model, needs, stats = rm_epsilon_model(flat)
    got = to_oracle(oracle, model)
    got.connect()
    ref = to_oracle(oracle, flat)
    ref.rm_epsilon()
    assert_flat_identical(got.to_flat(), ref.to_flat(), what, check_props=False)
    return needs, stats


def test_model_against_oracle(oracle):
    rng = np.random.default_rng(1234)
    with_arcs = 0
    for k in range(200):
        f = random_fst_flat(rng, int(rng.integers(1, 40)), 3, 3, p_eps_i=0.5, p_eps_o=0.5, p_final=0.3, acyclic=True,
                            sort=("none", "ilabel")[k % 2])
        if not np.isfinite(f["finals"]).any():
            f["finals"][-1] = 1.0
        needs, _ = assert_model_is_oracle(oracle, f, "random %d" % k)
        with_arcs += any(c > 1 for c, _, _ in needs.values())
    assert with_arcs > 100  # (the inputs do have closures to walk)


@pytest.mark.parametrize("name,size,need", FAMILY_CASES, ids=FAMILY_IDS)
def test_family_needs(oracle, name, size, need):
    """the start state of every family needs exactly what the family is there for, and the model is the oracle on it"""
    flat, (_, needs, stats) = family(name, size)
    assert needs[0] == need
    assert {s: v for s, v in needs.items() if s} == {flat["n_states"] - 1: (1, 1, 0)}  # (only the sink beside it)
    assert stats["batches"] == 2
    assert_model_is_oracle(oracle, flat, "%s(%d)" % (name, size))


def test_expected_stats_of_the_ladder():
    """the prediction itself at the rungs: fits at a capacity, retries one above it"""
    def one(need):
        return expected_stats([[need]])
    assert one((16, 32, 32)) == dict(batches=1, thread_launches=1, wave_launches=0, states_thread=1, states_wave=0,
                                     max_closure_cap=16)
    for need in ((17, 1, 1), (2, 33, 1), (2, 1, 33), (64, 128, 128)):
        assert one(need) == dict(batches=1, thread_launches=2, wave_launches=0, states_thread=1, states_wave=0,
                                 max_closure_cap=64), need
    for need in ((65, 1, 1), (2, 129, 1), (2, 1, 129), (1024, 1024, 1024)):
        assert one(need) == dict(batches=1, thread_launches=2, wave_launches=1, states_thread=0, states_wave=1,
                                 max_closure_cap=1024), need
    for need in ((1025, 1, 1), (2, 1025, 1), (2, 1, 1025)):
        assert one(need) == dict(batches=1, thread_launches=2, wave_launches=2, states_thread=0, states_wave=1,
                                 max_closure_cap=4096), need
    assert expected_stats([[(1, 1, 0), (2, 1, 1025)], [(17, 1, 1)]]) == dict(
        batches=2, thread_launches=4, wave_launches=2, states_thread=2, states_wave=1, max_closure_cap=4096)


def test_hand_made_inputs_are_what_they_claim(oracle):
    """the model is the oracle on every epsilon-acyclic hand-made input, and the inputs reach the kernels they are for"""
    for a, min_at, force in CHUNK_CASES:
        needs, stats = assert_model_is_oracle(oracle, chunk_case(a, min_at, force), "chunk")
        assert needs[0] == (3, 130 if force else 2, a - 3) and stats["states_wave"] == 1
    needs, stats = assert_model_is_oracle(oracle, push_case(), "push")
    assert needs[0][0] == 72 and stats["states_wave"] == 1
    needs, stats = assert_model_is_oracle(oracle, arena_case(), "arena")
    assert [needs[s] for s in (1, 2, 3, 5, 7, 8)] == [(1, 1, 200), (2, 1, 201), (2, 1, 3), (2, 129, 20), (2, 1, 21),
                                                      (3, 2, 201)]  # (q2's twenty keys are twenty of q's)
    assert stats["batches"] == 3 and stats["states_wave"] == 4
    needs, stats = assert_model_is_oracle(oracle, mixed_case(), "mixed")
    assert stats == dict(batches=2, thread_launches=4, wave_launches=4, states_thread=2 + 9 + 9, states_wave=6 + 6,
                         max_closure_cap=4096)
    for name, (flat, acyclic) in value_cases().items():
        if acyclic:
            assert_model_is_oracle(oracle, flat, name)
    for name, flat in props_random_inputs()[::3] + props_hand_made():
        assert_model_is_oracle(oracle, flat, name)


def test_property_inputs_give_distinct_words(oracle):
    words = set()
    for name, flat in props_random_inputs() + props_hand_made():
        words.add(to_oracle(oracle, flat).rm_epsilon().properties)
    assert len(words) >= 3, [hex(w) for w in words]
    # every hand-made pair differs in exactly the bit it is made for
    hand = [to_oracle(oracle, flat).rm_epsilon().properties for _, flat in props_hand_made()]
    assert not hand[0] & P.ACCEPTOR and hand[1] & P.ACCEPTOR
    assert not hand[2] & P.TOP_SORTED and hand[3] & P.TOP_SORTED
    assert hand[4] & P.ACYCLIC and not hand[4] & P.TOP_SORTED and not hand[5] & P.ACYCLIC


# ================================================================ device
def run(gpu_ctx, oracle, flat, what, model=True, expected=None):
    """rm_epsilon on the device against the oracle, bit for bit; the counters against the model.  Returns the counters."""
    import rustfst_amd
    ref = to_oracle(oracle, flat)
    ref.rm_epsilon()
    got = to_device(flat, gpu_ctx).rm_epsilon().to_flat()
    stats = rustfst_amd.rm_epsilon_stats(gpu_ctx)
    if model and expected is None:
        expected = rm_epsilon_model(flat)[2]
    print("%s: counters %s, model %s" % (what, stats, expected))
    assert_flat_identical(got, ref.to_flat(), what)
    if model:
        assert stats == expected, what
    return stats


@pytest.mark.gpu
@pytest.mark.parametrize("name,size,need", FAMILY_CASES, ids=FAMILY_IDS)
def test_family_on_device(gpu_ctx, oracle, name, size, need):
    flat, (_, _, expected) = family(name, size)
    run(gpu_ctx, oracle, flat, "%s(%d)" % (name, size), expected=expected)


@pytest.mark.gpu
@pytest.mark.parametrize("a,min_at,force_wave", CHUNK_CASES)
def test_wave_chunks_combine_duplicates(gpu_ctx, oracle, a, min_at, force_wave):
    stats = run(gpu_ctx, oracle, chunk_case(a, min_at, force_wave), "chunk(%d, min at %d)" % (a, min_at))
    assert stats["states_wave"] == 1
    if a == 130:  # the same arcs through the thread kernel
        stats = run(gpu_ctx, oracle, chunk_case(a, min_at, False), "chunk(%d, min at %d), thread" % (a, min_at))
        assert stats["states_wave"] == 0


@pytest.mark.gpu
def test_wave_push_order_across_a_chunk(gpu_ctx, oracle):
    assert run(gpu_ctx, oracle, push_case(), "push")["states_wave"] == 1


@pytest.mark.gpu
def test_rewritten_successors_are_read_from_the_arenas(gpu_ctx, oracle):
    stats = run(gpu_ctx, oracle, arena_case(), "arena")
    assert stats["states_wave"] == 4 and stats["batches"] == 3


@pytest.mark.gpu
def test_one_mixed_batch(gpu_ctx, oracle):
    stats = run(gpu_ctx, oracle, mixed_case(), "mixed")
    assert stats["thread_launches"] == 4 and stats["wave_launches"] == 4


@pytest.mark.gpu
@pytest.mark.parametrize("k", (2, 16, 64, 65, 300))
def test_epsilon_ring(gpu_ctx, oracle, k):
    flat, members, others = ring(k)
    stats = run(gpu_ctx, oracle, flat, "ring(%d)" % k, model=False)
    assert members == k and stats["batches"] == k + 1  # hubs and sink together, then one batch per member
    assert stats["states_wave"] == (0 if k <= WAVE_COMPONENT else members)
    assert stats["states_thread"] + stats["states_wave"] == members + others


@pytest.mark.gpu
@pytest.mark.parametrize("k", (64, 65))
@pytest.mark.parametrize("variant", ("permuted", "every_third", "two_rings"))
def test_epsilon_ring_variants(gpu_ctx, oracle, k, variant):
    flat, members, others = ring(k, seed=77 + k if variant == "permuted" else None, hub_every=3 if variant == "every_third" else 1,
                         two=variant == "two_rings")
    stats = run(gpu_ctx, oracle, flat, "ring(%d) %s" % (k, variant), model=False)
    assert stats["batches"] == members + 1
    if variant != "two_rings":
        assert stats["states_wave"] == (0 if k <= WAVE_COMPONENT else members)
    else:  # the upper ring's closures run into the lower ring: 65 states and more, whatever the component's size
        assert stats["states_wave"] >= 1
    assert stats["states_thread"] + stats["states_wave"] == members + others


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(value_cases()))
def test_values(gpu_ctx, oracle, name):
    flat, acyclic = value_cases()[name]
    run(gpu_ctx, oracle, flat, name, model=acyclic)


@pytest.mark.gpu
def test_no_start_leaves_the_counters_zero(gpu_ctx, oracle):
    flat = fan(15)
    assert run(gpu_ctx, oracle, flat, "fan(15)")["batches"] == 2  # (counters that the next call has to clear)
    stats = run(gpu_ctx, oracle, dict(flat, start=-1), "no start", model=False)
    assert stats == dict.fromkeys(STAT_KEYS, 0)


@pytest.mark.gpu
def test_property_word(gpu_ctx, oracle):
    words = set()
    for name, flat in props_random_inputs() + props_hand_made():
        run(gpu_ctx, oracle, flat, name)
        words.add(to_oracle(oracle, flat).rm_epsilon().properties)
    assert len(words) >= 3
