"""The chase run of string_compose_sp_kernel (compose.hip): a level with ONE frontier state, a block of at most 64 arcs, ONE
matching arc, a level behind it in the string and two free states in the LDS slice is taken by a loop that only follows the
matched arc; the run's distances, parents and arc weights are settled when it ends.

Every case is answered four times and compared bit for bit: WFST_STRING_RUN=1, WFST_STRING_RUN=0, the general kernel
(WFST_STRING_KERNEL=0) and the oracle — path arcs, weights and final weight of every string, and the composed states and arcs
the call reports (the per-problem level count is not exposed by the API; states and arcs are).  Context.string_run_stats() is
compared with what a pure-Python walk of the lattice predicts, so a run that is silently switched off fails the test."""
import functools

import numpy as np
import pytest

from rustfst_amd import synth

import helpers
from helpers import finals_of, fst, string, wstring
import string_cases as sc
from string_cases import four_ways, mix_t, predict, walk

INF = float("inf")


# ================================================================ generators
INTERRUPTS = {"same_destination": [4], "two_destinations": [5, 8], "two_destinations_stay": [5], "no_match": [6], "fan_and_collapse": [7, 7, 8]}


@functools.lru_cache(maxsize=None)
def interrupted_strings(L=21):
    """single-match labels with each interrupt at positions 0, 1, mid and L - 2 (its first label), and the plain string"""
    rng = np.random.default_rng(21)
    base = [int(x) for x in rng.integers(1, 4, L)]
    out = [string(base)]
    for ins in INTERRUPTS.values():
        for pos in (0, 1, L // 2, L - 2):
            s = list(base)
            s[pos:pos + len(ins)] = ins
            out.append(string(s))
    return out


RUN_LENGTHS = (1, 2, 3, 63, 64, 65, 66, 128, 129, 130)


@functools.lru_cache(maxsize=None)
def chain_t(n=7):
    """every state has ONE arc per label 1..3 with its own output label and weight (zeros among them): every level of a
    string over 1..3 is one match, and a label read from the wrong place changes the path"""
    rows = [[(l, 10 * s + l, ((s * 37 + l * 5) % 11) / 512.0, (s * l + 1) % n) for l in (1, 2, 3)] for s in range(n)]
    return fst(rows, finals_of(n, {s: (s % 4) / 512.0 for s in range(n)}))


@functools.lru_cache(maxsize=None)
def block_t():
    """state 1 has 64 arcs (labels 1..64), state 2 has 65 (labels 1..65); state 0 goes to 1 on label 1 and to 2 on label 2"""
    rows = [[(1, 500, 0.25, 1), (2, 501, 0.5, 2)],
            [(l, 1000 + l, (l % 5) / 512.0, 3) for l in range(1, 65)],
            [(l, 2000 + l, (l % 7) / 512.0, 3) for l in range(1, 66)],
            [(1, 3001, 1 / 512.0, 3), (2, 3002, 0.0, 0)]]
    return fst(rows, finals_of(4, {3: 0.0, 0: 0.5}))


@functools.lru_cache(maxsize=None)
def inf_t(n=140):
    """a chain: label 1 goes on at a finite weight, label 2 goes on at +inf"""
    rows = [[(1, 10 + s, ((s * 3) % 7) / 512.0, s + 1), (2, 2000 + s, INF, s + 1)] for s in range(n)] + [[]]
    return fst(rows, finals_of(n + 1, {s: 0.0 for s in range(n + 1)}))


# ================================================================ no GPU
def test_new_symbol_declared_exported_and_bound(wfst_lib):
    import ctypes as C
    import rustfst_amd
    name = "wfst_ctx_get_string_run_stats"
    helpers.check_counter_getter(wfst_lib, name, ("run_levels", "runs"), rustfst_amd.Context.string_run_stats)
    v = C.c_uint64(5)
    assert wfst_lib.wfst_ctx_get_string_run_stats(None, C.byref(v), C.byref(v)) != 0 and v.value == 5


def test_the_walk_counts_what_the_generators_promise():
    """every level but the last of a string over 1..3 against chain_t is a run level, in one run; an interrupt splits it"""
    for n in RUN_LENGTHS:
        s = string([1 + k % 3 for k in range(n)])
        assert walk(s["arcs"]["ilabel"], chain_t(), 2048) == (n + 1, 1, n - 1, 1 if n > 1 else 0)
    plain, at0, at1, mid, late = interrupted_strings()[:5]  # (same_destination)
    L = plain["n_states"] - 1
    assert walk(plain["arcs"]["ilabel"], mix_t(), 2048) == (L + 1, 1, L - 1, 1)
    assert walk(at0["arcs"]["ilabel"], mix_t(), 2048) == (L + 1, 1, L - 2, 1)
    assert walk(at1["arcs"]["ilabel"], mix_t(), 2048) == (L + 1, 1, L - 2, 2)
    assert walk(mid["arcs"]["ilabel"], mix_t(), 2048) == (L + 1, 1, L - 2, 2)
    assert walk(late["arcs"]["ilabel"], mix_t(), 2048) == (L + 1, 1, L - 2, 1)
    assert walk(string([1, 1, 1, 1])["arcs"]["ilabel"], block_t(), 2048)[2:] == (3, 1)   # the block of 64 is in the run
    assert walk(string([2, 1, 1, 1])["arcs"]["ilabel"], block_t(), 2048)[2:] == (2, 2)   # the block of 65 ends it


# ================================================================ GPU
@pytest.mark.gpu
def test_run_lengths_around_the_label_chunks(gpu_ctx, oracle, monkeypatch):
    rng = np.random.default_rng(130)
    strs = [string(rng.integers(1, 4, n), 0.25 * (k % 2)) for k, n in enumerate(RUN_LENGTHS)]
    four_ways(gpu_ctx, oracle, monkeypatch, strs, chain_t(), (len(strs),))


@pytest.mark.gpu
def test_interrupted_and_resumed_runs_in_every_batch_shape(gpu_ctx, oracle, monkeypatch):
    """each interrupt at positions 0, 1, mid and L - 2; batches of 8 (scalar rows: no run), 9 (unpacked), 16 and 17 (packed)"""
    strs = interrupted_strings()
    assert len(strs) == 21
    four_ways(gpu_ctx, oracle, monkeypatch, strs, mix_t(), (8, 9, 16, 17, 21))
    four_ways(gpu_ctx, oracle, monkeypatch, strs, mix_t(), (21,), unpacked=True)
    want, _ = predict(strs[:8], mix_t(), None, False)
    assert want == dict(run_levels=0, runs=0)


@pytest.mark.gpu
def test_blocks_of_64_and_65_arcs(gpu_ctx, oracle, monkeypatch):
    """the match in the first and in the last lane of a block of 64 (in the run) and of 65 (ends it: its last arc is the
    general level's second chunk)"""
    strs = [string(s) for s in ([1, 1, 1, 1], [1, 64, 1, 1], [2, 1, 1, 1], [2, 65, 1, 1], [1, 64, 2, 1, 64, 1], [2, 64, 2, 2, 65, 1])]
    four_ways(gpu_ctx, oracle, monkeypatch, strs * 2, block_t(), (12,))


@pytest.mark.gpu
def test_infinite_and_zero_weights_inside_a_run(gpu_ctx, oracle, monkeypatch):
    """a +inf arc weight (label 2 of inf_t) or a +inf string-arc weight at the first, a middle and the last level of a run of
    130 levels: every later state is unreached and there is no path; and the finite running sum over the whole run"""
    L = 131
    strs = [wstring([1] * L, [((k * 5) % 13) / 512.0 for k in range(L)], 0.25)]
    for k in (0, L // 2, L - 2):
        labels = [1] * L
        labels[k] = 2
        strs.append(wstring(labels))
        weights = [(j % 3) / 512.0 for j in range(L)]
        weights[k] = INF
        strs.append(wstring([1] * L, weights))
    strs += [wstring([1] * 5)] * 2
    four_ways(gpu_ctx, oracle, monkeypatch, strs, inf_t(), (len(strs),), min_run_levels=7 * (L - 1))


@pytest.mark.gpu
def test_state_limit_unpacked(gpu_ctx, oracle, monkeypatch):
    """2048 composed states are taken (the run stops one state short of the slice), 2049 are handed back as
    test_string_of_2048_states_is_taken_and_2049_is_not expects"""
    strs = [string([1] * 2047), string([1] * 2048)]
    assert walk(strs[0]["arcs"]["ilabel"], sc.ladder_t(1), 2048) == (2048, 1, 2046, 1)
    four_ways(gpu_ctx, oracle, monkeypatch, strs, sc.ladder_t(1), (2,), scalar="0", min_run_levels=2046)


@pytest.mark.gpu
def test_state_limit_packed(gpu_ctx, oracle, monkeypatch):
    """a packed batch of 16 (slice 512) whose longest string reaches state 511 inside a run: levels of up to 9 states, a
    collapse, then one state per level until the slice is full; one label more is handed back"""
    t = mix_t()
    head = [7] * 50 + [8]
    tail = next(r for r in range(1, 200) if walk(head + [1 + k % 3 for k in range(r)], t, 512)[0] == 512)
    strs = [string(head + [1 + k % 3 for k in range(tail + extra)]) for extra in (0, -1, 1)]
    assert [walk(s["arcs"]["ilabel"], t, 512)[0] for s in strs] == [512, 511, 513]
    assert 2 * strs[2]["n_states"] + 64 <= 512
    short = [string([1 + k % 3 for k in range(2 + j % 4)]) for j in range(13)]
    four_ways(gpu_ctx, oracle, monkeypatch, strs + short, t, (16,), min_run_levels=2 * (tail - 2))
    four_ways(gpu_ctx, oracle, monkeypatch, strs[:2] + short + [strs[2]], t, (15,), scalar="0")  # (unpacked: 2048 states each)


@pytest.mark.gpu
@pytest.mark.parametrize("sigma", [256, 16, 8])
def test_small_random_t(gpu_ctx, oracle, monkeypatch, sigma):
    """300 states, fan-out 10; 17 strings of 70 labels.  256 labels: most levels are single-match.  16: most are not, and the
    string kernel still answers every problem.  8: every problem outgrows its slice in the middle of its levels and is handed
    back (runs that were taken are thrown away with the rest of the attempt: the counters are 0)"""
    t = synth.make_transducer(300, 10, sigma, 0.0, seed=5)
    strs = synth.make_acceptors(t, 17, 70, seed0=1000)
    want, answered = predict(strs, t, None, False)
    levels = 17 * 70
    if sigma == 256:
        assert answered == 17 and want["run_levels"] > levels // 2
    elif sigma == 16:
        assert answered == 17 and 0 < want["run_levels"] < levels // 4
    else:
        assert answered == 0 and want == dict(run_levels=0, runs=0)
    four_ways(gpu_ctx, oracle, monkeypatch, strs, t, (17,), min_run_levels=1 if answered else 0)
