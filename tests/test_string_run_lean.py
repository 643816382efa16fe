"""The lean run level of string_compose_sp_kernel (compose.hip): inside a chase run a level reads the matched arc's fields off
its lane, asks for the next rows, and settles the new state under that load — ws = w1 (x) w2, c = (dd + ws) + 0 — where the
run used to park the arc and settle all of its states when it ended.  The string's labels and weights come from a 64-label
chunk in registers that is rotated between the segments of a run, not inside the level.  And the narrow general level: two
to four frontier states whose blocks each fit one 64-arc chunk have all their rows asked for at once and taken in order.

Every case is answered four ways and compared bit for bit (string_cases.four_ways: run on, WFST_STRING_RUN=0, the general
kernel, the oracle), with the composed states and arcs and with string_run_stats() against walk().  What the cases are built
to catch: a sum taken in another order or with a weight of the neighbouring chunk, a level settled from the wrong state, a
row loaded beyond its block, an exit that leaves the run with the wrong rows or on the wrong side of a chunk rotation."""
import functools

import numpy as np
import pytest
import string_cases as sc
from helpers import analyse, finals_of, fst, string, wstring
from string_cases import four_ways, walk

INF = float("inf")
SINGLES = (1, 2, 3)


def singles(n, k0=0):
    return [SINGLES[(k0 + k) % 3] for k in range(n)]


# ================================================================ generators
@functools.lru_cache(maxsize=None)
def sum_t(n=11):
    """every state carries the labels 1..3 once, each arc with its own output label and its own weight off the 1/512 grid:
    every level of a string over 1..3 is one match, and no two additions of a running sum are alike"""
    rows = [[(l, 10 * s + l, 0.1 * (3 * s + l + 1), (s * l + 1) % n) for l in SINGLES] for s in range(n)]
    return fst(rows, finals_of(n, {s: 0.1 * (s % 4) for s in range(n)}))


SUM_RUNS = (63, 64, 65, 66, 127, 128, 129, 130, 193)


@functools.lru_cache(maxsize=None)
def sum_strings():
    """a run of r levels is a string of r + 1 labels (the last level is the general level's).  Weights f32(0.1 * (k + 1)), a
    large second term (every later addition rounds: the order of the sum shows), and -0.0 on the first arc of every other
    (over a non-zero T weight: it only has to leave the product alone; signed_zero_strings has the zeros that keep a sign)"""
    out = []
    for j, r in enumerate(SUM_RUNS):
        w = [0.1 * (k + 1) for k in range(r + 1)]
        w[1] = 3.0e5 + 0.1 * j
        if j % 2:
            w[0] = -0.0
        out.append(wstring(singles(r + 1, j), w, 0.1 * j))
    return out


@functools.lru_cache(maxsize=None)
def short_run_strings():
    """runs of r = 1..6 levels between general levels: after a double match into one state (4: the run resumes at once),
    after two destinations and a collapse (5 8), between two double matches in a row, and in front of the last level.  Then
    strings whose first level already fails the run's test, and one with no run level at all"""
    out = []
    for r in range(1, 7):
        out.append(string(singles(r) + [4] + singles(r, 1) + [5, 8] + singles(r, 2) + [4, 4] + singles(r + 1), 0.25 * (r % 2)))
    out += [string([4] + singles(2) + [4] + singles(1) + [4, 1]), string([5, 8, 4] + singles(3) + [5, 8] + singles(2)),
            string([7, 7, 8] + singles(5) + [4] + singles(4)), string([4, 4, 5, 8, 4])]
    return out


N_CYC = 3


@functools.lru_cache(maxsize=None)
def exit_t():
    """states 0..2: a cycle on label 1 (one match); 2 -> B64 (a block of 64 arcs), 3 -> B65 (65 arcs), 4: two arcs into one
    state, 5: two arcs into two states, 6: no arc, 7 -> Z.  B64, B65 and Z lead back into the cycle on every label they
    carry; Z is the last state, so its block ends at T's last arc"""
    b64, b65, z = N_CYC, N_CYC + 1, N_CYC + 2
    rows = []
    for s in range(N_CYC):
        g = lambda k: (s + k) % N_CYC
        rows.append([(1, 10 + s, 0.1 * (s + 1), g(1)), (2, 20 + s, 0.3, b64), (3, 30 + s, 0.7, b65), (4, 40 + s, 0.9, g(2)),
                     (4, 50 + s, 0.2, g(2)), (5, 60 + s, 0.6, g(1)), (5, 70 + s, 0.4, g(2)), (7, 80 + s, 0.15, z)])
    rows.append([(l, 1000 + l, 0.01 * l, l % N_CYC) for l in range(1, 65)])
    rows.append([(l, 2000 + l, 0.02 * l, l % N_CYC) for l in range(1, 66)])
    rows.append([(l, 3000 + l, 0.03 * l, l % N_CYC) for l in SINGLES])
    return fst(rows, finals_of(N_CYC + 3, {0: 0.0, 1: 0.35, 2: 0.05, z: 0.5}))


EXITS = {"no_match": [6, 1, 1], "same_destination": [4, 1, 1], "two_destinations": [5, 1, 1], "last_level": [1],
         "block_64_arc_0": [2, 1, 1, 1], "block_64_arc_63": [2, 64, 1, 1], "block_65_arc_0": [3, 1, 1, 1],
         "block_65_arc_63": [3, 64, 1, 1], "block_65_arc_64": [3, 65, 1, 1], "last_block_of_t": [7, 3, 1, 1]}
EXIT_AFTER = (0, 1, 2, 3, 63, 64, 65)  # run levels in front of the exit = the string position of the exit


@functools.lru_cache(maxsize=None)
def exit_strings():
    return [string([1] * n + tail, 0.25 * (n % 2)) for tail in EXITS.values() for n in EXIT_AFTER]


N_FAN = 20


@functools.lru_cache(maxsize=None)
def fan_t():
    """string_cases.mix_t with 20 states, so that a level of 7s holds up to 20 states and a slice of 2048 fills within
    ~200 labels.  1, 2, 3: one arc each.  4: two arcs to ONE state.  5: two arcs to two states.  6: no arc.  7: three arcs to
    three states.  8: one arc to state 0"""
    rows = []
    for s in range(N_FAN):
        g = lambda k: (s + k) % N_FAN
        rows.append([(1, 10 + s, ((s * 5) % 9) / 512.0, g(1)), (2, 40 + s, ((s * 7) % 11) / 512.0, g(4)),
                     (3, 70 + s, 0.0, (2 * s + 1) % N_FAN), (4, 100 + s, 3 / 512.0, g(2)), (4, 130 + s, 1 / 512.0, g(2)),
                     (5, 160 + s, 2 / 512.0, g(1)), (5, 190 + s, 1 / 512.0, g(5)), (7, 220 + s, 0.0, g(1)), (7, 250 + s, 5 / 512.0, g(2)),
                     (7, 280 + s, 1 / 512.0, g(3)), (8, 310 + s, (s % 3) / 512.0, 0)])
    return fst(rows, finals_of(N_FAN, {s: s / 512.0 for s in range(N_FAN)}))


LIMIT_CASES = ((0, None), (1, None), (2, None), (3, None), (2, 63), (2, 64), (2, 65))  # (run levels before the exit, its position mod 64)
NO_LIMIT = 1 << 30


def head_states(a, j):
    """composed states after [5 8] * j + [7] * a + [8] against fan_t: 5 8 makes two states and one; the i-th 7 makes
    min(2 i + 1, 20); the last 8 one (checked against walk() in the generators' test)"""
    return 1 + 3 * j + sum(min(2 * i + 1, N_FAN) for i in range(1, a + 1)) + 1


def limit_labels(maxs, k, at):
    """[5 8]* 7* 8 | single-match labels | 4 | k single-match labels | one more | 6 1.  The head fills the slice up to a few
    states, the 4 forces a general level, the run behind it takes k levels, and the label after them would make state
    maxs - 1: hi + 1 == maxs ends the run there with TWO labels left in the string (so the last-level test does not end it
    as well).  The general level makes that state, the 6 finds no arc, and the string is answered with exactly maxs states.
    `at`: the string position of that exit modulo 64"""
    best = None
    for a in range(8, 120):
        for j in range(0, 9):
            head = [5, 8] * j + [7] * a + [8]
            x = maxs - 1 - head_states(a, j) - 1 - k
            if x < 0:
                break
            pos = len(head) + x + 1 + k
            if (at is None or pos % 64 == at % 64) and (best is None or pos + 3 < len(best)):  # the shortest such string
                best = head + singles(x) + [4] + singles(k) + [1, 6, 1]
    assert best is not None, (maxs, k, at)
    return best


@functools.lru_cache(maxsize=None)
def limit_strings(maxs):
    """the exit at hi + 1 == maxs after 0..3 run levels and on both sides of a label chunk; then a string that makes one state
    more than the slice holds (handed back)"""
    out = [string(limit_labels(maxs, k, at)) for k, at in LIMIT_CASES]
    over = limit_labels(maxs, 2, None)
    out.append(string(over[:-2] + [1]))
    return out


@functools.lru_cache(maxsize=None)
def inf_t(zero, n=140):
    """a chain: 1 goes on at a finite weight, 2 goes on at +inf, 3 goes on over two arcs (no run level)"""
    w = lambda s, k: 0.0 if zero else 0.1 * ((s * 3 + k) % 7)
    rows = [[(1, 10 + s, w(s, 0), s + 1), (2, 2000 + s, INF, s + 1), (3, 4000 + s, w(s, 1), s + 1), (3, 6000 + s, w(s, 2), s + 1)]
            for s in range(n)] + [[]]
    return fst(rows, finals_of(n + 1, {s: 0.0 for s in range(n + 1)}))


@functools.lru_cache(maxsize=None)
def signed_zero_t(n=80):
    """a chain: 1 goes on at -0.0, 2 goes on at +0.0, 3 goes on over two arcs at -0.0 and +0.0 (no run level)"""
    rows = [[(1, 10 + s, -0.0, s + 1), (2, 2000 + s, 0.0, s + 1), (3, 4000 + s, -0.0, s + 1), (3, 6000 + s, 0.0, s + 1)]
            for s in range(n)] + [[]]
    return fst(rows, finals_of(n + 1, {s: 0.0 for s in range(n + 1)}))


@functools.lru_cache(maxsize=None)
def signed_zero_strings():
    """w1 (x) w2 is -0.0 only where both are: the arc weights of the path carry that sign, level by level, and the distance
    (dd + ws) + 0.0 stays +0.0 all along.  Lengths on both sides of a label chunk; a 3 at position 2 makes a general level"""
    out = []
    for L in (5, 64, 65, 66, 70):
        for labels, weights in (([1] * L, [-0.0] * L), ([1 + k % 2 for k in range(L)], [-0.0] * L),
                                ([1] * L, [-0.0 if k % 3 else 0.0 for k in range(L)])):
            labels = list(labels)
            if L > 5:
                labels[2] = 3
            out.append(wstring(labels, weights, -0.0 if L % 2 else 0.0))
    return out


INF_L = 131
INF_AT = (0, 3, 63, 64, INF_L - 2)  # a run's first level (the string's, and the one behind the 3 at position 2), the last
                                    # level of a label chunk, the first of the next, the run's last level


@functools.lru_cache(maxsize=None)
def inf_strings(zero):
    base = [1] * INF_L
    base[2] = 3
    out = [wstring(base, [0.0 if zero else 0.1 * (k % 5) for k in range(INF_L)], 0.0 if zero else 0.25)]
    for k in INF_AT:
        labels = list(base)
        labels[k] = 2
        out.append(wstring(labels))
        weights = [0.0 if zero else 0.1 * (j % 3) for j in range(INF_L)]
        weights[k] = INF
        out.append(wstring(base, weights))
    return out


# ================================================================ no GPU
def test_the_generators_promise_their_runs():
    for r, s in zip(SUM_RUNS, sum_strings()):
        assert walk(s["arcs"]["ilabel"], sum_t(), 2048) == (r + 2, 1, r, 1)
    w = sum_t()["arcs"]["weight"]
    assert len(set(w.tolist())) == len(w) and np.mean(w * 512 == np.round(w * 512)) < 0.25  # (0.5 and its like are on the grid)
    assert any(np.signbit(s["arcs"]["weight"][0]) for s in sum_strings())
    for r, s in zip(range(1, 7), short_run_strings()):
        assert walk(s["arcs"]["ilabel"], sc.mix_t(), 2048)[2:] == (4 * r, 4)
    assert walk(short_run_strings()[-1]["arcs"]["ilabel"], sc.mix_t(), 2048)[2:] == (0, 0)
    t, per = exit_t(), len(EXIT_AFTER)
    assert int(t["offsets"][-1]) == int(t["offsets"][-2]) + 3  # Z's block ends T's arcs
    for j, name in enumerate(EXITS):
        for n, s in zip(EXIT_AFTER, exit_strings()[j * per:(j + 1) * per]):
            levels, runs = walk(s["arcs"]["ilabel"], t, 2048)[2:]
            assert levels >= n and runs >= (1 if n else 0), (name, n)
            if name in ("no_match", "last_level"):
                assert (levels, runs) == (n, 1 if n else 0), (name, n)
    for a, j in ((8, 0), (9, 3), (30, 8)):
        assert walk([5, 8] * j + [7] * a + [8], fan_t(), NO_LIMIT)[0] == head_states(a, j)
    for maxs in (512, 2048):
        strs = limit_strings(maxs)
        assert max(s["n_states"] for s in strs) <= 224  # (~200 labels; a packed slice of 512 needs 2 * states + 64 <= 512)
        for (k, at), s in zip(LIMIT_CASES, strs):
            labels = s["arcs"]["ilabel"]
            n, _, levels, runs = walk(labels, fan_t(), maxs)
            # without `hi + 1 < maxs` in the run's test the level at the limit would be one more run level (k == 0: a run more)
            assert n == maxs and walk(labels, fan_t(), NO_LIMIT)[2:] == (levels + 1, runs + (k == 0))
            exit_pos = len(labels) - 3
            assert walk(labels[:exit_pos], fan_t(), NO_LIMIT)[0] == maxs - 1 and exit_pos + 1 < len(labels)
            assert at is None or exit_pos % 64 == at % 64
        assert walk(strs[-1]["arcs"]["ilabel"], fan_t(), maxs)[0] == maxs + 1
    for zero in (False, True):
        for s in inf_strings(zero):
            assert walk(s["arcs"]["ilabel"], inf_t(zero), 2048) == (INF_L + 1, 1, INF_L - 2, 2)


# ================================================================ GPU
@pytest.mark.gpu
def test_sums_in_level_order_across_label_chunks(gpu_ctx, oracle, monkeypatch):
    strs = sum_strings()
    four_ways(gpu_ctx, oracle, monkeypatch, strs, sum_t(), (len(strs),), min_run_levels=sum(SUM_RUNS))


@pytest.mark.gpu
def test_runs_of_one_to_six_levels(gpu_ctx, oracle, monkeypatch):
    strs = short_run_strings()
    four_ways(gpu_ctx, oracle, monkeypatch, strs + strs[:6], sc.mix_t(), (9, 10, 16))


@pytest.mark.gpu
def test_every_exit_after_0_to_3_levels_and_around_a_label_chunk(gpu_ctx, oracle, monkeypatch):
    strs = exit_strings()
    assert len(strs) == 70
    four_ways(gpu_ctx, oracle, monkeypatch, strs, exit_t(), (70,))
    four_ways(gpu_ctx, oracle, monkeypatch, strs[3::9], exit_t(), (8,), scalar="0")  # (8 strings take the run only on request)


@pytest.mark.gpu
def test_exit_at_the_last_state_of_a_packed_slice(gpu_ctx, oracle, monkeypatch):
    strs = limit_strings(512)
    short = [string(singles(2 + j % 4)) for j in range(8)]
    four_ways(gpu_ctx, oracle, monkeypatch, strs + short, fan_t(), (16,))


@pytest.mark.gpu
def test_exit_at_the_last_state_of_an_unpacked_slice(gpu_ctx, oracle, monkeypatch):
    strs = limit_strings(2048)
    short = [string(singles(2 + j % 4)) for j in range(8)]
    four_ways(gpu_ctx, oracle, monkeypatch, strs + short, fan_t(), (16,), unpacked=True)


@pytest.mark.gpu
@pytest.mark.parametrize("zero", [False, True], ids=["weights", "zero_weights"])
def test_unreached_inside_a_run(gpu_ctx, oracle, monkeypatch, zero):
    """+inf on a T arc or on a string arc: every later state has no parent and the string no path; the counters are what
    the walk says, which does not look at weights"""
    strs = inf_strings(zero)
    four_ways(gpu_ctx, oracle, monkeypatch, strs, inf_t(zero), (len(strs),), min_run_levels=len(strs) * (INF_L - 2))


@pytest.mark.gpu
def test_signed_zero_weights_keep_their_sign(gpu_ctx, oracle, monkeypatch):
    strs = signed_zero_strings()
    four_ways(gpu_ctx, oracle, monkeypatch, strs, signed_zero_t(), (len(strs),), min_run_levels=12 * 60)


# ================================================================ narrow frontiers
@functools.lru_cache(maxsize=None)
def narrow_t():
    """the start state fans out to 2, 3, 4 or 5 states on the labels 2..5, to a state of 65 arcs beside one of 1 on 6, and to
    the last state of T on 7 and 8.  A1 (1 arc), A2 (10), A3 (64), A4 (none), A5 (65), then D and E (final), then Z, whose
    block ends T's arcs.  On label 1, A1 and A2 reach D at 3/4 both (the earlier source stays) and A3 reaches it later and
    worse; on label 2, A2 reaches E at 5/4 and A3, later, at 5/8 (the later one is strictly better)"""
    a1, a2, a3, a4, a5, d, e, z = 1, 2, 3, 4, 5, 6, 7, 8
    rows = [[(2, 12, 0.5, a1), (2, 13, 0.25, a2),
             (3, 14, 0.5, a1), (3, 15, 0.25, a2), (3, 16, 0.125, a3),
             (4, 17, 0.5, a1), (4, 18, 0.25, a2), (4, 19, 0.125, a3), (4, 20, 0.0, a4),
             (5, 21, 0.5, a1), (5, 22, 0.25, a2), (5, 23, 0.125, a3), (5, 24, 0.0, a4), (5, 25, 0.375, z),
             (6, 26, 0.5, a1), (6, 27, 0.25, a5),
             (7, 28, 0.25, a2), (7, 29, 0.5, z),
             (8, 30, 0.125, a3), (8, 31, 0.5, z), (8, 32, 0.5, a1)]]
    rows.append([(1, 101, 0.25, d)])
    rows.append([(1, 201, 0.5, d), (2, 202, 1.0, e)] + [(l, 200 + l, 0.1 * l, e if l % 2 else d) for l in range(3, 11)])
    rows.append([(1, 301, 0.75, d), (2, 302, 0.5, e)] + [(l, 300 + l, 0.01 * l, d if l % 2 else e) for l in range(3, 65)])
    rows.append([])
    rows.append([(l, 500 + l, 0.02 * l, d if l % 3 else e) for l in range(1, 66)])
    rows.append([(1, 601, 0.25, d), (2, 602, 0.1, e), (3, 603, 0.3, e)])
    rows.append([(1, 701, 0.2, d), (2, 702, 0.3, d), (2, 703, 0.1, e), (3, 704, 0.1, d)])
    rows.append([(1, 801, 0.3, d), (2, 802, 0.7, e), (3, 803, 0.05, e)])
    return fst(rows, finals_of(9, {d: 0.125, e: 0.0}))


NARROW = ([2, 1, 1], [2, 2, 2], [2, 5, 1], [3, 1, 1], [3, 2, 1], [3, 64, 2], [4, 1, 1], [4, 2, 2, 1], [4, 10, 3], [5, 1, 1], [5, 3, 1],
          [6, 1, 1], [6, 65, 2], [6, 2, 2, 2], [7, 1, 2], [7, 3, 1], [8, 1, 1], [8, 3, 2, 2, 1], [8, 2, 2])


@functools.lru_cache(maxsize=None)
def narrow_strings():
    return [string(s, 0.25 * (k % 2)) for k, s in enumerate(NARROW)]


def test_narrow_generator_has_its_frontiers_and_ties(oracle):
    t = narrow_t()
    assert int(t["offsets"][-1]) - int(t["offsets"][-2]) == 3
    widths = {}
    for s, a in zip(NARROW, narrow_strings()):
        an = analyse(oracle, a, t)
        widths[tuple(s)] = [hi - lo for lo, hi, _, _ in an["levels"]]
    assert [widths[(k, 1, 1)][1] for k in (2, 3, 4, 5)] == [2, 3, 4, 5]
    assert widths[(6, 65, 2)][1] == 2 and widths[(7, 3, 1)][1] == 2 and widths[(8, 1, 1)][1] == 3
    tie = analyse(oracle, narrow_strings()[NARROW.index([3, 1, 1])], t)["path"]
    assert {14, 101} <= set(tie["arcs"]["olabel"].tolist())  # A1, the earlier of the two sources at 3/4
    better = analyse(oracle, narrow_strings()[NARROW.index([3, 2, 1])], t)["path"]
    assert {16, 302} <= set(better["arcs"]["olabel"].tolist())  # A3, the later and strictly better one


def test_signed_zero_generator_has_both_signs_on_its_paths(oracle):
    signs = [np.signbit(analyse(oracle, a, signed_zero_t())["path"]["arcs"]["weight"]) for a in signed_zero_strings()]
    assert all(len(s) == a["n_states"] - 1 for s, a in zip(signs, signed_zero_strings()))  # every string has its path
    assert signs[0].all() and signs[1].any() and not signs[1].all() and signs[2].any() and not signs[2].all()
    assert all(s.any() for s in signs[3:])


@pytest.mark.gpu
def test_narrow_frontiers_ask_for_all_rows_at_once(gpu_ctx, oracle, monkeypatch):
    strs = narrow_strings()
    four_ways(gpu_ctx, oracle, monkeypatch, strs, narrow_t(), (9, len(strs)), min_run_levels=0)
    four_ways(gpu_ctx, oracle, monkeypatch, strs, narrow_t(), (8,), scalar="0", min_run_levels=0)
