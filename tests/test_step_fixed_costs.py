"""The fixed costs taken out of one serving step (string o T batch beside shortest_path(T)): path slices handed out by the
host, the parent walk by the whole wave, early issue of the next level's rows, the tail of a query over the handle's list
of final states, and one pass over the environment per solve / batch call.  Every result is compared bit for bit with
the CPU oracle and with the library's other path for the same input."""
import numpy as np
import pytest

import rustfst_amd
from rustfst_amd import synth
from rustfst_amd._lib import TR_DTYPE
from helpers import NOT_O_LABEL_SORTED, assert_flat_identical, to_device, to_oracle

pytestmark = pytest.mark.gpu

SIGMA = 4
N_POS = 150  # T of the string tests: 150 positions x 2 variants = 300 states; every arc goes to the next position


def _flat_from_rows(rows, finals):
    """Flat CSR from per-state arc lists (already sorted by ilabel)."""
    offsets = np.zeros(len(rows) + 1, dtype=np.uint32)
    offsets[1:] = np.cumsum([len(r) for r in rows])
    arcs = np.array([a for r in rows for a in r], dtype=TR_DTYPE)
    ol_sorted = all(all(r[i][1] <= r[i + 1][1] for i in range(len(r) - 1)) for r in rows)
    props = synth.I_LABEL_SORTED | (synth.O_LABEL_SORTED if ol_sorted else NOT_O_LABEL_SORTED)
    return dict(n_states=len(rows), start=0, offsets=offsets, arcs=arcs, finals=np.asarray(finals, dtype=np.float32), props=props)


def _string_t():
    """300 states, sigma = 4, fan-out 3-6.  State 2p + v is variant v of position p and its arcs go to the two variants of
    position p + 1, so a level of the composition has one or two states (a string of 200 labels composes to fewer than
    512 states: the packed string kernel keeps every problem) while labels match 0, 1, 2 or more arcs of a state and two
    arcs often meet in one destination.  State 0 and state 2 carry each label at most once (single-match levels); state 4
    carries 70 arcs, its label-4 run across the 64-arc chunk boundary, and is reached by the labels 1 1."""
    rng = np.random.default_rng(20_240)
    rows = []
    for s in range(2 * N_POS):
        nxt = 2 * ((s // 2 + 1) % N_POS)
        k = int(rng.integers(3, 7))
        arcs = [(int(rng.integers(1, SIGMA + 1)), int(rng.integers(1, SIGMA + 1)), float(rng.integers(0, 2560)) / 512.0,
                 nxt + int(rng.integers(0, 2))) for _ in range(k)]
        rows.append(sorted(arcs, key=lambda a: a[0]))
    rows[0] = [(1, 3, 0.5, 2), (2, 1, 1.25, 3), (3, 2, 0.75, 2)]
    rows[2] = [(1, 2, 0.25, 4), (2, 4, 2.0, 5), (3, 1, 1.5, 4)]
    big = [(1 + (i * SIGMA) // 70, int(rng.integers(1, SIGMA + 1)), float(rng.integers(0, 2560)) / 512.0, 6 + int(rng.integers(0, 2)))
           for i in range(70)]
    assert [a[0] for a in big] == sorted(a[0] for a in big) and big[63][0] == 4 and big[64][0] == 4 and big[50][0] == 3
    rows[4] = big
    finals = np.where(rng.random(2 * N_POS) < 0.5, rng.integers(0, 2560, 2 * N_POS) / 512.0, np.inf)
    for p in (1, 2, 63, 64, 65, 129, 200 % N_POS, 30):  # where the walks of the tested lengths end: paths exist
        finals[2 * p:2 * p + 2] = [0.5, 1.0]
    finals[10:12] = np.inf  # position 5: a string of 5 matching labels reaches no final state
    return _flat_from_rows(rows, finals)


def _walk(t, rng, length, prefix=()):
    """Labels along a walk through T that starts with `prefix` (the first arc carrying each prefix label is followed)."""
    s, labs = int(t["start"]), []
    for i in range(length):
        b, e = int(t["offsets"][s]), int(t["offsets"][s + 1])
        if i < len(prefix):
            k = b + int(np.flatnonzero(t["arcs"]["ilabel"][b:e] == prefix[i])[0])
        else:
            k = int(rng.integers(b, e))
        labs.append(int(t["arcs"]["ilabel"][k]))
        s = int(t["arcs"]["nextstate"][k])
    return labs


def _string_batch(t):
    rng = np.random.default_rng(99)
    labs = [_walk(t, rng, n) for n in (1, 2, 63, 64, 65, 129, 200)]
    labs.append(_walk(t, rng, 30, prefix=(1, 1, 4)))   # single match, single match, then the 70-arc block (matches in both chunks)
    labs.append(_walk(t, rng, 64, prefix=(1, 1, 1)))   # ... with its matches in the first chunk only
    labs.append(_walk(t, rng, 30) + [9] + _walk(t, rng, 20))  # dead end in the middle (label 9 is not in T)
    labs.append(_walk(t, rng, 20) + [9])                       # the last label matches nothing
    labs.append(_walk(t, rng, 5))                              # every label matches, no final state at the end
    labs.append(_walk(t, rng, 200, prefix=(1, 1, 4)))
    labs += [[int(x) for x in rng.integers(1, SIGMA + 1, n)] for n in (7, 90, 200)]  # random strings: most die early
    assert len(labs) == 16
    return [synth.linear_acceptor_flat(np.array(l, dtype=np.uint32), final_weight=0.25 * (k % 3)) for k, l in enumerate(labs)]


@pytest.fixture(scope="module")
def string_case(oracle):
    t = _string_t()
    accs = _string_batch(t)
    ot = to_oracle(oracle, t)
    want, want_arcs = [], []
    for a in accs:
        oc = to_oracle(oracle, a).compose(ot, connect=False)
        assert oc.num_states < 512  # (the slice of a packed wave: no problem leaves the string kernel)
        want_arcs.append(oc.num_arcs)
        want.append(oc.shortest_path_canonical().to_flat())
    n_paths = sum(w["n_states"] > 0 for w in want)
    assert 9 <= n_paths <= 14, n_paths  # the walks have a path; the dead ends, the unmatched label and position 5 have none
    assert want[9]["n_states"] == 0 and want[10]["n_states"] == 0 and want[11]["n_states"] == 0
    assert want[7]["n_states"] == 31 and want[12]["n_states"] == 201
    return t, accs, want, want_arcs


def _run_batch(ctx, accs, t, want, want_arcs, n_string, what):
    outs, n_arcs = rustfst_amd.compose_shortest_path_batch(rustfst_amd.DeviceFst.upload_many(accs, ctx), to_device(t, ctx), ctx=ctx)
    assert ctx.stats()["string_problems"] == n_string, what
    flats = [o.to_flat() for o in outs]
    for k, (got, exp) in enumerate(zip(flats, want)):
        assert_flat_identical(got, exp, f"{what}: string {k}")
    assert n_arcs == sum(want_arcs), what
    return flats


def test_string_batch_of_16_on_the_packed_vector_path(gpu_ctx, string_case, monkeypatch):
    """16 strings (the smallest batch on the packed vector path) of 1, 2, 63, 64, 65, 129 and 200 labels, among them single-match
    levels in front of a 70-arc block, a dead end, an unmatched last label and a string that reaches no final state: the
    oracle's paths from the string kernel, from the general kernel (WFST_STRING_KERNEL=0), with WFST_BATCH_COPY=1 (the
    copy-command path) and with per-launch profiling (results in device buffers, copied back: the used part of the path buffer is
    the host's own sum)."""
    t, accs, want, want_arcs = string_case
    ctx = rustfst_amd.Context(0)
    got = _run_batch(ctx, accs, t, want, want_arcs, 16, "string kernel")
    again = _run_batch(ctx, accs, t, want, want_arcs, 16, "string kernel, second batch")
    monkeypatch.setenv("WFST_STRING_KERNEL", "0")
    general = _run_batch(ctx, accs, t, want, want_arcs, 0, "general kernel")
    monkeypatch.delenv("WFST_STRING_KERNEL")
    for k in range(16):
        assert_flat_identical(got[k], general[k], f"string vs general kernel, string {k}")
        assert_flat_identical(got[k], again[k], f"two batches, string {k}")
    monkeypatch.setenv("WFST_BATCH_COPY", "1")
    _run_batch(ctx, accs, t, want, want_arcs, 16, "WFST_BATCH_COPY=1")
    monkeypatch.delenv("WFST_BATCH_COPY")
    ctx.set_profiling(1)
    _run_batch(ctx, accs, t, want, want_arcs, 16, "profiling: device buffers and copies")
    ctx.set_profiling(0)
    _run_batch(ctx, accs, t, want, want_arcs, 16, "string kernel, after the other paths")


def test_string_batch_of_8_on_the_scalar_path(gpu_ctx, string_case):
    """Eight strings over the same T take the scalar-row path (n <= 8), which early issue leaves alone."""
    t, accs, want, want_arcs = string_case
    pick = [0, 2, 4, 6, 7, 9, 11, 12]
    ctx = rustfst_amd.Context(0)
    _run_batch(ctx, [accs[k] for k in pick], t, [want[k] for k in pick], [want_arcs[k] for k in pick], 8, "batch of 8")


def test_path_slices_of_17_strings_with_and_without_a_path(gpu_ctx, string_case, oracle):
    """17 strings of 17 different lengths; the even ones walk through T to a position with final states (a path), the odd ones
    end in a label T does not have (none): slices of the path buffer that overlapped or were shifted by a problem without a
    path would show as wrong arcs."""
    t = string_case[0]
    rng = np.random.default_rng(5)
    ends = [1, 2, 63, 64, 65, 129, 30, 1 + N_POS, 2 + N_POS]  # lengths that end on the positions with final states
    labs = []
    for k in range(17):
        labs.append(_walk(t, rng, ends[k // 2]) if k % 2 == 0 else _walk(t, rng, 3 + 11 * k) + [9])
    assert len({len(l) for l in labs}) == 17
    accs = [synth.linear_acceptor_flat(np.array(l, dtype=np.uint32), final_weight=0.5 * (k % 2)) for k, l in enumerate(labs)]
    ot = to_oracle(oracle, t)
    comps = [to_oracle(oracle, a).compose(ot, connect=False) for a in accs]
    want = [c.shortest_path_canonical().to_flat() for c in comps]
    assert [w["n_states"] > 0 for w in want] == [k % 2 == 0 for k in range(17)]
    ctx = rustfst_amd.Context(0)
    _run_batch(ctx, accs, t, want, [c.num_arcs for c in comps], 17, "17 strings")


# ---------------------------------------------------------------------------------------------------------------- the tail

_TAIL_T = {}


def _tail_t(n):
    """Cyclic T with a little more than 2^18 arcs (the transpose, and with it the one-launch tail, from the second query on),
    weights on the 1/4 grid so that totals tie."""
    if n not in _TAIL_T:
        t = synth.make_transducer(n, (1 << 18) // n + 1, 64, 0.0, seed=31)
        t["arcs"]["weight"] = (np.round(t["arcs"]["weight"] * 2.0) / 4.0 + 0.25).astype(np.float32)
        assert t["arcs"].shape[0] >= 1 << 18
        _TAIL_T[n] = t
    return _TAIL_T[n]


def _final_set(n, kind, rng):
    fin = np.full(n, np.inf, dtype=np.float32)
    if kind == "none":
        return fin
    if kind == "start":
        fin[0] = 0.5
        return fin
    k = {"one": 1, "1025": 1025, "4097": 4097, "n/8+1": n // 8 + 1}[kind]
    idx = rng.choice(np.arange(1, n), size=k, replace=False)
    fin[idx] = (rng.integers(0, 8, k) / 4.0).astype(np.float32)
    return fin


def _force_tied_final_states(t, oracle):
    """The first and the last final state (the two ends of the handle's list: different workgroups of a tail over more than
    4096 entries) attain the same total from state 0, below every other final state's: the tie flag has to cross workgroups."""
    dist = to_oracle(oracle, t).shortest_path_canonical().distance
    fin = t["finals"]
    idx = np.flatnonzero(np.isfinite(fin))
    a, b = int(idx[0]), int(idx[-1])
    c = np.float32(max(dist[a], dist[b]))
    fin[idx] += np.float32(100.0)
    fin[a], fin[b] = c - dist[a], c - dist[b]


# (n, final set, does the handle get a list: at most 65 536 final states and at most one state in eight)
TAIL_CASES = [(5000, "none", True), (5000, "start", True), (5000, "one", True), (5000, "1025", False), (5000, "4097", False),
              (5000, "n/8+1", False),
              # the same sizes where the rule admits them: one workgroup up to 4096 entries, two for 4097, the scan beyond n / 8
              (40_000, "1025", True), (40_000, "4097", True), (40_000, "n/8+1", False)]


@pytest.mark.parametrize("n,kind,listed", TAIL_CASES, ids=[f"{n}-{k}" for n, k, _ in TAIL_CASES])
def test_tail_over_the_list_of_final_states(oracle, monkeypatch, n, kind, listed):
    """The one-launch tail over the handle's list of final states and over all of `finals` (WFST_SSSP_FINAL_LIST=0): the same
    path, the same count of tied choices, both the canonical oracle's — from the third query on (transpose cached, the solve
    predicted: the fused tail), then again from another start state on the same handle.  WFST_SSSP_FINAL_LIST=2 (the list or an
    error) tells which handles have a list."""
    t = dict(_tail_t(n))
    t["finals"] = _final_set(n, kind, np.random.default_rng(n + len(kind)))
    if n == 40_000:
        _force_tied_final_states(t, oracle)
    ctx = rustfst_amd.Context(0)
    d = to_device(t, ctx)
    tied = 0
    for start in (0, n // 3):
        if start:
            d.set_start(start)
        can = to_oracle(oracle, dict(t, start=start)).shortest_path_canonical()
        want = can.to_flat()
        if kind == "none":
            assert want["n_states"] == 0
        elif kind == "start" and start == 0:
            assert want["n_states"] == 1  # the start state is the best final state: no arcs
        else:
            assert want["n_states"] > 1
        for q in range(3):
            assert_flat_identical(d.shortest_path().to_flat(), want, f"warm-up {q} from {start}")
        res = {}
        for mode in (None, "0", None, "2"):
            if mode is None:
                monkeypatch.delenv("WFST_SSSP_FINAL_LIST", raising=False)
            else:
                monkeypatch.setenv("WFST_SSSP_FINAL_LIST", mode)
            if mode == "2" and not listed:
                with pytest.raises(rustfst_amd.WfstError, match="no list of final states"):
                    d.shortest_path()
                continue
            got = d.shortest_path().to_flat()
            ties = ctx.stats()["tied_choices"]
            assert ties != rustfst_amd._lib.TIES_UNKNOWN  # (counted by the one-launch tail only)
            assert_flat_identical(got, want, f"FINAL_LIST={mode} from {start}")
            assert ties == can.n_tied_choices, (mode, start, ties, can.n_tied_choices)
            res[mode] = (got, ties)
        assert_flat_identical(res[None][0], res["0"][0], f"list vs scan from {start}")
        assert res[None][1] == res["0"][1]
        tied += can.n_tied_choices
        monkeypatch.delenv("WFST_SSSP_FINAL_LIST", raising=False)
    if kind in ("1025", "4097", "n/8+1"):
        assert tied > 0  # (weights on the 1/4 grid: the tie flag of the merge is exercised)


def test_knobs_are_read_at_the_start_of_every_solve(oracle, monkeypatch):
    """The environment is looked at once per solve — not once per variable, and not once per process: WFST_SSSP_MAILBOX=0 set
    between two solves of one handle selects the atomic sweeps, and the default comes back when the variable is removed."""
    monkeypatch.delenv("WFST_SSSP_MAILBOX", raising=False)
    t = synth.make_transducer(70_000, 8, 64, 0.0, seed=9)  # (from 65 536 states on the mailbox sweeps are the default)
    want = to_oracle(oracle, t).shortest_path_canonical().to_flat()
    ctx = rustfst_amd.Context(0)
    d = to_device(t, ctx)
    assert_flat_identical(d.shortest_path().to_flat(), want, "default")
    k_default = ctx.stats()["relax_kernel"]
    assert k_default in (1, 2)  # a mailbox kernel
    monkeypatch.setenv("WFST_SSSP_MAILBOX", "0")
    assert_flat_identical(d.shortest_path().to_flat(), want, "WFST_SSSP_MAILBOX=0")
    assert ctx.stats()["relax_kernel"] == 0
    monkeypatch.delenv("WFST_SSSP_MAILBOX")
    assert_flat_identical(d.shortest_path().to_flat(), want, "default again")
    assert ctx.stats()["relax_kernel"] == k_default
