"""Where the waves of the string kernels sit (rustfst_amd/csrc/string_placement.h): one rule, from (strings, states per LDS
slice, compute units of the context, "a resident relaxation grid is at work on this device", WFST_STRING_WPB) to waves per
workgroup.  The rule moves nothing but the waves: every path, the composed states and arcs and every other route counter of a
call are the same under every placement, and Context.string_placement() says which one a launch took.

Host: tests/placement_check.cpp restates the rule as its issue words it and sweeps the header's function over the edges of
every line (built under the address and undefined-behaviour sanitizers, like slab_check).  The GPU tests ask the same program
what the header gives for the launch they made, so the counters are compared with the header, not with a third restatement."""
import functools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from rustfst_amd._lib import STRING_PLACEMENT
from rustfst_amd import synth

import helpers
from helpers import analyse_string, assert_flat_identical, finals_of, fst, string, to_device
from string_cases import string_slice

ROOT = helpers.ROOT
KNOBS = ("WFST_STRING_WPB", "WFST_STRING_UNPACKED", "WFST_STRING_SCALAR", "WFST_STRING_KERNEL", "WFST_STRING_RUN",
         "WFST_STRING_PAIR", "WFST_SSSP_BOUNDED")
ZERO = dict.fromkeys(STRING_PLACEMENT, 0)


# ================================================================ the header's function, through its check program
@functools.lru_cache(maxsize=None)
def check_program():
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    import tempfile
    exe = os.path.join(tempfile.mkdtemp(prefix="placement_check_"), "placement_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "rustfst_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "placement_check.cpp")])
    return exe


@functools.lru_cache(maxsize=None)
def header_says(n, maxs, n_cus, hint, forced_text):
    """string_placement(n, maxs, n_cus, hint, string_forced_wpb(forced_text)) of the header, as string_placement() reports it"""
    out = subprocess.run([check_program(), str(n), str(maxs), str(n_cus), str(int(hint)), forced_text or ""], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    wpb, groups, packed, forced = (int(v) for v in out.stdout.split())
    return dict(waves_per_workgroup=wpb, slice_states=maxs, workgroups=groups, packed_for_resident=packed, forced=forced)


def test_placement_rule(tmp_path):
    """string_placement.h alone in a stand-alone program: n = 1, 15, 16, 17, n_cus, n_cus + 1, 2, 4 and 8 times n_cus (+ 1), 4096
    and 2^20; n_cus 1, 4, 256, 304; slices 512 / 1024 / 2048; the hint on and off; WFST_STRING_WPB 0, 1, 2, 3, 4, 8, 9 (and what
    is no number); always wpb * 16 * maxs <= 64 KB and ceil(n / wpb) * wpb >= n"""
    out = subprocess.run([check_program()], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 mismatches" in out.stdout
    assert header_says(64, 512, 256, False, None)["waves_per_workgroup"] == 1   # the bench batch: a compute unit per string
    assert header_says(64, 512, 256, True, None)["waves_per_workgroup"] == 8    # ... beside a resident grid: 8 compute units
    assert header_says(512, 512, 256, False, None)["waves_per_workgroup"] == 2


# ================================================================ inputs
N_T = 20


@functools.lru_cache(maxsize=None)
def t20():
    """20 states (a level never has more: no string is handed back for its width), every arc with its own output label, so a
    path names its arcs.  Labels 1 and 2 have one arc in every state; label 3 has two, to two states but in state 14 (both
    to 15); label 4 keeps a state.  A label read from the wrong place of the string changes the path."""
    rows = []
    for s in range(N_T):
        rows.append([(1, 100 + 10 * s + 1, ((s + 1) % 4) / 4.0, (3 * s + 1) % N_T), (2, 100 + 10 * s + 2, ((s + 2) % 4) / 4.0, (3 * s + 2) % N_T),
                     (3, 100 + 10 * s + 3, ((s + 3) % 8) / 8.0, (s + 1) % N_T), (3, 100 + 10 * s + 4, (s % 8) / 8.0, (2 * s + 7) % N_T),
                     (4, 100 + 10 * s + 5, 0.125, s)])
    return fst(rows, finals_of(N_T, {s: s / 512.0 for s in range(N_T)}))


LENGTHS = (1, 2, 3, 62, 63, 64, 65, 66, 126, 127, 128, 129, 130)


@functools.lru_cache(maxsize=None)
def strings33():
    """33 strings of 1 to 130 labels, around the 64-label chunks; mostly labels 1, 2 and 4, with a label 3 (a level of two
    matches) in each.  The last string of a batch of 17 or 33 is a last workgroup's lone wave under every packing."""
    rng = np.random.default_rng(1633)
    out = []
    for k in range(33):
        n = LENGTHS[k % len(LENGTHS)] if k < 26 else int(rng.integers(1, 131))
        labels = rng.choice([1, 2, 4], n)
        labels[int(rng.integers(0, n))] = 3  # (one: labels 1, 2 and 4 permute the states, so every 3 doubles the levels behind it)
        out.append(string(labels, 0.25 * (k % 2)))
    assert {len(s["arcs"]) for s in out} >= set(LENGTHS)
    return out


@functools.lru_cache(maxsize=None)
def no_start():
    return dict(string([1, 2, 3]), start=-1)


def clear(monkeypatch):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)


def n_cus_of_device():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


T_SOLVE = (70_000, 8, 64)  # tests/test_bounded_head.py, tests/test_rearm.py: the smallest shape that takes a resident launch


@functools.lru_cache(maxsize=None)
def solve_input():
    return synth.make_transducer(*T_SOLVE, 0.0, seed=9)


def solve(monkeypatch, full):
    """One predicted shortest-path query on a context of its own: `full` relaxes every level in a resident launch
    (WFST_SSSP_BOUNDED=0), otherwise the bounded head ends it.  Leaves the device's record accordingly."""
    import rustfst_amd
    ctx = rustfst_amd.Context(0)
    d = to_device(solve_input(), ctx)
    if full:
        monkeypatch.setenv("WFST_SSSP_BOUNDED", "0")
    else:
        monkeypatch.delenv("WFST_SSSP_BOUNDED", raising=False)
    for _ in range(2):  # the transpose and the list exist and the solve is predicted from the second query on
        d.shortest_path()
    before = ctx.bounded_stats()
    d.shortest_path()
    after, st = ctx.bounded_stats(), ctx.stats()
    monkeypatch.delenv("WFST_SSSP_BOUNDED", raising=False)
    if full:
        assert after["stops"] == before["stops"] and st["relax_kernel"] == 2 and st["sweeps"] > 1 and st["resident_aborts"] == 0, (after, st)
    else:
        assert after["stops"] == before["stops"] + 1 and st["sweeps"] == 1, (after, st)


@pytest.fixture()
def no_resident_grid(wfst_lib, monkeypatch):
    """the device's record says "no resident grid at work", whatever ran in this process before"""
    clear(monkeypatch)
    solve(monkeypatch, full=False)


def batch(ctx, handles, dt, ans, what):
    """one fused call; every path and the arc count against the oracle; -> the counters that no placement may change"""
    import rustfst_amd
    outs, n_arcs = rustfst_amd.compose_shortest_path_batch(handles, dt, ctx=ctx)
    for k, a in enumerate(ans):
        assert_flat_identical(outs[k].to_flat(), a["path"], "%s, string %d" % (what, k), check_props=True)
    assert n_arcs == sum(a["n_arcs"] for a in ans), what
    assert int(ctx.stats()["compose_states"]) == sum(a["n_states"] for a in ans), what
    return dict(path=ctx.compose_path_stats(), run=ctx.string_run_stats(), pair=ctx.string_pair_counts())


# ================================================================ GPU: the same answers wherever the waves sit
@pytest.mark.gpu
@pytest.mark.parametrize("scalar", ["0", "1"])
@pytest.mark.parametrize("n", [16, 17, 33])
def test_every_placement_answers_alike(gpu_ctx, oracle, monkeypatch, no_resident_grid, n, scalar):
    """batches of 16, 17 and 33 strings (17 and 33: a last workgroup of one wave under every packing) under the default
    placement and under WFST_STRING_WPB = 1, 2, 4, 8, scalar rows off and on: paths, composed states and arcs as the oracle has
    them, compose_path_stats, string_run_stats and string_pair_counts equal across the placements, string_placement() as the
    header has it.  An acceptor without a start state rides in the calls of 17 and 33: it is no string (fst_store.hip:
    detect_string wants start state 0), so it is the general kernel's in the same call and the string launch keeps its size."""
    import rustfst_amd
    strs, t = strings33()[:n], t20()
    extra = [no_start()] if n > 16 else []
    dt, handles = to_device(t, gpu_ctx), rustfst_amd.DeviceFst.upload_many(strs + extra, gpu_ctx)
    ans = [analyse_string(oracle, s, t) for s in strs + extra]
    maxs = string_slice(n, max(s["n_states"] for s in strs))
    assert maxs == 512 and all(a["n_states"] <= maxs for a in ans)  # every string is the kernel's
    assert not extra or (ans[-1]["n_states"] == 0 and ans[-1]["path"]["n_states"] == 0)
    cus = n_cus_of_device()
    monkeypatch.setenv("WFST_STRING_SCALAR", scalar)
    first = None
    for forced in (None, "1", "2", "4", "8"):
        if forced is None:
            monkeypatch.delenv("WFST_STRING_WPB", raising=False)
        else:
            monkeypatch.setenv("WFST_STRING_WPB", forced)
        what = "n %d, scalar %s, WFST_STRING_WPB=%s" % (n, scalar, forced)
        got = batch(gpu_ctx, handles, dt, ans, what)
        assert got["path"]["string_answered"] == n and got["path"]["string_handed_back"] == 0, (what, got)
        if scalar == "0":
            assert got["run"]["run_levels"] > 0 and got["pair"]["pair_levels"] > 0, (what, got)
        first = first or got
        assert got == first, (what, got, first)
        place = gpu_ctx.string_placement()
        assert place == header_says(n, maxs, cus, False, forced), (what, place)
        assert place["waves_per_workgroup"] == (int(forced) if forced else 1) and place["forced"] == (forced is not None)
        assert place["workgroups"] == -(-n // place["waves_per_workgroup"])
    clear(monkeypatch)


@pytest.mark.gpu
def test_knob_values_and_small_batches(gpu_ctx, oracle, monkeypatch, no_resident_grid):
    """WFST_STRING_WPB=3 is 2, 9 is 8, 0 and a word are not there; WFST_STRING_UNPACKED is one wave and the 2048-state slice
    whatever WFST_STRING_WPB says; 15 strings are one wave each; a call without a string launch reports zeros"""
    import rustfst_amd
    strs, t = strings33()[:16], t20()
    dt, handles = to_device(t, gpu_ctx), rustfst_amd.DeviceFst.upload_many(strs, gpu_ctx)
    ans = [analyse_string(oracle, s, t) for s in strs]
    cus = n_cus_of_device()
    first = None
    for text, wpb in (("3", 2), ("9", 8), ("0", 1), ("many", 1), ("", 1)):
        monkeypatch.setenv("WFST_STRING_WPB", text)
        got = batch(gpu_ctx, handles, dt, ans, "WFST_STRING_WPB=%r" % text)
        first = first or got
        place = gpu_ctx.string_placement()
        assert got == first and place == header_says(16, 512, cus, False, text) and place["waves_per_workgroup"] == wpb, (text, place)
        assert place["forced"] == (text in ("3", "9"))
    monkeypatch.setenv("WFST_STRING_WPB", "8")
    monkeypatch.setenv("WFST_STRING_UNPACKED", "1")
    assert batch(gpu_ctx, handles, dt, ans, "unpacked")["path"] == first["path"]
    assert gpu_ctx.string_placement() == dict(waves_per_workgroup=1, slice_states=2048, workgroups=16, packed_for_resident=0, forced=1)
    clear(monkeypatch)
    batch(gpu_ctx, handles[:15], dt, ans[:15], "15 strings")
    assert gpu_ctx.string_placement() == dict(waves_per_workgroup=1, slice_states=2048, workgroups=15, packed_for_resident=0, forced=0)
    assert gpu_ctx.string_placement() == header_says(15, 2048, cus, False, None)
    monkeypatch.setenv("WFST_STRING_KERNEL", "0")
    batch(gpu_ctx, handles[:3], dt, ans[:3], "general kernel")
    assert gpu_ctx.string_placement() == ZERO
    clear(monkeypatch)


# ================================================================ GPU: the slice pin under spreading
def ladder_t(w):
    """label 1 leads from the start state to w states that loop on it: every level of 1^L has w states.  Label 2 loops too,
    and adds ONE state from g0: a string that ends in 2 has one state more in all, and w + 1 in its last level."""
    g = lambda j: 1 + j
    rows = [[(1, 100 + j, (j % 4) / 4.0, g(j)) for j in range(w)]]
    for j in range(w):
        rows.append([(1, 100 + j, 0.25, g(j)), (2, 200 + j, 0.0, g(j))] + ([(2, 300, 0.25, g(w))] if j == 0 else []))
    rows.append([(1, 400, 0.25, g(w))])
    return fst(rows, finals_of(w + 2, {g(j): ((j * 3) % 5) / 4.0 for j in range(w + 1)}))


@functools.lru_cache(maxsize=None)
def slice_batch(beyond):
    """a batch of 16: one string of 73 labels that sets the 512-state slice (2 * 74 + 64 = 212) and composes with ladder_t(7)
    to exactly 1 + 73 * 7 = 512 states (beyond: 513), and 15 short ones"""
    w, L = 7, 73
    return [string([1] * (L - 1) + [2 if beyond else 1])] + [string([1] * (1 + k % 3)) for k in range(15)], ladder_t(w)


@pytest.mark.gpu
@pytest.mark.parametrize("forced", [None, "1", "8"])
@pytest.mark.parametrize("beyond", [False, True], ids=["fits", "one_more"])
def test_slice_of_a_batch_wherever_it_sits(gpu_ctx, oracle, monkeypatch, no_resident_grid, beyond, forced):
    """a batch of 16 whose longest string picks the 512-state slice: exactly 512 composed states are answered and 513 are
    handed back, at the default placement and with one wave per workgroup as with eight"""
    import rustfst_amd
    accs, t = slice_batch(beyond)
    dt, handles = to_device(t, gpu_ctx), rustfst_amd.DeviceFst.upload_many(accs, gpu_ctx)
    ans = [analyse_string(oracle, a, t) for a in accs]
    assert ans[0]["n_states"] == 512 + beyond and string_slice(16, accs[0]["n_states"]) == 512
    if forced is not None:
        monkeypatch.setenv("WFST_STRING_WPB", forced)
    got = batch(gpu_ctx, handles, dt, ans, "slice 512%s, WFST_STRING_WPB=%s" % ("+1" if beyond else "", forced))
    assert (got["path"]["string_answered"], got["path"]["string_handed_back"]) == (16 - beyond, int(beyond)), got
    place = gpu_ctx.string_placement()
    assert place == header_says(16, 512, n_cus_of_device(), False, forced) and place["slice_states"] == 512, place
    assert place["waves_per_workgroup"] == (8 if forced == "8" else 1)
    clear(monkeypatch)


@pytest.mark.gpu
def test_forced_eight_with_the_largest_slice_is_two(gpu_ctx, oracle, monkeypatch, no_resident_grid):
    """a string of 1000 labels picks the 2048-state slice (2 * 1001 + 64 > 1024): 64 KB of LDS hold two of them"""
    import rustfst_amd
    accs, t = [string([1] * 1000)] + [string([1] * (1 + k % 3)) for k in range(15)], ladder_t(1)
    dt, handles = to_device(t, gpu_ctx), rustfst_amd.DeviceFst.upload_many(accs, gpu_ctx)
    ans = [analyse_string(oracle, a, t) for a in accs]
    monkeypatch.setenv("WFST_STRING_WPB", "8")
    got = batch(gpu_ctx, handles, dt, ans, "2048-state slice, WFST_STRING_WPB=8")
    assert got["path"]["string_answered"] == 16
    assert gpu_ctx.string_placement() == dict(waves_per_workgroup=2, slice_states=2048, workgroups=8, packed_for_resident=0, forced=1)
    clear(monkeypatch)


# ================================================================ GPU: the compute units of a masked context
@pytest.mark.gpu
def test_four_compute_units_take_four_waves_each(wfst_lib, oracle, monkeypatch, no_resident_grid):
    """a context whose stream may use 4 compute units: 16 strings are 4 workgroups of 4 waves, and answer as anywhere"""
    import rustfst_amd
    words = [0] * ((n_cus_of_device() + 31) // 32)
    words[0] = 0xF
    ctx = rustfst_amd.Context(0, cu_mask=words)
    strs, t = strings33()[:16], t20()
    dt, handles = to_device(t, ctx), rustfst_amd.DeviceFst.upload_many(strs, ctx)
    ans = [analyse_string(oracle, s, t) for s in strs]
    got = batch(ctx, handles, dt, ans, "4-CU mask")
    assert got["path"]["string_answered"] == 16
    assert ctx.string_placement() == dict(waves_per_workgroup=4, slice_states=512, workgroups=4, packed_for_resident=0, forced=0)
    assert ctx.string_placement() == header_says(16, 512, 4, False, None)
    ctx.synchronize()


# ================================================================ GPU: the hint
@pytest.mark.gpu
def test_a_resident_solve_packs_the_next_batch_and_a_stopped_one_spreads_it(gpu_ctx, oracle, monkeypatch):
    """after a solve that ran its levels in a resident launch (WFST_SSSP_BOUNDED=0) a batch of 16 packs eight waves to a
    workgroup and says why; after a solve that stops in its head it spreads again.  WFST_STRING_WPB overrides the record."""
    import rustfst_amd
    clear(monkeypatch)
    strs, t = strings33()[:16], t20()
    dt, handles = to_device(t, gpu_ctx), rustfst_amd.DeviceFst.upload_many(strs, gpu_ctx)
    ans = [analyse_string(oracle, s, t) for s in strs]
    cus = n_cus_of_device()
    solve(monkeypatch, full=True)
    packed = batch(gpu_ctx, handles, dt, ans, "after a resident solve")
    assert gpu_ctx.string_placement() == dict(waves_per_workgroup=8, slice_states=512, workgroups=2, packed_for_resident=1, forced=0)
    assert gpu_ctx.string_placement() == header_says(16, 512, cus, True, None)
    monkeypatch.setenv("WFST_STRING_WPB", "2")
    assert batch(gpu_ctx, handles, dt, ans, "forced beside the record") == packed
    assert gpu_ctx.string_placement() == header_says(16, 512, cus, True, "2")
    assert gpu_ctx.string_placement()["packed_for_resident"] == 0
    monkeypatch.delenv("WFST_STRING_WPB")
    solve(monkeypatch, full=False)
    assert batch(gpu_ctx, handles, dt, ans, "after a stop in the head") == packed
    assert gpu_ctx.string_placement() == dict(waves_per_workgroup=1, slice_states=512, workgroups=16, packed_for_resident=0, forced=0)
    clear(monkeypatch)


FRESH_PROCESS = """
import sys
sys.path.insert(0, %r)
import rustfst_amd
from rustfst_amd import synth
ctx = rustfst_amd.Context(0)
assert not any(ctx.string_placement().values()), ctx.string_placement()
t = synth.make_transducer(20, 4, 8, 0.0, seed=5)
strs = synth.make_acceptors(t, 16, 30, seed0=1)
dt = rustfst_amd.DeviceFst.from_arrays(t["n_states"], t["start"], t["offsets"], t["arcs"], t["finals"], t["props"], ctx)
outs, _ = rustfst_amd.compose_shortest_path_batch(rustfst_amd.DeviceFst.upload_many(strs, ctx), dt, ctx=ctx)
assert ctx.compose_path_stats()["string_answered"] + ctx.compose_path_stats()["string_handed_back"] == 16
print("placement", ctx.string_placement())
"""


@pytest.mark.gpu
def test_a_process_that_never_solved_spreads(wfst_lib):
    """a fresh context in a fresh process: nothing has been solved on the device, the record reads "no resident grid", a batch
    of 16 is sixteen workgroups of one wave.  (A process of its own: the record is the process's, and this one has solved.)"""
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    out = subprocess.run([sys.executable, "-c", FRESH_PROCESS % ROOT], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    want = dict(waves_per_workgroup=1, slice_states=512, workgroups=16, packed_for_resident=0, forced=0)
    assert "placement %r" % (want,) in out.stdout, out.stdout + out.stderr


# ================================================================ the getter's plumbing
def test_getter_plumbing(wfst_lib):
    import ctypes as C
    import rustfst_amd
    name = "wfst_ctx_get_string_placement"
    helpers.check_counter_getter(wfst_lib, name, STRING_PLACEMENT, rustfst_amd.Context.string_placement)
    v = C.c_uint64(5)
    assert wfst_lib.wfst_ctx_get_string_placement(None, None, None, None, None, C.byref(v)) != 0 and v.value == 5


@pytest.mark.gpu
def test_getter_pointer_by_pointer(wfst_lib, gpu_ctx, monkeypatch):
    """any out-pointer may be NULL, and each one alone receives the counter of its position"""
    import ctypes as C
    import rustfst_amd
    clear(monkeypatch)
    monkeypatch.setenv("WFST_STRING_WPB", "4")
    strs = strings33()[:17]
    rustfst_amd.compose_shortest_path_batch(rustfst_amd.DeviceFst.upload_many(strs, gpu_ctx), to_device(t20(), gpu_ctx), ctx=gpu_ctx)
    clear(monkeypatch)
    full = gpu_ctx.string_placement()
    assert full == dict(waves_per_workgroup=4, slice_states=512, workgroups=5, packed_for_resident=0, forced=1)
    fn, n, sentinel = wfst_lib.wfst_ctx_get_string_placement, len(STRING_PLACEMENT), 0xA5A5A5A5A5A5A5A5
    assert fn(gpu_ctx._h, *[None] * n) == 0
    for i, key in enumerate(STRING_PLACEMENT):
        vals = [C.c_uint64(sentinel) for _ in range(n)]
        assert fn(gpu_ctx._h, *[C.byref(v) if k == i else None for k, v in enumerate(vals)]) == 0
        assert [v.value for v in vals] == [full[key] if k == i else sentinel for k in range(n)], key


# ================================================================ GPU: the sigma kernel's launch
@pytest.mark.gpu
def test_sigma_batch_wherever_its_waves_sit(gpu_ctx, oracle, monkeypatch, no_resident_grid):
    """string_sigma_sp_kernel takes its placement from the same function: a seeded batch of 17 utterances against a sigma
    grammar (tests/sigma_batch_cases.py; a last workgroup of one wave under every packing) at the default placement, under
    WFST_STRING_WPB = 1, 2, 4, 8, with WFST_STRING_UNPACKED, and after a resident solve: the oracle's paths every time, composed
    arcs and sigma_batch_stats equal across the placements, string_placement() as the header has it and zeroed by a call that
    launches nothing"""
    import rustfst_amd
    from rustfst_amd import ComposeConfig, ComposeFilter, MatcherConfig, MatcherRewriteMode
    from oracle.model import fst_to_flat
    import sigma_batch_cases as B
    import sigma_ref as R
    name, strs, t, m2 = next(c for c in B.seeded_cases() if len(c[1]) == 17)
    want = [B.expected_path(oracle, R.compose_sigma(a, t, R.SEQUENCE, True, None, m2)) for a in strs]
    cfg = ComposeConfig(ComposeFilter(R.SEQUENCE), True, None, MatcherConfig(m2[0], MatcherRewriteMode(m2[1]), m2[2]))
    handles, dt = [to_device(fst_to_flat(a), gpu_ctx) for a in strs], to_device(fst_to_flat(t), gpu_ctx)
    cus = n_cus_of_device()

    def call(what):
        outs, n_arcs = rustfst_amd.compose_shortest_path_batch(handles, dt, cfg, ctx=gpu_ctx)
        for i, o in enumerate(outs):
            assert_flat_identical(o.to_flat(), want[i], "%s: %s item %d" % (name, what, i))
        return n_arcs, gpu_ctx.sigma_batch_stats()

    first = call("default")
    k = first[1]["items_in_kernel"] + first[1]["items_handed_back"]
    assert first[1]["launches"] == 1 and k == 17, first
    assert gpu_ctx.string_placement() == header_says(k, 512, cus, False, None)
    assert gpu_ctx.string_placement() == dict(waves_per_workgroup=1, slice_states=512, workgroups=17, packed_for_resident=0, forced=0)
    for forced in ("1", "2", "4", "8"):
        monkeypatch.setenv("WFST_STRING_WPB", forced)
        assert call("WFST_STRING_WPB=" + forced) == first
        place = gpu_ctx.string_placement()
        assert place == header_says(k, 512, cus, False, forced) and place["workgroups"] == -(-k // int(forced)), place
    monkeypatch.setenv("WFST_STRING_UNPACKED", "1")
    assert call("unpacked") == first
    assert gpu_ctx.string_placement() == dict(waves_per_workgroup=1, slice_states=2048, workgroups=17, packed_for_resident=0, forced=1)
    clear(monkeypatch)
    solve(monkeypatch, full=True)
    assert call("after a resident solve") == first
    assert gpu_ctx.string_placement() == header_says(k, 512, cus, True, None)
    assert gpu_ctx.string_placement() == dict(waves_per_workgroup=8, slice_states=512, workgroups=3, packed_for_resident=1, forced=0)
    # a call with a matcher on side 1 never reaches the kernel: it zeroes the counters and leaves them so
    side1 = ComposeConfig(ComposeFilter(R.SEQUENCE), True, MatcherConfig(m2[0], MatcherRewriteMode(m2[1]), m2[2]), None)
    try:
        rustfst_amd.compose_shortest_path_batch(handles[:1], dt, side1, ctx=gpu_ctx)
    except rustfst_amd.WfstError:
        pass
    assert gpu_ctx.sigma_batch_stats()["launches"] == 0 and gpu_ctx.string_placement() == ZERO
    solve(monkeypatch, full=False)
    clear(monkeypatch)
