"""isomorphic on the device (isomorphic.hip through wfst_isomorphic) against the sequential restatement tests/isomorphic_ref.py:
the verdict or the error's message character for character, under WFST_ISOMORPHIC_PATH=auto, narrow and wide, with the
counters of wfst_ctx_get_isomorphic_counters read after every call.  K22, the seeded parity families, the limits of the
kernel file (sort routes, wave walk, the two narrow limits, regime changes), the edge verdicts and the errors."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import rustfst_amd
from rustfst_amd import WfstError, _lib

from oracle.model import F32, KDELTA

import helpers
from helpers import dev
import isomorphic_cases as K
import isomorphic_ref as R

pytestmark = pytest.mark.gpu
ROUTE_FREE = ("levels", "pairs", "events", "max_level_width")


def run_device(ctx, f1, f2, delta=None):
    """(1, 0 or the KO message, counters)"""
    try:
        got = 1 if dev(f1, ctx).isomorphic(dev(f2, ctx), delta) else 0
    except WfstError as e:
        got = str(e).split(": ", 1)[1]
    return got, ctx.isomorphic_stats()


def check_case(ctx, f1, f2, what, delta=None):
    """the device against the restatement: verdict, message and the counters that do not depend on the route"""
    info = {}
    exp = R.verdict(f1, f2, KDELTA if delta is None else F32(delta), info)
    got, st = run_device(ctx, f1, f2, delta)
    assert got == exp, (what, got, exp)
    assert {k: st[k] for k in ROUTE_FREE} == {k: info.get(k, 0) for k in ROUTE_FREE}, (what, st, info)
    if exp == 1:
        assert st["nondet_marks"] == info.get("nondet_marks", 0), (what, st, info)
    return got, st


def shuffled(fst, rng):
    """the same FST, the arcs of every state in another stored order: isomorphic whatever it holds"""
    out = dict(fst, rows=[[list(a) for a in row] for row in fst["rows"]])
    for row in out["rows"]:
        rng.shuffle(row)
    return out


# ---------------------------------------------------------------- known answers
@pytest.mark.parametrize("path", K.PATHS)
def test_k22(gpu_ctx, monkeypatch, path):
    monkeypatch.setenv("WFST_ISOMORPHIC_PATH", path)
    for name, f1, f2, delta, expected in K.k22_cases():
        got, st = check_case(gpu_ctx, f1, f2, "%s path=%s" % (name, path), delta)
        assert got == expected, (name, path, got)
        if path == "wide":
            assert st["narrow_launches"] == 0 and st["wide_launches"] == 4 * st["levels"], (name, st)
        else:
            assert st["wide_launches"] == 0 and st["narrow_launches"] == 1 and st["narrow_levels"] == st["levels"], (name, st)


def test_cpp_isomorphic_tests_run(gpu_ctx, tmp_path):
    """examples/isomorphic_tests.cpp: the reference's tests of isomorphic and invert against include/wfst.hpp, end to end"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = tmp_path / "isomorphic_tests"
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(helpers.ROOT, "include"),
                    os.path.join(helpers.ROOT, "examples", "isomorphic_tests.cpp"), "-L", libdir, "-lwfst_amd",
                    f"-Wl,-rpath,{libdir}", "-Wl,--allow-shlib-undefined", "-o", str(exe)], check=True)
    env = dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all isomorphic tests passed" in r.stdout, r.stdout + r.stderr


# ---------------------------------------------------------------- random parity
@pytest.mark.parametrize("path", K.PATHS)
@pytest.mark.parametrize("name", sorted(K.FAMILIES))
def test_family(gpu_ctx, monkeypatch, name, path):
    """every case against the restatement, never against a verdict assumed in advance (tests/test_isomorphic.py shows that
    the restatement gives each verdict in at least a tenth of the cases)"""
    monkeypatch.setenv("WFST_ISOMORPHIC_PATH", path)
    seen = set()
    for what, f1, f2 in K.family(name):
        got, _ = check_case(gpu_ctx, f1, f2, "%s path=%s" % (what, path))
        seen.add(got if got in (0, 1) else "KO")
    assert seen == {0, 1, "KO"}


# ---------------------------------------------------------------- the limits
@pytest.mark.parametrize("path", K.PATHS)
@pytest.mark.parametrize("deg", [16, 17, 63, 64, 256, 257, 1000])
def test_sort_routes_and_wave_walk(gpu_ctx, monkeypatch, deg, path):
    """a hub of `deg` arcs over nine label pairs and a coarse weight grid (negative weights at 1000): 16 / 17 the rank sort's
    one-register form and its chunks, 256 / 257 the last rank-sorted state and the first of the radix route, 63 / 64 the
    last pair a lane walks and the first its wave walks.  Against itself with every row in another stored order the answer
    is 1 whatever the hub holds — unless the two sorted copies differ; against a renumbered copy, the restatement's."""
    monkeypatch.setenv("WFST_ISOMORPHIC_PATH", path)
    rng = np.random.default_rng(2200 + deg)
    h = K.hub(deg, rng, negative=deg == 1000)
    got, st = check_case(gpu_ctx, h, shuffled(h, rng), "hub %d shuffled" % deg)
    assert got == 1
    assert st["big_states_sorted"] == (2 if deg > K.RANK_MAX else 0), st
    assert st["wave_pairs"] == (1 if deg >= K.WAVE_ARCS else 0), st
    assert st["nondet_marks"] > 0 or deg < 256, st
    _, st = check_case(gpu_ctx, h, K.permuted(h, rng), "hub %d permuted" % deg)
    assert st["big_states_sorted"] == (2 if deg > K.RANK_MAX else 0)
    # one arc's weight moved beyond delta in the middle of the sorted row: the wave (or the lane) stops there
    m = shuffled(h, rng)
    m["rows"][0][deg // 2][2] = F32(m["rows"][0][deg // 2][2] + F32(100.0))
    check_case(gpu_ctx, h, m, "hub %d one weight" % deg)


@pytest.mark.parametrize("width", [K.NARROW_PAIRS, K.NARROW_PAIRS + 1])
def test_pair_limit(gpu_ctx, monkeypatch, width):
    """level 2 of exactly the narrow pair limit stays in the one launch; one pair more takes one WIDE level between two
    narrow launches; pinned narrow, the same level runs from the call's global scratch"""
    f = K.fan(width, 1)
    rng = np.random.default_rng(width)
    for path in K.PATHS:
        monkeypatch.setenv("WFST_ISOMORPHIC_PATH", path)
        got, st = check_case(gpu_ctx, f, K.permuted(f, rng), "fan %d path=%s" % (width, path))
        assert got == 1 and (st["levels"], st["max_level_width"], st["pairs"]) == (3, width, width + 2)
        if path == "auto" and width <= K.NARROW_PAIRS:
            assert (st["narrow_launches"], st["wide_launches"], st["narrow_levels"]) == (1, 0, 3), st
        elif path == "auto":
            assert (st["narrow_launches"], st["wide_launches"], st["narrow_levels"]) == (2, 4, 2), st
        elif path == "narrow":
            assert (st["narrow_launches"], st["wide_launches"], st["narrow_levels"]) == (1, 0, 3), st
        else:
            assert (st["narrow_launches"], st["wide_launches"], st["narrow_levels"]) == (0, 12, 0), st


@pytest.mark.parametrize("events", [K.NARROW_EVENTS, K.NARROW_EVENTS + 1])
def test_event_limit(gpu_ctx, monkeypatch, events):
    """a start state of exactly the narrow event limit in arcs stays in the one launch; one arc more makes level 1 WIDE"""
    rng = np.random.default_rng(events)
    h = K.hub(events, rng, n_targets=5)
    for path in K.PATHS:
        monkeypatch.setenv("WFST_ISOMORPHIC_PATH", path)
        got, st = check_case(gpu_ctx, h, shuffled(h, rng), "hub %d path=%s" % (events, path))
        assert got == 1 and (st["levels"], st["events"], st["wave_pairs"], st["big_states_sorted"]) == (2, events, 1, 2), st
        if path == "auto" and events <= K.NARROW_EVENTS:
            assert (st["narrow_launches"], st["wide_launches"], st["narrow_levels"]) == (1, 0, 2), st
        elif path == "auto":
            assert (st["narrow_launches"], st["wide_launches"], st["narrow_levels"]) == (1, 4, 1), st


def test_diamond_goes_narrow_wide_narrow(gpu_ctx, monkeypatch):
    monkeypatch.setenv("WFST_ISOMORPHIC_PATH", "auto")
    f = K.diamond(600)
    rng = np.random.default_rng(600)
    got, st = check_case(gpu_ctx, f, K.permuted(f, rng), "diamond")
    assert got == 1 and st["max_level_width"] == 600 and st["levels"] == 8
    assert (st["narrow_launches"], st["wide_launches"], st["narrow_levels"]) == (2, 4, 7), st
    # a final weight changed behind the wide level: found by the second narrow launch
    m = K.permuted(f, rng)
    last = [s for s, w in enumerate(m["finals"]) if w is not None][0]
    m["finals"][last] = F32(5.0)
    got, st = check_case(gpu_ctx, f, m, "diamond, last level")
    assert got == 0 and (st["levels"], st["narrow_launches"], st["wide_launches"]) == (8, 2, 4)


def test_chain_runs_in_one_launch(gpu_ctx, monkeypatch):
    """5 000 levels of one pair: the narrow kernel leaves its loop only for a level beyond its limits or the end of the
    search, and a chain has neither before its last state — ONE launch whatever the length"""
    monkeypatch.setenv("WFST_ISOMORPHIC_PATH", "auto")
    f = K.chain(5000)
    rng = np.random.default_rng(5000)
    got, st = check_case(gpu_ctx, f, K.permuted(f, rng), "chain")
    assert got == 1 and (st["levels"], st["narrow_launches"], st["wide_launches"], st["narrow_levels"]) == (5000, 1, 0, 5000), st
    assert (st["pairs"], st["events"], st["max_level_width"]) == (5000, 4999, 1)


@pytest.mark.parametrize("path", K.PATHS)
def test_failure_in_the_first_and_in_the_last_level(gpu_ctx, monkeypatch, path):
    monkeypatch.setenv("WFST_ISOMORPHIC_PATH", path)
    f = K.chain(40)
    last = dict(f, finals=f["finals"][:-1] + [None])
    got, st = check_case(gpu_ctx, f, last, "last level")
    assert got == 0 and st["levels"] == 40
    first = dict(f, finals=[F32(1.0)] + f["finals"][1:])
    got, st = check_case(gpu_ctx, f, first, "first level")
    assert got == 0 and (st["levels"], st["pairs"], st["events"]) == (1, 1, 1)


# ---------------------------------------------------------------- edge verdicts and errors
def test_start_states_decide_before_any_search(gpu_ctx, monkeypatch):
    monkeypatch.setenv("WFST_ISOMORPHIC_PATH", "auto")
    f = K.chain(5)
    none_a, none_b = dict(f, start=None), dict(K.chain(9), start=None)
    zeros = dict.fromkeys(_lib.ISOMORPHIC_COUNTERS, 0)
    for a, b, exp in ((none_a, none_b, 1), (none_a, f, 0), (f, none_b, 0)):
        got, st = check_case(gpu_ctx, a, b, "start states")
        assert got == exp and st == zeros
    empty = helpers.to_device(helpers.empty_flat(), gpu_ctx)
    assert empty.isomorphic(helpers.to_device(helpers.empty_flat(), gpu_ctx)) is True
    assert empty.isomorphic(dev(f, gpu_ctx)) is False and dev(f, gpu_ctx).isomorphic(empty) is False
    assert empty.isomorphic(dev(none_a, gpu_ctx)) is True


def still_works(ctx):
    name, f1, f2, delta, expected = [c for c in K.k22_cases() if c[0] == "b_mark_below_failure"][0]
    assert isinstance(expected, str)
    got, _ = run_device(ctx, f1, f2, delta)
    assert got == expected
    assert run_device(ctx, f1, f1)[0] == 1


def test_errors_leave_the_context_working(gpu_ctx, monkeypatch):
    f = K.chain(5)
    a = dev(f, gpu_ctx)
    other = rustfst_amd.Context(0)
    b = dev(f, other)
    with pytest.raises(WfstError, match="isomorphic: fst2 belongs to another context"):
        a.isomorphic(b)
    still_works(gpu_ctx)
    res = C.c_int(7)
    assert helpers.ko_message(_lib.lib().wfst_isomorphic(gpu_ctx._h, b._h, a._h, None, C.byref(res))) == \
        "isomorphic: fst1 belongs to another context"
    assert helpers.ko_message(_lib.lib().wfst_isomorphic(gpu_ctx._h, a._h, None, None, C.byref(res))) == "null pointer"
    still_works(gpu_ctx)
    monkeypatch.setenv("WFST_ISOMORPHIC_PATH", "fast")
    with pytest.raises(WfstError, match="WFST_ISOMORPHIC_PATH: expected auto, narrow or wide, not 'fast'"):
        a.isomorphic(a)
    monkeypatch.setenv("WFST_ISOMORPHIC_PATH", "auto")
    still_works(gpu_ctx)
    assert b.isomorphic(dev(f, other)) is True  # the other context too


def test_module_functions_and_vector_fst(gpu_ctx):
    from rustfst_amd import Tr, VectorFst
    fst1 = VectorFst()
    s1, s2 = fst1.add_state(), fst1.add_state()
    fst1.set_start(s1)
    fst1.set_final(s2)
    fst1.add_tr(s1, Tr(12, 25, None, s2))
    fst2 = fst1.copy()
    assert fst1.isomorphic(fst2) and rustfst_amd.isomorphic(fst1, fst2)
    fst2.add_tr(s1, Tr(1, 2, None, s2))
    assert not fst1.isomorphic(fst2)
    d1, d2 = fst1.to_device(gpu_ctx), fst2.to_device(gpu_ctx)
    assert rustfst_amd.isomorphic(d1, d1) and not rustfst_amd.isomorphic(d1, d2) and d1.isomorphic(d2, delta=0.5) is False
