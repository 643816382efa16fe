"""determinize / determinize_with_config of acceptors (wfst_determinize): the C-ABI surface without a GPU, a Python
restatement of rustfst's DeterminizeFsa (oracle/model/determinize.py) checked against the K12 / K15 known answers and the oracle,
and on the device parity with the oracle in every regime, closed-form answers at scale, invariants and error handling."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

from rustfst_amd._lib import TR_DTYPE

from oracle.model import ACCEPTOR, KDELTA, determinize_props, determinize_ref
from helpers import (ROOT, assert_flat_identical, enumerate_paths, flat_of, golden, ko_message, random_fst_flat,
                     to_device, to_oracle)
from inputs import diamond_chain, twin_copy
from determinize_cases import collision_level, parity_inputs, random_acceptor

PATHS = ("narrow", "wide", "auto")


def same(got, exp, what, props=True):
    assert_flat_identical(got, exp, what, check_props=props)


# ================================================================ no GPU
def test_new_symbol_declared_and_bound(wfst_lib):
    from rustfst_amd import _lib
    with open(os.path.join(ROOT, "include", "wfst.h")) as f:
        header = f.read()
    assert re.search(r"\bwfst_status\s+wfst_determinize\s*\(", header)
    assert re.search(r"typedef struct \{\s*float delta;\s*uint32_t det_type;\s*\} wfst_determinize_config;", header)
    assert "wfst_determinize" in {name for name, _, _ in _lib.SYMBOLS}
    assert hasattr(wfst_lib, "wfst_determinize")
    assert C.sizeof(_lib.DeterminizeConfig) == 8
    assert _lib.DeterminizeConfig.delta.offset == 0 and _lib.DeterminizeConfig.det_type.offset == 4


def test_argument_validation_without_gpu(wfst_lib):
    from rustfst_amd import _lib
    out = C.c_void_p()
    assert "null" in ko_message(wfst_lib.wfst_determinize(None, None, None, C.byref(out)))
    assert "null" in ko_message(wfst_lib.wfst_determinize(None, None, None, None))
    bad = _lib.DeterminizeConfig(KDELTA, 3)
    assert "det_type" in ko_message(wfst_lib.wfst_determinize(None, None, C.byref(bad), C.byref(out)))
    for d in (0.0, -1.0, float("nan"), float("inf")):
        cfg = _lib.DeterminizeConfig(d, 0)
        assert "delta" in ko_message(wfst_lib.wfst_determinize(None, None, C.byref(cfg), C.byref(out)))
    assert out.value is None


def test_python_surface():
    import rustfst_amd
    T = rustfst_amd.DeterminizeType
    assert (T.DETERMINIZE_FUNCTIONAL.value, T.DETERMINIZE_NON_FUNCTIONAL.value, T.DETERMINIZE_DISAMBIGUATE.value) == (0, 1, 2)
    cfg = rustfst_amd.DeterminizeConfig(T.DETERMINIZE_FUNCTIONAL)
    assert cfg.delta == KDELTA and cfg.det_type is T.DETERMINIZE_FUNCTIONAL
    assert rustfst_amd.DeterminizeConfig(T.DETERMINIZE_NON_FUNCTIONAL, 0.25).delta == 0.25
    for name in ("determinize", "determinize_with_config", "DeterminizeConfig", "DeterminizeType"):
        assert name in rustfst_amd.__all__ and hasattr(rustfst_amd, name)
    assert list(inspect.signature(rustfst_amd.DeviceFst.determinize).parameters) == ["self", "config"]
    assert list(inspect.signature(rustfst_amd.VectorFst.determinize).parameters) == ["self", "config"]


def test_restatement_reproduces_k12_and_k15():
    for c in golden("k12_determinize.json"):
        got = determinize_ref(flat_of(c["fst"]))
        same(got, flat_of(c["expected"]), c["name"], props=False)
    cases = golden("k15_determinize.json")
    assert len(cases) >= 10
    for c in cases:
        same(determinize_ref(flat_of(c["fst"]), c["delta"], c["det_type"]), flat_of(c["expected"]), c["name"])
    n = {c["name"]: flat_of(c["expected"])["n_states"] for c in cases}
    assert n["non_transitive_3_4_5"] == 4 and n["non_transitive_4_3_5"] == 3


def test_restatement_matches_the_oracle(oracle):
    for name, flat, delta in parity_inputs() + [("collisions", collision_level(8, 40), KDELTA)]:
        exp = to_oracle(oracle, flat).determinize_fsa(delta).to_flat()
        same(determinize_ref(flat, delta), exp, name, props=False)
    for c in golden("k15_determinize.json"):
        flat = flat_of(c["fst"])
        same(to_oracle(oracle, flat).determinize_fsa(c["delta"]).to_flat(), flat_of(c["expected"]), c["name"], props=False)


def test_twin_copy_closed_form_matches_the_restatement():
    N, exp = twin_copy(300)
    same(determinize_ref(N), exp, "twin copy n=300")


# ================================================================ GPU
def _det(flat, ctx, delta=KDELTA, det_type=0):
    import rustfst_amd
    cfg = rustfst_amd.DeterminizeConfig(rustfst_amd.DeterminizeType(det_type), delta)
    return to_device(flat, ctx).determinize(cfg).to_flat()


@pytest.mark.gpu
def test_known_answers_on_the_device(gpu_ctx, monkeypatch):
    for path in PATHS:
        monkeypatch.setenv("WFST_DETERMINIZE_PATH", path)
        for c in golden("k12_determinize.json"):
            same(_det(flat_of(c["fst"]), gpu_ctx), flat_of(c["expected"]), f"{c['name']} {path}", props=False)
        for c in golden("k15_determinize.json"):
            same(_det(flat_of(c["fst"]), gpu_ctx, c["delta"], c["det_type"]), flat_of(c["expected"]), f"{c['name']} {path}")


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
def test_oracle_parity_in_every_regime(gpu_ctx, oracle, monkeypatch, path):
    monkeypatch.setenv("WFST_DETERMINIZE_PATH", path)
    for name, flat, delta in parity_inputs():
        exp = to_oracle(oracle, flat).determinize_fsa(delta).to_flat()
        exp["props"] = determinize_props(flat["props"], True)
        same(_det(flat, gpu_ctx, delta), exp, f"{name} {path}")


@pytest.mark.gpu
def test_level_full_of_approx_equal_collisions(gpu_ctx, oracle, monkeypatch):
    flat = collision_level()
    exp = to_oracle(oracle, flat).determinize_fsa().to_flat()
    exp["props"] = determinize_props(ACCEPTOR, True)
    assert exp["n_states"] > 4  # the non-transitive chains split {A, B} into several states
    for path in PATHS:
        monkeypatch.setenv("WFST_DETERMINIZE_PATH", path)
        same(_det(flat, gpu_ctx), exp, f"collisions {path}")


@pytest.mark.gpu
def test_twin_copy_graph_at_scale(gpu_ctx, oracle, monkeypatch):
    N, exp = twin_copy(3000)
    ref = to_oracle(oracle, N).determinize_fsa().to_flat()
    same(ref, exp, "oracle vs closed form n=3000", props=False)
    for path in ("wide", "auto"):
        monkeypatch.setenv("WFST_DETERMINIZE_PATH", path)
        same(_det(N, gpu_ctx), exp, f"twin copy n=3000 {path}")
    monkeypatch.setenv("WFST_DETERMINIZE_PATH", "auto")
    N, exp = twin_copy(250_000)
    same(_det(N, gpu_ctx), exp, "twin copy n=250000")


@pytest.mark.gpu
def test_deep_and_thin_diamond_chain(gpu_ctx, oracle, monkeypatch):
    flat = diamond_chain(20_000)
    exp = to_oracle(oracle, flat).determinize_fsa().to_flat()
    exp["props"] = determinize_props(ACCEPTOR, True)
    assert exp["n_states"] == 20_001
    monkeypatch.setenv("WFST_DETERMINIZE_PATH", "auto")
    same(_det(flat, gpu_ctx), exp, "diamond chain auto")
    small = diamond_chain(300)
    exp = to_oracle(oracle, small).determinize_fsa().to_flat()
    exp["props"] = determinize_props(ACCEPTOR, True)
    for path in ("narrow", "wide"):
        monkeypatch.setenv("WFST_DETERMINIZE_PATH", path)
        same(_det(small, gpu_ctx), exp, f"diamond chain {path}")


@pytest.mark.gpu
def test_invariants_on_small_acyclic_inputs(gpu_ctx):
    rng = np.random.default_rng(99)
    for k in range(12):
        flat = random_acceptor(rng, int(rng.integers(3, 14)), 3, 2, acyclic=True, p_eps_i=0.2)
        got = _det(flat, gpu_ctx)
        best_in, best_out = {}, {}
        for w, il, _ in enumerate_paths(flat):
            best_in[il] = min(best_in.get(il, math.inf), w)
        for w, il, _ in enumerate_paths(got):
            assert il not in best_out, f"case {k}: string {il} accepted twice"
            best_out[il] = w
        assert best_in.keys() == best_out.keys(), f"case {k}"
        for il, w in best_in.items():
            assert abs(best_out[il] - w) <= 1e-3 * max(1.0, abs(w)), f"case {k}: {il} {best_out[il]} != {w}"
        off, arcs = got["offsets"], got["arcs"]
        for s in range(got["n_states"]):
            labels = arcs["ilabel"][off[s]:off[s + 1]]
            assert len(set(labels.tolist())) == len(labels) and np.all(np.diff(labels.astype(np.int64)) > 0)


@pytest.mark.gpu
def test_errors_and_isolation(gpu_ctx, monkeypatch):
    import rustfst_amd
    rng = np.random.default_rng(5)
    t = random_fst_flat(rng, 10, 3, 4)  # a transducer (olabels differ, word without ACCEPTOR)
    with pytest.raises(rustfst_amd.WfstError, match="transducers are not supported"):
        to_device(t, gpu_ctx).determinize()
    a = random_acceptor(rng, 10, 3, 4)
    a["props"] &= ~ACCEPTOR  # an acceptor whose word does not say so: the reference takes the transducer branch
    with pytest.raises(rustfst_amd.WfstError, match="transducers are not supported"):
        to_device(a, gpu_ctx).determinize()
    # no twins property: 0 -1/1-> 0, 0 -1/2-> 1, 1 -1/0-> 1 grows one subset per level
    arcs = np.array([(1, 1, 1.0, 0), (1, 1, 2.0, 1), (1, 1, 0.0, 1)], dtype=TR_DTYPE)
    bad = dict(n_states=2, start=0, offsets=np.array([0, 2, 3], np.uint32), arcs=arcs,
               finals=np.array([np.inf, 0.0], np.float32), props=ACCEPTOR)
    monkeypatch.setenv("WFST_DETERMINIZE_MAX_STATES", "1000")
    for path in PATHS:
        monkeypatch.setenv("WFST_DETERMINIZE_PATH", path)
        with pytest.raises(rustfst_amd.WfstError, match="more than"):
            to_device(bad, gpu_ctx).determinize()
    monkeypatch.delenv("WFST_DETERMINIZE_MAX_STATES")
    monkeypatch.setenv("WFST_DETERMINIZE_PATH", "auto")
    flat = random_acceptor(rng, 30, 3, 3, acyclic=True)
    dev = to_device(flat, gpu_ctx)
    before = dev.to_flat()
    got = dev.determinize().to_flat()  # the same context still works after the KO
    same(got, determinize_ref(flat), "after the KO")
    same(dev.to_flat(), before, "source handle")
    # determinize -> shortest_path has the weight of shortest_path on the input
    w_in = enumerate_paths(dev.shortest_path().to_flat())
    w_out = enumerate_paths(dev.determinize().shortest_path().to_flat())
    assert len(w_in) == len(w_out) == 1 and abs(w_in[0][0] - w_out[0][0]) <= 1e-3
    # VectorFst: a new FST, the input left as it is
    v = rustfst_amd.VectorFst.from_flat(flat) if hasattr(rustfst_amd.VectorFst, "from_flat") else dev.to_vector_fst()
    d = rustfst_amd.determinize(v)
    assert d is not v and d.num_states() == got["n_states"]
