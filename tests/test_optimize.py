"""tr_sum, tr_unique and optimize (wfst_tr_sum, wfst_tr_unique, wfst_optimize): the C-ABI surface without a GPU, a literal
sequential Python restatement of rustfst's tr_sum.rs, tr_unique.rs, encode/decode (EncodeLabels), rm_final_epsilon.rs and
optimize.rs (tropical semiring; oracle/model/optimize.py) checked against the hand-derived K17 known answers, and on the device
bit-exact parity with the restatement: states, offsets, arcs (weights by bit pattern), finals and property word.

The restatement reuses determinize_ref, minimize_ref, the weight and property rules, tr_unique and rm_final_epsilon of
oracle/model/ and the oracle's rm_epsilon.

Shapes of the arc-list tests, and why: the kernel keeps a state in one register per lane up to 16 arcs, works in chunks of
16 up to 256 arcs and hands larger states to a radix sort, so the degrees are 0, 1, 16, 17, 256, 257 and 300; duplicate
runs straddle a 16-arc chunk boundary (the write pass counts survivors per chunk) and cover a whole state."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import model
from oracle.model import (ACCEPTOR, ACYCLIC, EPSILONS, F32, INF, I_DETERMINISTIC, NOT_I_DETERMINISTIC, NO_EPSILONS,
                          Unsupported, apply_op, branch_of, content_word_of_flat, decode_labels, det_min,
                          determinize_encoded, determinize_ref, encode_labels, minimize_ref, norm, optimize_ref,
                          rows_flat, tr_key, tr_sum)
from helpers import assert_flat_identical, golden_flat, ko_message, to_device, to_oracle
from optimize_cases import golden_cases, optimize_input, part_a_rows, part_b_rows, random_arc_lists

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATHS = ("narrow", "wide", "auto")


# ---------------------------------------------------------------- inputs
def regime_cases(seed=21):
    """(name, flat, branch of step 4 it must take)"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(4):
        n = int(rng.integers(150, 400))
        out.append((f"acceptor-{i}", optimize_input(rng, n, False), "det-min"))
        out.append((f"transducer-{i}", optimize_input(rng, n, True), "encode"))
        out.append((f"deterministic-{i}", optimize_input(rng, n, False, deterministic=True), "min"))
    out.append(("acceptor-no-eps", optimize_input(rng, 200, False, eps=False), "det-min"))
    out.append(("transducer-no-eps", optimize_input(rng, 200, True, eps=False), "encode"))
    return out


# ================================================================ CPU
def test_symbols_declared_and_bound(wfst_lib):
    from rustfst_amd import _lib
    with open(os.path.join(ROOT, "include", "wfst.h")) as f:
        header = f.read()
    for name in ("wfst_tr_sum", "wfst_tr_unique", "wfst_optimize"):
        assert re.search(r"\bwfst_status\s+" + name + r"\s*\(wfst_ctx\* ctx, const wfst_fst\* fst, wfst_fst\*\* out\)", header)
        assert name in {n for n, _, _ in _lib.SYMBOLS}
        assert hasattr(wfst_lib, name)


def test_argument_validation_without_gpu(wfst_lib):
    for name in ("wfst_tr_sum", "wfst_tr_unique", "wfst_optimize"):
        fn = getattr(wfst_lib, name)
        out = C.c_void_p(1)
        assert "null" in ko_message(fn(None, None, C.byref(out)))
        assert out.value is None
        assert "null" in ko_message(fn(None, None, None))


def test_python_surface():
    import rustfst_amd
    for name in ("optimize", "tr_sum", "tr_unique"):
        assert name in rustfst_amd.__all__ and callable(getattr(rustfst_amd, name))
        assert callable(getattr(rustfst_amd.DeviceFst, name)) and callable(getattr(rustfst_amd.VectorFst, name))


def golden_error(c, oracle):
    try:
        apply_op(c["op"], golden_flat(c), oracle)
    except (Unsupported, ValueError) as e:
        return e.args[0]
    return None


def test_k17_restatement_reproduces_the_derivations(oracle):
    """the hand derivations of K17_DERIVATION.md, replayed by this file's restatement (checks the restatement itself)"""
    cases = golden_cases()
    names = {c["name"] for c in cases}
    assert len(cases) >= 11 and "reference_python_test" in names
    for c in cases:
        if "error" in c:
            msg = golden_error(c, oracle)
            assert msg is not None and (msg in c["error"] or c["error"] in msg), (c["name"], msg)
            continue
        got = apply_op(c["op"], golden_flat(c), oracle)
        assert_flat_identical(got, golden_flat(c, "expected"), c["name"])
        for stage, word in c.get("words", {}).items():  # the property word after every stage of the derivation
            assert stage_words(golden_flat(c), oracle)[stage] == int(word, 16), (c["name"], stage)


def stage_words(flat, oracle):
    """the words the derivations record for an optimize case: after rm_epsilon, tr_sum, encode, determinize, minimize"""
    out = {}
    cur = norm(flat)
    if not cur["props"] & NO_EPSILONS:
        cur = norm(to_oracle(oracle, cur).rm_epsilon().to_flat())
    out["rm_epsilon"] = cur["props"]
    fst = model.flat_to_fst(cur)
    tr_sum(fst)
    out["tr_sum"] = fst["props"]
    encoded = not flat["props"] & ACCEPTOR
    if encoded:
        encode_labels(fst)
        out["encode"] = fst["props"]
    cur = model.fst_to_flat(fst)
    if not cur["props"] & I_DETERMINISTIC:
        cur = norm(determinize_encoded(cur) if encoded else determinize_ref(cur))
        out["determinize"] = cur["props"]
    out["minimize"] = minimize_ref(cur)["props"]
    return out


def test_reference_python_test_machine(oracle):
    """rustfst-python/tests/algorithms/test_optimize.py: the one transducer result on record that rustfst itself produced
    (through its gallic determinizer)"""
    c = next(c for c in golden_cases() if c["name"] == "reference_python_test")
    got = optimize_ref(golden_flat(c), oracle)
    assert got["n_states"] == 4 and got["start"] == 0
    arcs = [(int(a["ilabel"]), int(a["olabel"]), float(a["weight"]), int(a["nextstate"])) for a in got["arcs"]]
    assert arcs == [(1, 2, 4.0, 1), (1, 3, 7.0, 2), (4, 6, 1.0, 3), (7, 8, 0.0, 3)]
    assert got["offsets"].tolist() == [0, 2, 3, 4, 4]
    assert [None if not np.isfinite(f) else float(f) for f in got["finals"]] == [None, 0.0, None, 0.0]


def test_transducer_branch_equals_the_acceptor_steps_on_pair_ids(oracle):
    """a random acyclic acceptor over pair ids whose rows are sorted and whose ids appear in first-occurrence order, and the
    transducer whose pairs decode them (a monotone map, so tr_sum leaves both in the same order and encode gives the ids
    back): optimize(transducer) = decode(determinize + minimize of the acceptor)"""
    rng = np.random.default_rng(9)

    def pair(i):
        return ((i - 1) // 3 + 1, (i - 1) % 3 + 5)
    for case in range(20):
        n, next_id, rows, finals = int(rng.integers(5, 60)), 1, [], []
        for s in range(n):
            row = []
            if s + 1 < n:
                old = sorted(rng.choice(np.arange(1, next_id), size=min(next_id - 1, int(rng.integers(0, 3))), replace=False)) \
                    if next_id > 1 else []
                new = list(range(next_id, next_id + int(rng.integers(0, 3))))
                next_id += len(new)
                for i in list(old) + new:
                    for t in sorted(set(int(x) for x in rng.integers(s + 1, min(n, s + 4), size=int(rng.integers(1, 3))))):
                        row.append((int(i), int(i), float(rng.integers(0, 3)), t))
            rows.append(row)
            finals.append(float(rng.integers(0, 2)) if rng.random() < 0.3 or s == n - 1 else INF)
        acc = rows_flat(rows, finals)
        acc["props"] = content_word_of_flat(acc)
        tra = rows_flat([[pair(il) + (w, t) for il, _, w, t in r] for r in rows], finals)
        tra["props"] = content_word_of_flat(tra)
        assert not tra["props"] & ACCEPTOR and tra["props"] & ACYCLIC and tra["props"] & NO_EPSILONS
        assert branch_of(tra, oracle) == "encode" and branch_of(acc, oracle) == "det-min"
        got = optimize_ref(tra, oracle)
        fst = model.flat_to_fst(norm(acc))
        tr_sum(fst)
        assert model.fst_to_flat(fst)["arcs"].tolist() == norm(acc)["arcs"].tolist()
        mini = model.flat_to_fst(det_min(model.fst_to_flat(fst), False))
        decode_labels(mini, [pair(i) for i in range(1, next_id)])
        assert_flat_identical(got, model.fst_to_flat(mini), f"case {case}", check_props=False)


def test_tr_sum_is_idempotent_and_keeps_duplicate_free_rows():
    for flat in (part_a_rows(), part_b_rows(), random_arc_lists(2, 300)):
        once = apply_op("tr_sum", flat)
        assert_flat_identical(apply_op("tr_sum", once), once, "tr_sum twice")
        off = once["offsets"]
        for s in range(once["n_states"]):
            keys = [tr_key(t) for t in once["arcs"][off[s]:off[s + 1]].tolist()]
            assert keys == sorted(set(keys)), s
    rng = np.random.default_rng(4)
    rows = [[(int(il), 1, float(rng.integers(0, 9)), int(rng.integers(0, 30))) for il in rng.permutation(40)[:int(rng.integers(0, 30))]]
            for _ in range(30)]
    flat = rows_flat(rows, [INF] * 30)
    got = apply_op("tr_sum", flat)
    assert np.array_equal(got["offsets"], flat["offsets"])
    for s, row in enumerate(rows):  # no duplicate keys: the same arcs, sorted
        seg = got["arcs"][got["offsets"][s]:got["offsets"][s + 1]]
        assert [tuple(t) for t in seg.tolist()] == sorted((il, ol, float(F32(w)), ns) for il, ol, w, ns in row)


def test_kdelta_chain_compares_with_the_last_kept_arc():
    flat = rows_flat([[(1, 1, 0.0, 0), (1, 1, 0.0009, 0), (1, 1, 0.0018, 0)]], [0.0])
    assert [float(w) for w in apply_op("tr_unique", flat)["arcs"]["weight"]] == [0.0, float(F32(0.0018))]
    assert [float(w) for w in apply_op("tr_sum", flat)["arcs"]["weight"]] == [0.0]


def test_generator_reaches_every_branch(oracle):
    """the inputs of the device parity tests, on the CPU: none lands in a KO branch, each takes the branch it is meant for"""
    seen = set()
    for name, flat, want in regime_cases():
        assert branch_of(flat, oracle) == want, name
        exp = optimize_ref(flat, oracle)
        assert exp["n_states"] > 0, name
        seen.add(want)
        if want != "min":
            assert flat["props"] & NOT_I_DETERMINISTIC, name
    assert seen == {"det-min", "encode", "min"}
    with_eps = [f for _, f, _ in regime_cases() if f["props"] & EPSILONS]
    assert len(with_eps) >= 8


# ================================================================ GPU
def dev_op(op, flat, ctx):
    return getattr(to_device(flat, ctx), op)()


def check_op(op, flat, ctx, what, oracle=None):
    dev = to_device(flat, ctx)
    before = dev.to_flat()
    got = getattr(dev, op)().to_flat()
    assert_flat_identical(got, apply_op(op, flat, oracle), f"{op} {what}")
    assert_flat_identical(dev.to_flat(), before, f"{op} {what}: the input handle")


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["tr_sum", "tr_unique"])
def test_arc_lists_part_a(gpu_ctx, op):
    check_op(op, part_a_rows(), gpu_ctx, "degrees 0, 1, 16, 17, 256, 257, 300")


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["tr_sum", "tr_unique"])
def test_arc_lists_part_b(gpu_ctx, op):
    check_op(op, part_b_rows(), gpu_ctx, "edge keys and weights")
    check_op(op, random_arc_lists(3, 3000), gpu_ctx, "3000 random states")
    check_op(op, rows_flat([], [], start=None), gpu_ctx, "no states")
    check_op(op, rows_flat([[], []], [INF, 0.0]), gpu_ctx, "no arcs")


@pytest.mark.gpu
def test_k17_on_the_device(gpu_ctx, oracle):
    import rustfst_amd
    for c in golden_cases():
        flat = golden_flat(c)
        if "error" in c:
            with pytest.raises(rustfst_amd.WfstError, match=re.escape(c["error"])):
                dev_op(c["op"], flat, gpu_ctx)
            continue
        assert_flat_identical(dev_op(c["op"], flat, gpu_ctx).to_flat(), golden_flat(c, "expected"), c["name"])


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
def test_optimize_matches_the_restatement_in_every_regime(gpu_ctx, oracle, monkeypatch, path):
    monkeypatch.setenv("WFST_DETERMINIZE_PATH", path)
    monkeypatch.setenv("WFST_MINIMIZE_PATH", path)
    for name, flat, _ in regime_cases():
        check_op("optimize", flat, gpu_ctx, f"{name} [{path}]", oracle)


@pytest.mark.gpu
def test_ko_messages_and_the_context_afterwards(gpu_ctx, oracle):
    import rustfst_amd
    good = next(c for c in golden_cases() if c["name"] == "reference_python_test")
    for c in golden_cases():
        if "error" not in c:
            continue
        dev = to_device(golden_flat(c), gpu_ctx)
        before = dev.to_flat()
        with pytest.raises(rustfst_amd.WfstError, match=re.escape(c["error"])):
            dev.optimize()
        assert_flat_identical(dev.to_flat(), before, c["name"] + ": the input handle")
        got = dev_op("optimize", golden_flat(good), gpu_ctx).to_flat()  # the context still works
        assert_flat_identical(got, golden_flat(good, "expected"), "after " + c["name"])


@pytest.mark.gpu
def test_vector_fst_surface_on_the_device(gpu_ctx):
    import rustfst_amd
    fst = rustfst_amd.VectorFst()
    s = [fst.add_state() for _ in range(4)]
    fst.set_start(s[0])
    fst.set_final(s[3], 0.0)
    for src, tr in ((0, (1, 2, 1.0, 1)), (0, (1, 3, 2.0, 2)), (1, (0, 0, 3.0, 3)), (1, (4, 6, 4.0, 3)), (2, (7, 8, 5.0, 3))):
        fst.add_tr(s[src], rustfst_amd.Tr(*tr))
    assert rustfst_amd.optimize(fst) is fst
    assert fst.num_states() == 4
    got = [(t.ilabel, t.olabel, float(t.weight), t.next_state) for st in range(4) for t in fst.trs(st)]
    assert got == [(1, 2, 4.0, 1), (1, 3, 7.0, 2), (4, 6, 1.0, 3), (7, 8, 0.0, 3)]
    assert [fst.final_weight(q) for q in range(4)] == [None, 0.0, None, 0.0]
