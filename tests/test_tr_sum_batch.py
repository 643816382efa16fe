"""wfst_tr_sum_batch / wfst_tr_unique_batch: the C-ABI and Python surface without a GPU, a host predictor of the in_kernel
flag with one input on each side of every limit of the rule; and on the device parity of every batch item with
test_optimize's restatement AND with the single call on the same handle, bit for bit including the property word, the
flags against the predictor, the launch counters, untouched inputs and the KO of a foreign handle.

Shapes, and why: the kernel keeps a state in one register per lane up to 16 arcs and works in chunks of 16 up to 256 arcs
(degrees 0, 1, 16, 17, 256; 257 leaves the kernel); the workgroup scan gives every thread one count up to 256 states and a
chunk of several beyond (257 and 4096 states); 300 items are more workgroups than one wave of blocks holds."""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest

from oracle.model import INF, apply_op, rows_flat
import helpers
from helpers import assert_flat_identical, to_device
from optimize_cases import part_a_rows, part_b_rows, random_arc_lists

ROOT = helpers.ROOT
MAX_STATES, MAX_ARCS, RANK_MAX = 4096, 16384, 256  # include/wfst.h: the in_kernel rule
OPS = ("tr_sum", "tr_unique")
BATCH_ARGS = "wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, wfst_fst** outs, uint8_t* in_kernel"
SIGNATURES = {
    "wfst_tr_sum_batch": BATCH_ARGS,
    "wfst_tr_unique_batch": BATCH_ARGS,
    "wfst_ctx_get_tr_sum_batch_stats": "wfst_ctx* ctx, uint64_t* launches, uint64_t* items_in_kernel, uint64_t* items_single",
}


def predict_in_kernel(flat):
    """wfst.h: an item without states or with at most one arc counts as in the kernel; otherwise at most 4096 states, at
    most 16384 arcs and no state with more than 256 arcs"""
    n, e = flat["n_states"], len(flat["arcs"])
    if n == 0 or e <= 1:
        return 1
    if n > MAX_STATES or e > MAX_ARCS:
        return 0
    return int(int(np.diff(flat["offsets"].astype(np.int64)).max()) <= RANK_MAX)


def same(got, exp, what):
    assert_flat_identical(got, exp, what, check_props=True)


# ---------------------------------------------------------------- inputs
def rows_of(flat):
    off = flat["offsets"]
    return [[tuple(t) for t in flat["arcs"][off[s]:off[s + 1]].tolist()] for s in range(flat["n_states"])]


def part_a_in_kernel():
    """optimize_cases.part_a_rows with its states of more than 256 arcs cut to 256: degrees 0, 1, 16, 17, 256, the runs over a
    chunk boundary and over a whole state, all inside the kernel"""
    flat = part_a_rows()
    return rows_flat([r[:RANK_MAX] for r in rows_of(flat)], list(flat["finals"]))


def nan_rows():
    nan = float("nan")
    rows = [[(1, 1, 1.0, 0), (1, 1, nan, 0), (1, 1, 0.5, 0), (2, 2, nan, 1), (2, 2, 3.0, 1), (3, 3, 2.0, 1), (3, 3, nan, 1)],
            [(4, 4, 2.0, 0)] * 9 + [(4, 4, nan, 0)] + [(4, 4, 1.0, 0)] * 9]  # a NaN inside a run over a chunk boundary
    return rows_flat(rows, [INF, 0.0])


def short_lists(seed, n, max_deg, props=0):
    """n states of 0..max_deg arcs, half of them repeats of an earlier key of the state"""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(n):
        row = []
        for _ in range(int(rng.integers(0, max_deg + 1))):
            if row and rng.random() < 0.5:
                il, ol, _, ns = row[int(rng.integers(0, len(row)))]
            else:
                il, ol, ns = int(rng.integers(0, 4)), int(rng.integers(0, 4)), int(rng.integers(0, n))
            row.append((il, ol, float(rng.integers(0, 64)) / 1024.0 if rng.random() < 0.5 else float(rng.integers(0, 4)), ns))
        rows.append(row)
    return rows_flat(rows, [0.0 if rng.random() < 0.2 else INF for _ in range(n)], props=props)


def pairs_chain(n):
    """n states, two arcs with one key into the next state each (the last state: none)"""
    rows = [[(1 + s % 3, 1 + s % 3, float(s % 5), s + 1), (1 + s % 3, 1 + s % 3, float((s + 2) % 5), s + 1)] for s in range(n - 1)]
    return rows_flat(rows + [[]], [INF] * (n - 1) + [0.0])


def block_of_arcs(total, per_state=128):
    """`total` arcs, per_state to a state (every key twice), the remainder in one more state"""
    rows, left = [], total
    while left:
        k = min(per_state, left)
        rows.append([(1 + j // 2, 1, float(j % 7), 0) for j in range(k)])
        left -= k
    return rows_flat(rows, [0.0] + [INF] * (len(rows) - 1))


def one_wide_state(deg):
    return rows_flat([[(1 + j % 100, 2, float((j * 7) % 11), j % 3) for j in range(deg)], [(1, 1, 1.0, 0)] * 3, []], [INF, INF, 0.0])


@functools.lru_cache(maxsize=None)
def limit_families():
    """(name, flat, expected flag): one input on each side of every limit"""
    return [("states 4096", pairs_chain(MAX_STATES), 1), ("states 4097", pairs_chain(MAX_STATES + 1), 0),
            ("arcs 16384", block_of_arcs(MAX_ARCS), 1), ("arcs 16385", block_of_arcs(MAX_ARCS + 1), 0),
            ("a state of 256 arcs", one_wide_state(RANK_MAX), 1), ("a state of 257 arcs", one_wide_state(RANK_MAX + 1), 0)]


@functools.lru_cache(maxsize=None)
def parity_items():
    """[(name, flat)]: the mixed list"""
    return [("part a, degrees up to 256", part_a_in_kernel()),
            ("part a, degrees 257 and 300", part_a_rows()),
            ("part b, edge keys and weights", part_b_rows()),
            ("NaN inside a run", nan_rows()),
            ("257 states", short_lists(7, 257, 11)),
            ("4096 states", short_lists(8, 4096, 6)),
            ("no states", rows_flat([], [], start=None)),
            ("one arc", rows_flat([[(1, 2, 0.5, 1)], []], [INF, 0.0])),
            ("no arcs", rows_flat([[], []], [INF, 0.0])),
            ("no start state", dict(short_lists(9, 20, 11), start=None)),
            ("a word to mask", random_arc_lists(3, 40))]


_REF = {}


def reference(op, name, flat):
    """the restatement's answer, computed once per (op, item) and left unchanged"""
    if (op, name) not in _REF:
        _REF[op, name] = apply_op(op, flat)
    return _REF[op, name]


@functools.lru_cache(maxsize=None)
def many_small(count=300):
    return [("small %d" % k, short_lists(1000 + k, 3 + k % 18, 9)) for k in range(count)]


# ================================================================ no GPU
def test_new_symbols_declared_exported_and_bound(wfst_lib):
    from rustfst_amd import _lib
    with open(os.path.join(ROOT, "include", "wfst.h")) as f:
        header = f.read()
    vp, u64 = C.c_void_p, C.POINTER(C.c_uint64)
    batch = [vp, C.POINTER(vp), C.c_size_t, C.POINTER(vp), vp]
    args = {"wfst_tr_sum_batch": batch, "wfst_tr_unique_batch": batch, "wfst_ctx_get_tr_sum_batch_stats": [vp, u64, u64, u64]}
    bound = {name: a for name, _, a in _lib.SYMBOLS}
    version = header[header.index("#define WFST_ABI_VERSION"):header.index("6: wfst_ctx_set_resident_share")]
    for name, want in SIGNATURES.items():
        m = re.search(r"\bwfst_status\s+%s\s*\(([^)]*)\)" % name, header)
        assert m and " ".join(m.group(1).split()) == want, name
        assert bound[name] == args[name] and hasattr(wfst_lib, name), name
        assert re.search(r"\b%s\b" % name, version), name + " in the version-7 list"
    assert re.search(r"#define\s+WFST_ABI_VERSION\s+7\b", header) and wfst_lib.wfst_abi_version() == 7
    text = header[header.index("tr_sum / tr_unique of n FSTs in one call"):header.index("wfst_status wfst_tr_sum_batch")]
    assert "4096 states" in text and "16384 arcs" in text and "256 arcs" in text and "split the list" in text


@pytest.mark.parametrize("name", ["wfst_tr_sum_batch", "wfst_tr_unique_batch"])
def test_argument_validation_without_gpu(wfst_lib, name):
    ko = helpers.ko_message
    fn = getattr(wfst_lib, name)
    outs = (C.c_void_p * 3)(1, 1, 1)
    fsts = (C.c_void_p * 3)()
    assert fn(None, None, 0, None, None) == 0  # n == 0: OK
    assert "null" in ko(fn(None, fsts, 3, outs, None))  # NULL ctx
    assert [outs[i] for i in range(3)] == [None] * 3
    assert "null" in ko(fn(None, fsts, 3, None, None))  # NULL outs
    outs = (C.c_void_p * 3)(1, 1, 1)
    assert "null" in ko(fn(None, None, 3, outs, None))  # NULL fsts with n > 0
    assert [outs[i] for i in range(3)] == [None] * 3
    assert "null" in ko(wfst_lib.wfst_ctx_get_tr_sum_batch_stats(None, None, None, None))
    # a NULL entry is reported with its index before anything else is done with the context: no context can be made
    # without a device, so this one is zeroed memory, and the call may do no more with it than clear its counters
    ctx = C.create_string_buffer(1 << 20)
    outs = (C.c_void_p * 3)(1, 1, 1)
    assert ko(fn(C.cast(ctx, C.c_void_p), fsts, 3, outs, None)) == "item 0: null FST in batch"
    assert [outs[i] for i in range(3)] == [None] * 3 and ctx.raw == bytes(1 << 20)


def test_python_surface():
    import rustfst_amd
    for name in ("tr_sum_batch", "tr_unique_batch", "tr_sum_batch_stats"):
        assert name in rustfst_amd.__all__ and callable(getattr(rustfst_amd, name))
    for name in ("tr_sum_batch", "tr_unique_batch"):
        fn = getattr(rustfst_amd, name)
        p = inspect.signature(fn).parameters
        assert list(p) == ["fsts", "ctx", "return_in_kernel"]
        assert p["ctx"].default is None and p["return_in_kernel"].default is False
        assert fn([]) == []
        res, flags = fn([], return_in_kernel=True)
        assert res == [] and flags.dtype == np.uint8 and len(flags) == 0
    p = inspect.signature(rustfst_amd.tr_sum_batch_stats).parameters
    assert list(p) == ["ctx"] and p["ctx"].default is None


def test_predictor_on_both_sides_of_every_limit():
    fams = {name: (f, want) for name, f, want in limit_families()}
    assert fams["states 4096"][0]["n_states"] == MAX_STATES and fams["states 4097"][0]["n_states"] == MAX_STATES + 1
    assert len(fams["arcs 16384"][0]["arcs"]) == MAX_ARCS and len(fams["arcs 16385"][0]["arcs"]) == MAX_ARCS + 1

    def widest(f):
        return int(np.diff(f["offsets"].astype(np.int64)).max())
    assert widest(fams["a state of 256 arcs"][0]) == RANK_MAX and widest(fams["a state of 257 arcs"][0]) == RANK_MAX + 1
    for name, (f, want) in fams.items():
        assert predict_in_kernel(f) == want, name
        if not name.startswith("a state"):  # (only the size decides these four)
            assert widest(f) <= RANK_MAX and f["n_states"] <= MAX_STATES + 1 and len(f["arcs"]) <= MAX_ARCS + 1, name
    items = dict(parity_items())
    assert [predict_in_kernel(items[k]) for k in ("no states", "one arc", "no arcs")] == [1, 1, 1]
    assert predict_in_kernel(items["part a, degrees up to 256"]) == 1 and predict_in_kernel(items["part a, degrees 257 and 300"]) == 0
    assert predict_in_kernel(dict(one_wide_state(RANK_MAX + 1), start=None)) == 0  # (a start state is not part of the rule)
    degs = set(np.diff(items["part a, degrees up to 256"]["offsets"].astype(np.int64)).tolist())
    assert {0, 1, 16, 17, 256} <= degs and max(degs) == 256
    assert all(predict_in_kernel(f) for _, f in many_small())


def test_restatement_on_the_new_inputs():
    """what the device tests compare with: NaN never replaces and is never within KDELTA of anything"""
    got = apply_op("tr_sum", nan_rows())
    assert got["offsets"].tolist() == [0, 3, 4]
    w = got["arcs"]["weight"]
    assert float(w[0]) == 0.5 and np.isnan(w[1]) and float(w[2]) == 2.0 and float(w[3]) == 1.0
    got = apply_op("tr_unique", nan_rows())
    assert got["offsets"].tolist() == [0, 7, 10]


# ================================================================ GPU
def _fn(op):
    import rustfst_amd
    return getattr(rustfst_amd, op + "_batch")


def _batch(op, devs, ctx):
    outs, flags = _fn(op)(devs, ctx, return_in_kernel=True)
    return [o.to_flat() for o in outs], [int(x) for x in flags]


def _stats(ctx):
    import rustfst_amd
    return rustfst_amd.tr_sum_batch_stats(ctx)


def check_list(op, items, ctx, single=True):
    """one batch call; every result against the restatement and the single call on the same handle, the flags against the
    predictor, the counters against the flags.  Returns (results, flags, handles)."""
    devs = [to_device(f, ctx) for _, f in items]
    got, flags = _batch(op, devs, ctx)
    want = [predict_in_kernel(f) for _, f in items]
    st = _stats(ctx)
    print("flags %s\nstats %s" % (flags, st))
    assert flags == want
    assert st["items_in_kernel"] == sum(want) and st["items_single"] == len(want) - sum(want)
    for k, ((name, flat), g) in enumerate(zip(items, got)):
        same(g, reference(op, name, flat), f"{op} item {k} ({name}) vs the restatement")
        if single:
            same(g, getattr(devs[k], op)().to_flat(), f"{op} item {k} ({name}) vs the single call")
    return got, flags, devs


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS)
def test_parity_of_one_mixed_list(gpu_ctx, op):
    items = parity_items()
    got, flags, devs = check_list(op, items, gpu_ctx)
    assert _stats(gpu_ctx)["launches"] == 1 and flags.count(0) == 1
    by = dict(zip((name for name, _ in items), got))
    assert by["no states"]["n_states"] == 0 and by["no start state"]["start"] in (None, -1)
    if op == "tr_unique":  # the KDELTA chain 0, 0.0009, 0.0018, 0.0027 of part b's state 9: the first and the third stay
        b = by["part b, edge keys and weights"]
        seg = b["arcs"][b["offsets"][9]:b["offsets"][10]]
        assert [float(w) for w in seg["weight"]] == [0.0, float(np.float32(0.0018))]
    # the inputs are left as they are, by download and word
    before = [to_device(f, gpu_ctx).to_flat() for _, f in items]
    for (name, _), d, b in zip(items, devs, before):
        same(d.to_flat(), b, f"{name}: the input after the batch call")
    # the same handle twice, and an item between the two
    outs = _fn(op)([devs[0], devs[2], devs[0]], gpu_ctx)
    same(outs[0].to_flat(), got[0], "the same handle twice: first")
    same(outs[2].to_flat(), got[0], "the same handle twice: second")
    same(outs[1].to_flat(), got[2], "the same handle twice: between")
    assert _stats(gpu_ctx) == dict(launches=1, items_in_kernel=3, items_single=0)


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS)
def test_both_sides_of_every_limit(gpu_ctx, op):
    fams = limit_families()
    got, flags, _ = check_list(op, [(name, f) for name, f, _ in fams], gpu_ctx)
    assert flags == [want for _, _, want in fams]
    assert _stats(gpu_ctx) == dict(launches=1, items_in_kernel=3, items_single=3)


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS)
def test_lists_of_1_and_of_300_items(gpu_ctx, op):
    items = many_small()
    got, flags, devs = check_list(op, items, gpu_ctx, single=False)
    assert _stats(gpu_ctx) == dict(launches=1, items_in_kernel=300, items_single=0)
    for k in (0, 150, 299):
        same(got[k], getattr(devs[k], op)().to_flat(), f"{op} item {k} of 300 vs the single call")
    one, flags = _batch(op, devs[7:8], gpu_ctx)
    assert flags == [1] and _stats(gpu_ctx) == dict(launches=1, items_in_kernel=1, items_single=0)
    same(one[0], got[7], "a list of one item")
    _batch(op, devs[:3], gpu_ctx)
    assert _stats(gpu_ctx) == dict(launches=1, items_in_kernel=3, items_single=0)


@pytest.mark.gpu
def test_no_launch_when_every_item_is_trivial_or_single(gpu_ctx):
    items = dict(parity_items())
    names = ["no states", "one arc", "no arcs", "part a, degrees 257 and 300"]
    fams = {name: f for name, f, _ in limit_families()}
    listed = [(k, items[k]) for k in names] + [(k, fams[k]) for k in ("states 4097", "arcs 16385", "a state of 257 arcs")]
    # (the host's rule refuses two of the four single items; the two with a wide state need a launch to be found)
    host_only = [x for x in listed if x[0] not in ("part a, degrees 257 and 300", "a state of 257 arcs")]
    for op in OPS:
        check_list(op, host_only, gpu_ctx)
        assert _stats(gpu_ctx) == dict(launches=0, items_in_kernel=3, items_single=2)
        check_list(op, listed, gpu_ctx, single=False)
        assert _stats(gpu_ctx) == dict(launches=1, items_in_kernel=3, items_single=4)


@pytest.mark.gpu
def test_foreign_handle_is_ko_and_the_context_works_afterwards(gpu_ctx):
    import rustfst_amd
    from rustfst_amd import _lib
    items = parity_items()[2:6]
    devs = [to_device(f, gpu_ctx) for _, f in items]
    good, _ = _batch("tr_sum", devs, gpu_ctx)
    other = rustfst_amd.Context(0)
    foreign = to_device(items[1][1], other)
    hs = [d._h.value for d in devs]
    for fn_name, what in (("wfst_tr_sum_batch", "tr_sum_batch"), ("wfst_tr_unique_batch", "tr_unique_batch")):
        for handles, text in ((hs[:1] + [foreign._h.value] + hs[2:], "item 1: " + what + ": the FST belongs to another context"),
                              (hs[:3] + [None], "item 3: null FST in batch")):
            arr = (C.c_void_p * 4)(*handles)
            outs = (C.c_void_p * 4)(1, 1, 1, 1)
            status = getattr(_lib.lib(), fn_name)(gpu_ctx._h, arr, 4, outs, None)
            assert helpers.ko_message(status) == text
            assert [outs[i] for i in range(4)] == [None] * 4
            assert _stats(gpu_ctx) == dict(launches=0, items_in_kernel=0, items_single=0)
    del foreign
    for g, e in zip(_batch("tr_sum", devs, gpu_ctx)[0], good):
        same(g, e, "after the KO calls")
    assert _lib.lib().wfst_tr_sum_batch(gpu_ctx._h, None, 0, None, None) == 0
    assert _stats(gpu_ctx) == dict(launches=0, items_in_kernel=0, items_single=0)
