"""Shared test helpers: seeded random FSTs, flat <-> oracle conversion, comparison, the library's last error."""
import ctypes as C
import json
import os

import numpy as np

from rustfst_amd._lib import TR_DTYPE
from rustfst_amd import ComposeFilter, synth

from oracle.model import ACCEPTOR, B, F32, INF, csr_next, fst_to_flat, make_flat, reach, reverse_len_rule, to_oracle
from oracle.model.props import NOT_I_LABEL_SORTED, NOT_O_LABEL_SORTED

P = synth  # property bit names
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_fst_flat(rng, n_states, max_fanout, sigma, p_eps_i=0.0, p_eps_o=0.0, p_final=0.3, sort="ilabel",
                    weight_grid=512, max_w=2560, acyclic=False, min_fanout=0):
    """Small random FST as flat CSR with weights on the 1/weight_grid grid; arcs sorted by `sort`
    (ilabel|olabel|none); property word states sortedness truthfully."""
    offsets = [0]
    rows = []
    for s in range(n_states):
        k = int(rng.integers(min_fanout, max_fanout + 1))
        arcs = []
        for _ in range(k):
            il = 0 if rng.random() < p_eps_i else int(rng.integers(1, sigma + 1))
            ol = 0 if rng.random() < p_eps_o else int(rng.integers(1, sigma + 1))
            w = float(rng.integers(0, max_w)) / weight_grid
            if acyclic:
                if s + 1 >= n_states:
                    continue
                ns = int(rng.integers(s + 1, n_states))
            else:
                ns = int(rng.integers(0, n_states))
            arcs.append((il, ol, w, ns))
        if sort == "ilabel":
            arcs.sort(key=lambda a: a[0])
        elif sort == "olabel":
            arcs.sort(key=lambda a: a[1])
        rows.extend(arcs)
        offsets.append(len(rows))
    arcs = np.array(rows, dtype=TR_DTYPE) if rows else np.zeros(0, dtype=TR_DTYPE)
    finals = np.where(rng.random(n_states) < p_final, rng.integers(0, max_w, n_states) / weight_grid, np.inf).astype(
        np.float32)
    props = 0
    il_sorted = all(np.all(np.diff(arcs["ilabel"][offsets[s]:offsets[s + 1]].astype(np.int64)) >= 0)
                    for s in range(n_states))
    ol_sorted = all(np.all(np.diff(arcs["olabel"][offsets[s]:offsets[s + 1]].astype(np.int64)) >= 0)
                    for s in range(n_states))
    props |= P.I_LABEL_SORTED if il_sorted else NOT_I_LABEL_SORTED
    props |= P.O_LABEL_SORTED if ol_sorted else NOT_O_LABEL_SORTED
    return dict(n_states=n_states, start=0 if n_states else None, offsets=np.array(offsets, dtype=np.uint32), arcs=arcs,
                finals=finals, props=props)


def to_device(flat, ctx=None):
    import rustfst_amd
    return rustfst_amd.DeviceFst.from_arrays(flat["n_states"], flat["start"], flat["offsets"], flat["arcs"],
                                             flat["finals"], flat["props"], ctx)


def assert_flat_identical(a, b, what="", check_props=True):
    """Bit-exact comparison of two flat FSTs (indices AND float bit patterns)."""
    assert a["n_states"] == b["n_states"], f"{what}: num_states {a['n_states']} != {b['n_states']}"
    assert a["start"] == b["start"], f"{what}: start {a['start']} != {b['start']}"
    np.testing.assert_array_equal(a["offsets"], b["offsets"], err_msg=f"{what}: offsets")
    for k in ("ilabel", "olabel", "nextstate"):
        np.testing.assert_array_equal(a["arcs"][k], b["arcs"][k], err_msg=f"{what}: arcs.{k}")
    np.testing.assert_array_equal(a["arcs"]["weight"].view(np.uint32), b["arcs"]["weight"].view(np.uint32),
                                  err_msg=f"{what}: arc weights (bit pattern)")
    np.testing.assert_array_equal(a["finals"].view(np.uint32), b["finals"].view(np.uint32),
                                  err_msg=f"{what}: final weights (bit pattern)")
    if check_props:
        assert a["props"] == b["props"], f"{what}: props {a['props']:#x} != {b['props']:#x}"


def enumerate_paths(flat, max_paths=200_000):
    """Every complete path (start -> a final state) of an ACYCLIC flat FST by exhaustive depth-first enumeration:
    [(total weight as float64 of left-folded f32 sums, (ilabels...), (olabels...))].  Independent of the oracle and of
    the library: the brute force the n-best results are checked against."""
    if flat["start"] is None or flat["n_states"] == 0:
        return []
    off, arcs, fin = flat["offsets"], flat["arcs"], flat["finals"]
    out = []

    def rec(s, w, il, ol):
        if len(out) > max_paths:
            raise RuntimeError("too many paths for the brute force")
        if np.isfinite(fin[s]):
            out.append((float(np.float32(w) + np.float32(fin[s])), tuple(il), tuple(ol)))
        for a in arcs[off[s]:off[s + 1]]:
            rec(int(a["nextstate"]), np.float32(np.float32(w) + np.float32(a["weight"])), il + [int(a["ilabel"])], ol + [int(a["olabel"])])

    rec(int(flat["start"]), np.float32(0.0), [], [])
    return out


def check_nbest_against_brute_force(result_flat, input_flat, n, what=""):
    """`result_flat` = shortest_path(nshortest = n) of the ACYCLIC `input_flat`: it must hold exactly min(n, #paths)
    complete paths, each a real path of the input (same label strings once epsilons are removed, same weight), and their
    weights must be the n smallest path weights of the input (as a multiset: ties may pick either path)."""
    def strip(t):
        return tuple(x for x in t if x != 0)
    brute = enumerate_paths(input_flat)
    got = enumerate_paths(result_flat)
    assert len(got) == min(n, len(brute)), f"{what}: {len(got)} paths in the result, {len(brute)} in the input, n = {n}"
    want_w = sorted(w for w, _, _ in brute)[:len(got)]
    np.testing.assert_allclose(sorted(w for w, _, _ in got), want_w, rtol=0, atol=1e-4, err_msg=f"{what}: the n smallest weights")
    have = {}
    for w, il, ol in brute:
        have.setdefault((strip(il), strip(ol)), []).append(w)
    for w, il, ol in got:
        ws = have.get((strip(il), strip(ol)))
        assert ws is not None, f"{what}: the result holds a string the input does not accept: {il} / {ol}"
        assert min(abs(w - x) for x in ws) <= 1e-4, f"{what}: path {il} has weight {w}, the input gives {ws}"


def walk_labels(rng, flat, state, side, length):
    """labels (`side`: ilabel|olabel) along a random walk of at most `length` labelled steps from `state`; epsilons are
    followed without being recorded.  At least one label (1 where the walk finds none)."""
    off, arcs = flat["offsets"], flat["arcs"]
    labs, s = [], int(state)
    for _ in range(4 * length):
        if len(labs) == length or off[s] == off[s + 1]:
            break
        a = arcs[int(rng.integers(off[s], off[s + 1]))]
        if int(a[side]):
            labs.append(int(a[side]))
        s = int(a["nextstate"])
    return np.array(labs or [1], dtype=np.uint32)


def linear_transducer_flat(rng, length, sigma):
    """A chain like utils::acceptor's, but a transducer: every arc has ilabel != olabel, both non-epsilon."""
    f = synth.linear_acceptor_flat(rng.integers(1, sigma + 1, length))
    f["arcs"]["olabel"] = f["arcs"]["ilabel"] % sigma + 1
    f["arcs"]["weight"] = (rng.integers(0, 2560, length) / 512).astype(np.float32)
    f["props"] = 0
    return f


def one_sided_eps_transducer(rng, n_states, max_fanout, sigma, eps_side, p_eps=0.2, p_final=0.08, sort="ilabel"):
    """Cyclic transducer with epsilons on `eps_side` (ilabel|olabel) only; arcs in `sort` order, sortedness stated truthfully."""
    f = random_fst_flat(rng, n_states, max_fanout, sigma, p_eps_i=p_eps if eps_side == "ilabel" else 0.0,
                        p_eps_o=p_eps if eps_side == "olabel" else 0.0, p_final=p_final, sort=sort, min_fanout=1)
    assert np.any(f["arcs"][eps_side] == 0)
    return f


def ko_message(status):
    from rustfst_amd import _lib
    assert status == 1
    msg = C.c_char_p()
    assert _lib.lib().wfst_last_error(C.byref(msg)) == 0
    text = msg.value.decode()
    _lib.lib().wfst_string_destroy(msg)
    return text


def header_params(header, name):
    """the parameter list of `name` as include/wfst.h declares it, comments dropped and white space folded"""
    import re
    m = re.search(r"\bwfst_status\s+%s\s*\(([^)]*)\)" % name, header)
    assert m, name
    return " ".join(re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S).split()).replace(" ,", ",")


def null_ctx_is_ko(lib, name, n):
    """a null ctx is KO with "null", and what the first out-pointer points at is left as it was"""
    v = C.c_uint64(5)
    assert "null" in ko_message(getattr(lib, name)(None, C.byref(v), *[None] * (n - 1)))
    assert v.value == 5


def check_counter_getter(lib, name, counters, accessor):
    """The plumbing of one route-counter getter, against the test's own restatement of its counters: declared in wfst.h as
    (wfst_ctx* ctx, uint64_t* <counter>, ...) in that order, bound with those argtypes, exported, named in the version-7
    note of WFST_ABI_VERSION by a library of that version, read by a callable Python accessor, and KO on a null ctx."""
    import re
    from rustfst_amd import _lib
    with open(os.path.join(ROOT, "include", "wfst.h")) as f:
        header = f.read()
    assert header_params(header, name) == "wfst_ctx* ctx, " + ", ".join("uint64_t* " + k for k in counters)
    bound = {n: a for n, _, a in _lib.SYMBOLS}
    assert bound[name] == [C.c_void_p] + [C.POINTER(C.c_uint64)] * len(counters) and hasattr(lib, name)
    m = re.search(r"#define\s+WFST_ABI_VERSION\s+7\b(.*)", header)
    assert m and name in m.group(1).split("; 6:")[0] and lib.wfst_abi_version() == 7
    assert callable(accessor)
    null_ctx_is_ko(lib, name, len(counters))
    return header


FILTERS = [ComposeFilter.NULLFILTER, ComposeFilter.TRIVIALFILTER, ComposeFilter.SEQUENCEFILTER,
           ComposeFilter.ALTSEQUENCEFILTER, ComposeFilter.MATCHFILTER, ComposeFilter.NOMATCHFILTER]


def flat_matches_spec(flat, spec):
    assert flat["n_states"] == spec["n_states"]
    assert flat["start"] == spec.get("start")
    got = []
    for s in range(flat["n_states"]):
        for a in flat["arcs"][flat["offsets"][s]:flat["offsets"][s + 1]]:
            got.append([s, int(a["ilabel"]), int(a["olabel"]), float(a["weight"]), int(a["nextstate"])])
    exp = spec["arcs"]
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        assert g[:3] == e[:3] and g[4] == e[4], (g, e)
        assert abs(g[3] - e[3]) <= 1.0 / 1024.0, (g, e)
    fin = {s: w for s, w in spec["finals"]}
    for s in range(flat["n_states"]):
        if s in fin:
            assert abs(float(flat["finals"][s]) - fin[s]) <= 1.0 / 1024.0
        else:
            assert np.isinf(flat["finals"][s])


def _flat(n, start, rows, finals, props=None):
    """rows[s] = [(ilabel, olabel, weight, nextstate)]; the property word states label sortedness truthfully"""
    offsets = np.zeros(n + 1, dtype=np.uint32)
    offsets[1:] = np.cumsum([len(r) for r in rows])
    flat_rows = [a for r in rows for a in r]
    arcs = np.array(flat_rows, dtype=TR_DTYPE) if flat_rows else np.zeros(0, dtype=TR_DTYPE)
    if props is None:
        il = all(all(r[i][0] <= r[i + 1][0] for i in range(len(r) - 1)) for r in rows)
        ol = all(all(r[i][1] <= r[i + 1][1] for i in range(len(r) - 1)) for r in rows)
        props = (synth.I_LABEL_SORTED if il else NOT_I_LABEL_SORTED) | (synth.O_LABEL_SORTED if ol else NOT_O_LABEL_SORTED)
    return dict(n_states=n, start=start, offsets=offsets, arcs=arcs, finals=np.asarray(finals, dtype=np.float32), props=props)


def empty_flat(props=0, start=None):
    return dict(n_states=0, start=start, offsets=np.zeros(1, np.uint32), arcs=np.zeros(0, TR_DTYPE), finals=np.zeros(0, np.float32),
                props=props)


def fst(rows, finals, props=None):
    return _flat(len(rows), 0, rows, finals, props)


def finals_of(n, where):
    f = np.full(n, np.inf, dtype=np.float32)
    for s, w in where.items():
        f[s] = w
    return f


def string(labels, final_weight=0.0):
    return synth.linear_acceptor_flat(np.asarray(labels, dtype=np.uint32), final_weight)


_AN = {}


def analyse(oracle, a, b, flt=0):
    """the untrimmed composition with its BFS levels (lo, hi, arcs emitted, new states), the trimmed one, the canonical path"""
    key = (id(a), id(b), flt)
    if key not in _AN:
        oa, ob = to_oracle(oracle, a), to_oracle(oracle, b)
        c = oa.compose(ob, connect=False, compose_filter=flt)
        cf = c.to_flat()
        n, off, nx = cf["n_states"], cf["offsets"].astype(np.int64), cf["arcs"]["nextstate"].astype(np.int64)
        if len(nx):  # first-touch order: an arc names a state seen before, or the next new one
            seen = np.maximum.accumulate(np.concatenate([[0], nx]))
            assert np.all(np.diff(seen) <= 1), "the oracle's ids are not first-touch order"
        levels, lo, hi = [], 0, min(n, 1)
        while lo < hi:
            e0, e1 = int(off[lo]), int(off[hi])
            new_hi = max(hi, int(nx[e0:e1].max()) + 1 if e1 > e0 else 0)
            levels.append((lo, hi, e1 - e0, new_hi - hi))
            lo, hi = hi, new_hi
        assert hi == n
        path = c.shortest_path_canonical().to_flat()
        _AN[key] = dict(a=a, b=b, full=cf, trim=oa.compose(ob, connect=True, compose_filter=flt).to_flat(), levels=levels, path=path,
                        hops=path["n_states"] - 1 if path["n_states"] else None)
    return _AN[key]


_AN_STRING = {}


def analyse_string(oracle, a, t):
    """the oracle's untrimmed composition (states, arcs) and its canonical shortest path"""
    key = (id(a), id(t))
    if key not in _AN_STRING:
        c = to_oracle(oracle, a).compose(to_oracle(oracle, t), connect=False, compose_filter=0)
        cf = c.to_flat()
        _AN_STRING[key] = dict(a=a, t=t, n_states=cf["n_states"], n_arcs=len(cf["arcs"]), path=c.shortest_path_canonical().to_flat())
    return _AN_STRING[key]


def wstring(labels, weights=None, final_weight=0.0):
    """a string whose arcs carry weights"""
    L = len(labels)
    weights = [0.0] * L if weights is None else weights
    rows = [[(int(labels[i]), int(labels[i]), float(weights[i]), i + 1)] for i in range(L)] + [[]]
    return fst(rows, finals_of(L + 1, {L: final_weight}))


def names_to_word(names):
    return sum(1 << B[n] for n in names)


def golden_fst(m):
    return dict(rows=[[[il, ol, F32(w), ns] for il, ol, w, ns in row] for row in m["rows"]],
                finals=[None if w is None else F32(w) for w in m["finals"]], start=m["start"], props=names_to_word(m["props"]))


def make_fst(rows, finals, start, props=0):
    return dict(rows=[[[il, ol, F32(w), ns] for il, ol, w, ns in row] for row in rows],
                finals=[None if w is None else F32(w) for w in finals], start=start, props=props)


def dev(fst, ctx):
    return to_device(fst_to_flat(fst), ctx)


def _vector_fst(m):
    import rustfst_amd
    f = rustfst_amd.VectorFst()
    for _ in m["rows"]:
        f.add_state()
    if m["start"] is not None:
        f.set_start(m["start"])
    for s, w in enumerate(m["finals"]):
        if w is not None:
            f.set_final(s, float(w))
    for s, row in enumerate(m["rows"]):
        for il, ol, w, ns in row:
            f.add_tr(s, rustfst_amd.Tr(il, ol, float(w), ns))
    return f


def golden_flat(c, key="input"):
    g = c[key]
    n = g["n_states"]
    rows = [[] for _ in range(n)]
    for s, il, ol, w, ns in g["arcs"]:
        rows[s].append((il, ol, w, ns))
    finals = [INF] * n
    for s, w in g["finals"]:
        finals[s] = w
    return make_flat(n, g["start"], rows, finals, int(g["props"], 16))


GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")


def golden(name):
    with open(os.path.join(GOLDEN_DIR, name)) as f:
        return json.load(f)["cases"]


def flat_of(e, default_props=ACCEPTOR):
    """the k15 format (offsets, [il, ol, w, ns] rows, finals with null) or the k12 one (arc rows [s, il, ol, w, ns],
    finals as [s, w] pairs)"""
    n = e["n_states"]
    if "offsets" in e:
        rows, offsets = e["arcs"], e["offsets"]
        fin = [np.inf if w is None else w for w in e["finals"]]
    else:
        per = [[] for _ in range(n)]
        for s, il, ol, w, ns in e["arcs"]:
            per[s].append((il, ol, w, ns))
        rows, offsets = [r for p in per for r in p], np.cumsum([0] + [len(p) for p in per])
        fin = [np.inf] * n
        for s, w in e["finals"]:
            fin[s] = w
    arcs = np.zeros(len(rows), TR_DTYPE)
    for k, r in enumerate(rows):
        arcs[k] = tuple(r)
    props = int(e["props"], 16) if "props" in e else default_props
    return dict(n_states=n, start=e["start"], offsets=np.array(offsets, np.uint32), arcs=arcs,
                finals=np.array(fin, np.float32), props=props)


def assert_same(got, exp, what):
    assert got["n_states"] == exp["n_states"], f"{what}: num_states {got['n_states']} != {exp['n_states']}"
    assert got["start"] == exp["start"], f"{what}: start"
    np.testing.assert_array_equal(got["offsets"], exp["offsets"], err_msg=f"{what}: offsets")
    for k in ("ilabel", "olabel", "nextstate"):
        np.testing.assert_array_equal(got["arcs"][k], exp["arcs"][k], err_msg=f"{what}: arcs.{k}")
    np.testing.assert_array_equal(got["arcs"]["weight"].view(np.uint32), exp["arcs"]["weight"].view(np.uint32),
                                  err_msg=f"{what}: arc weights (bit pattern)")
    np.testing.assert_array_equal(got["finals"].view(np.uint32), exp["finals"].view(np.uint32),
                                  err_msg=f"{what}: final weights (bit pattern)")
    assert got["props"] == exp["props"], f"{what}: props {got['props']:#x} != {exp['props']:#x}"


def _oracle_dist(oracle, flat, to_final):
    o = to_oracle(oracle, flat)
    if to_final:
        if flat["start"] is None:
            return []
        n = flat["n_states"]
        off, nxt = csr_next(flat)
        ln = int(np.nonzero(reach(n, off, nxt, [flat["start"]]))[0].max()) + 1
        return list(o.shortest_distance()[:ln])
    return list(o.reverse().shortest_distance()[1:][:reverse_len_rule(flat)])
