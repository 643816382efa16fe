"""isomorphic and invert on the inputs of the README row: the benchmark's T (1 M states / 10 M arcs) against a copy with its
states renamed and its rows shuffled; the same with one arc weight changed in the last level of the search; the lattice-like
DAG of the top_sort row; a chain of 100 000 states; invert of T.
For each: the first and the median of repeated calls under WFST_ISOMORPHIC_PATH=auto, wall clock around the synchronous
call, and the counters of wfst_ctx_get_isomorphic_counters.  No compiled comparator exists: for the small inputs the time of
the reference's search restated in interpreted Python (tests/isomorphic_ref.py, one core of this host: an upper bound for a
compiled search, not a stand-in for it), whose verdict the device's is checked against; for the large inputs the time of
downloading both operands, which is what the call replaces.
python tools/isomorphic_timing.py [n_states of T] [chain length]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import rustfst_amd
from rustfst_amd import synth
from oracle.model import flat_to_fst, fst_to_flat
import isomorphic_cases as K
import isomorphic_ref as R
from top_sort_timing import apply_order, forward_dag, lattice

ctx = None


def dev(f):
    return rustfst_amd.DeviceFst.from_arrays(f["n_states"], f["start"], f["offsets"], f["arcs"], f["finals"], f["props"], ctx)


def permuted(flat, rng):
    """the states renamed by a random permutation, every row in a random stored order"""
    out = apply_order(flat, rng.permutation(flat["n_states"]).astype(np.uint32))
    off = out["offsets"].astype(np.int64)
    src = np.repeat(np.arange(out["n_states"]), np.diff(off))
    out["arcs"] = out["arcs"][np.lexsort((rng.random(len(src)), src))]
    return out


def last_level_arc(flat):
    """an arc of a state on the last breadth-first level that has arcs: (state, position in its row)"""
    n, off, nxt = flat["n_states"], flat["offsets"].astype(np.int64), flat["arcs"]["nextstate"]
    src = np.repeat(np.arange(n), np.diff(off))
    depth = np.full(n, -1, np.int64)
    depth[flat["start"]] = 0
    d = 0
    while True:
        t = np.unique(nxt[depth[src] == d])
        t = t[depth[t] < 0]
        if not len(t):
            break
        d += 1
        depth[t] = d
    with_arcs = np.nonzero((np.diff(off) > 0) & (depth >= 0))[0]
    s = int(with_arcs[np.argmax(depth[with_arcs])])
    return s, 0, int(depth[s]) + 1


def timed(fn, reps=5):
    t0 = time.perf_counter(); out = fn(); ctx.synchronize(); first = (time.perf_counter() - t0) * 1e3
    rep = []
    for _ in range(reps):
        t0 = time.perf_counter(); out = fn(); ctx.synchronize(); rep.append((time.perf_counter() - t0) * 1e3)
    return first, float(np.median(rep)), out


def verdict_of(d1, d2):
    try:
        return 1 if d1.isomorphic(d2) else 0
    except rustfst_amd.WfstError as e:
        return str(e).split(": ", 1)[1]


def report(name, f1, f2, small):
    os.environ["WFST_ISOMORPHIC_PATH"] = "auto"
    d1, d2 = dev(f1), dev(f2)
    first, rep, got = timed(lambda: verdict_of(d1, d2))
    st = ctx.isomorphic_stats()
    if small:
        a, b = flat_to_fst(f1), flat_to_fst(f2)
        t0 = time.perf_counter(); exp = R.verdict(a, b); other = (time.perf_counter() - t0) * 1e3
        assert got == exp, (name, got, exp)
        what = "restatement (Python, one core)"
    else:
        e1, e2 = dev(f1), dev(f2)  # fresh handles: nothing of them is on the host
        ctx.synchronize()
        t0 = time.perf_counter(); e1.to_flat(); e2.to_flat(); other = (time.perf_counter() - t0) * 1e3
        what = "download of both operands"
    print(f"{name:14s} {f1['n_states']:>8d} states / {len(f1['arcs']):>8d} arcs   verdict {got!r:>3}   first {first:9.2f} ms   "
          f"repeated {rep:9.2f} ms   {what} {other:9.2f} ms", flush=True)
    print("               " + "  ".join(f"{k}={v}" for k, v in st.items()), flush=True)


def main(argv):
    global ctx
    n = int(argv[1]) if len(argv) > 1 else 1_000_000
    chain_n = int(argv[2]) if len(argv) > 2 else 100_000
    ctx = rustfst_amd.default_context()
    rng = np.random.default_rng(22)
    t = synth.make_transducer(n, 10, 256, 0.0, seed=3)
    tp = permuted(t, rng)
    report("T permuted", t, tp, small=False)
    s, k, levels = last_level_arc(tp)
    changed = dict(tp, arcs=tp["arcs"].copy())
    changed["arcs"]["weight"][int(tp["offsets"][s]) + k] += np.float32(1.0)
    print(f"               (one weight changed at state {s}, breadth-first level {levels})")
    report("T one weight", t, changed, small=False)
    rng19 = np.random.default_rng(19)  # the top_sort row's lattice: the second input of tools/top_sort_timing.py
    forward_dag(1_000_000, rng19, 64)
    lat = lattice(rng19)
    report("lattice", lat, permuted(lat, rng), small=True)
    ch = fst_to_flat(K.chain(chain_n))
    report("chain", ch, permuted(ch, rng), small=True)
    d = dev(t)
    first, rep, _ = timed(lambda: d.invert(), reps=6)  # (an even number of edits after the first: T again, then inverted)
    e = dev(t)
    ctx.synchronize()
    t0 = time.perf_counter(); flat = e.to_flat(); down = (time.perf_counter() - t0) * 1e3
    arcs = flat["arcs"].copy()
    t0 = time.perf_counter(); arcs["ilabel"], arcs["olabel"] = flat["arcs"]["olabel"], flat["arcs"]["ilabel"].copy(); swap = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter(); dev(dict(flat, arcs=arcs)); ctx.synchronize(); up = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(d.to_flat()["arcs"]["ilabel"], flat["arcs"]["olabel"])  # seven edits: inverted
    print(f"{'invert T':14s} {n:>8d} states / {len(t['arcs']):>8d} arcs   first {first:9.2f} ms   repeated {rep:9.2f} ms   "
          f"download {down:.2f} + swap on the host {swap:.2f} + upload {up:.2f} ms", flush=True)


if __name__ == "__main__":
    main(sys.argv)
