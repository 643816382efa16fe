"""top_sort on three shapes: a wide DAG (the benchmark generator's graph with the arcs that do not go up in a random rank
dropped and its states renamed at random), a lattice-like DAG of a few hundred states and a deep thin chain of diamonds;
then the worst case: the same graph with ranks = ids, whose ring backbone makes every level one state wide.
For each: the first and the median of repeated calls under WFST_TOP_SORT_PATH=auto, wall clock around the synchronous
call, the counters of wfst_ctx_get_top_sort_stats, and the comparator: the reference's depth-first search restated below on
flat arrays, one core of this host, interpreted Python (so an upper bound for a compiled search, not a stand-in for it).
The device result is checked against state_sort by the comparator's order before anything is printed.
python tools/top_sort_timing.py [wide_n] [diamond_levels] [backbone_n (0: skip)]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import rustfst_amd
from rustfst_amd import synth
from rustfst_amd._lib import TR_DTYPE
from inputs import diamond_chain  # the input the tests use

ctx = None  # main() makes it: importing this file (tools/top_sort_batch_timing.py takes host_dfs_order) starts nothing


def dev(f):
    return rustfst_amd.DeviceFst.from_arrays(f["n_states"], f["start"], f["offsets"], f["arcs"], f["finals"], f["props"], ctx)


def rename(flat, rng):
    """the same machine with its states renamed by a random permutation (rows keep their arc order)"""
    n = flat["n_states"]
    name = rng.permutation(n).astype(np.uint32)
    return apply_order(flat, name)


def apply_order(flat, order):
    """state_sort.rs:16-78 on flat arrays: state order[s] holds s's row, nextstate = order[nextstate]"""
    n = flat["n_states"]
    off = flat["offsets"].astype(np.int64)
    deg = np.diff(off)
    new_deg = np.zeros(n, np.int64)
    new_deg[order] = deg
    new_off = np.concatenate([[0], np.cumsum(new_deg)])
    src = np.repeat(np.arange(n), deg)
    pos = np.arange(len(flat["arcs"])) - off[src]
    arcs = np.empty(len(flat["arcs"]), TR_DTYPE)
    arcs[new_off[order[src]] + pos] = flat["arcs"]
    arcs["nextstate"] = order[arcs["nextstate"]]
    fin = np.empty(n, np.float32)
    fin[order] = flat["finals"]
    return dict(n_states=n, start=int(order[flat["start"]]), offsets=new_off.astype(np.uint32), arcs=arcs, finals=fin, props=0)


def forward_dag(n, rng, ranks):
    """the benchmark generator's graph with the arcs that do not go up in rank dropped.  ranks = n: a state's rank is its
    id, and the generator's ring s -> s + 1 survives as a backbone: n levels of one state, the worst case for a method
    that works level by level.  ranks = 64: random ranks, at most 64 levels, each about n / 64 states wide."""
    t = synth.make_transducer(n)
    off = t["offsets"].astype(np.int64)
    src = np.repeat(np.arange(n), np.diff(off))
    rank = np.arange(n) if ranks == n else rng.integers(0, ranks, n)
    keep = rank[t["arcs"]["nextstate"]] > rank[src]
    deg = np.zeros(n, np.int64)
    np.add.at(deg, src[keep], 1)
    flat = dict(n_states=n, start=0, offsets=np.concatenate([[0], np.cumsum(deg)]).astype(np.uint32), arcs=t["arcs"][keep].copy(),
                finals=t["finals"].astype(np.float32), props=0)
    return rename(flat, rng)


def lattice(rng, layers=120):
    widths = rng.integers(1, 6, layers)
    first = np.concatenate([[0], np.cumsum(widths)])
    rows = [[] for _ in range(int(first[-1]))]
    for k in range(layers - 1):
        for t in range(first[k + 1], first[k + 2]):
            for _ in range(int(rng.integers(1, 4))):
                s = int(rng.integers(first[k], first[k + 1]))
                lab = int(rng.integers(1, 50))
                rows[s].append((lab, lab, float(rng.integers(0, 16)) / 8, t))
    n = len(rows)
    flat = dict(n_states=n, start=0, offsets=np.cumsum([0] + [len(r) for r in rows]).astype(np.uint32),
                arcs=np.array([a for r in rows for a in r], dtype=TR_DTYPE), finals=np.where(np.arange(n) >= first[-2], 0.0, np.inf).astype(np.float32),
                props=0)
    return rename(flat, rng)


def host_dfs_order(flat):
    """dfs_visit.rs:97-187 + TopOrderVisitor (top_sort.rs:12-61) on an acyclic input: order[s] = rank of s in the reverse
    finishing order; roots: the start, then 0, 1, 2, ..; arcs in stored order"""
    n = flat["n_states"]
    off = flat["offsets"].tolist()
    nxt = flat["arcs"]["nextstate"].tolist()
    color = bytearray(n)
    finish = []
    for root in [flat["start"]] + list(range(n)):
        if color[root]:
            continue
        color[root] = 1
        stack = [root]
        pos = [off[root]]
        while stack:
            s = stack[-1]
            i = pos[-1]
            if i == off[s + 1]:
                stack.pop()
                pos.pop()
                finish.append(s)
                continue
            pos[-1] = i + 1
            t = nxt[i]
            if not color[t]:
                color[t] = 1
                stack.append(t)
                pos.append(off[t])
    order = np.empty(n, np.uint32)
    order[np.array(finish[::-1], dtype=np.int64)] = np.arange(n, dtype=np.uint32)
    return order


def timed(fn, reps=5):
    t0 = time.perf_counter(); out = fn(); ctx.synchronize(); first = (time.perf_counter() - t0) * 1e3
    rep = []
    for _ in range(reps):
        t0 = time.perf_counter(); out = fn(); ctx.synchronize(); rep.append((time.perf_counter() - t0) * 1e3)
    return first, float(np.median(rep)), out


def report(name, flat):
    os.environ["WFST_TOP_SORT_PATH"] = "auto"
    d = dev(flat)
    first, rep, out = timed(lambda: d.top_sort())
    st = ctx.top_sort_stats()
    t0 = time.perf_counter(); order = host_dfs_order(flat); host = (time.perf_counter() - t0) * 1e3
    got, exp = out.to_flat(), apply_order(flat, order)
    assert got["start"] == exp["start"] and np.array_equal(got["offsets"], exp["offsets"]) and np.array_equal(got["finals"], exp["finals"])
    assert got["arcs"].tobytes() == exp["arcs"].tobytes(), name
    print(f"{name:9s} {flat['n_states']:>8d} states / {len(flat['arcs']):>8d} arcs   first {first:9.2f} ms   repeated {rep:9.2f} ms"
          f"   host DFS (Python, one core) {host:9.2f} ms", flush=True)
    print(f"          " + "  ".join(f"{k}={v}" for k, v in st.items()), flush=True)


def main(argv):
    global ctx
    wide = int(argv[1]) if len(argv) > 1 else 1_000_000
    diamonds = int(argv[2]) if len(argv) > 2 else 20_000
    backbone = int(argv[3]) if len(argv) > 3 else 100_000
    ctx = rustfst_amd.default_context()
    rng = np.random.default_rng(19)
    report("wide", forward_dag(wide, rng, 64))
    report("lattice", lattice(rng))
    report("diamonds", diamond_chain(diamonds))
    if backbone:
        report("backbone", forward_dag(backbone, rng, backbone))


if __name__ == "__main__":
    main(sys.argv)
