"""Timing of the sigma-matcher composition (wfst_compose_with_matchers) against the plain composition of the explicitly
expanded grammar, on resident handles.  usage: python tools/compose_sigma_timing.py [--grammar-states N] [--lattice-levels L]
[--lattice-width W] [--labels K] [--repeats R] [--skip-large]

Two workloads, each run both ways and compared equal before a figure is printed:
  (a) small   a three-label query against the four-state "play <sigma> please" grammar (expanded: one arc per label)
  (b) large   a lattice of L levels x W states (three arcs per state into the next level, labels 1..K-1) against a grammar
              of N states in which every state has one sigma arc (sigma = K) and three explicit arcs, all of them
              acceptor arcs; the expanded grammar has K - 1 arcs per state
fst1 says NOT_O_LABEL_SORTED, so that both runs iterate it (the expansion identity of tests/test_compose_sigma.py).
For (a) the C++ oracle's plain composition of the expanded form on one CPU core is timed as well.
Host clock around the blocking call plus a stream synchronisation; uploads are timed apart and reported with their bytes."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rustfst_amd  # noqa: E402
from rustfst_amd import ComposeConfig, ComposeFilter, MatcherConfig, synth  # noqa: E402
from rustfst_amd._lib import TR_DTYPE  # noqa: E402

NOT_I_LABEL_SORTED, NOT_O_LABEL_SORTED = synth.I_LABEL_SORTED << 1, synth.O_LABEL_SORTED << 1
ACCEPTOR = 1 << 16


def flat(n, offsets, arcs, finals, props):
    return dict(n_states=n, start=0, offsets=np.ascontiguousarray(offsets, np.uint32), arcs=arcs,
                finals=np.ascontiguousarray(finals, np.float32), props=int(props))


def upload(f, ctx):
    t = time.perf_counter()
    d = rustfst_amd.DeviceFst.from_arrays(f["n_states"], f["start"], f["offsets"], f["arcs"], f["finals"], f["props"], ctx)
    ctx.synchronize()
    return d, 1e3 * (time.perf_counter() - t), f["offsets"].nbytes + f["arcs"].nbytes + f["finals"].nbytes


def timed(fn, ctx, repeats):
    """(result of the first call, first call ms, [repeat ms]) after one more warm-up call"""
    t = time.perf_counter()
    first = fn()
    ctx.synchronize()
    first_ms = 1e3 * (time.perf_counter() - t)
    fn()
    ctx.synchronize()
    ms = []
    for _ in range(repeats):
        t = time.perf_counter()
        r = fn()
        ctx.synchronize()
        ms.append(1e3 * (time.perf_counter() - t))
        del r
    return first, first_ms, ms


def fmt(ms):
    return "%.3f ms [%.3f, %.3f]" % (statistics.median(ms), min(ms), max(ms))


def same(a, b):
    a, b = a.to_flat(), b.to_flat()
    return (a["n_states"] == b["n_states"] and np.array_equal(a["offsets"], b["offsets"]) and np.array_equal(a["arcs"], b["arcs"])
            and np.array_equal(a["finals"].view(np.uint32), b["finals"].view(np.uint32)) and a["props"] == b["props"])


def chain(labels, props):
    n = len(labels)
    arcs = np.zeros(n, TR_DTYPE)
    arcs["ilabel"] = arcs["olabel"] = labels
    arcs["nextstate"] = np.arange(1, n + 1)
    return flat(n + 1, np.r_[np.arange(n + 1), n], arcs, np.r_[np.full(n, np.inf), 0.0], props)


def small(k):
    """query play X please; grammar play <sigma> please with sigma = k; expanded: state 1 carries every label but sigma"""
    q = chain([2, 3, 5], synth.I_LABEL_SORTED | NOT_O_LABEL_SORTED | ACCEPTOR)
    g = chain([2, k, 5], synth.I_LABEL_SORTED | synth.O_LABEL_SORTED | ACCEPTOR)
    labs = np.arange(1, k, dtype=np.uint32)
    arcs = np.zeros(2 + labs.size, TR_DTYPE)
    arcs["ilabel"] = arcs["olabel"] = np.r_[2, labs, 5]
    arcs["nextstate"] = np.r_[1, np.full(labs.size, 2), 3]
    e = flat(4, [0, 1, 1 + labs.size, 2 + labs.size, 2 + labs.size], arcs, [np.inf, np.inf, np.inf, 0.0], g["props"])
    return q, g, e


def large(n, levels, width, k, seed=5):
    rng = np.random.default_rng(seed)
    # lattice: level l holds states 1 + (l - 1) * width ..; the start state fans out into level 1; the last level is final
    n1 = 1 + levels * width
    deg = np.full(n1, 3, np.int64)
    deg[0] = min(width, 64)
    deg[1 + (levels - 1) * width:] = 0
    off = np.r_[0, np.cumsum(deg)]
    arcs = np.zeros(off[-1], TR_DTYPE)
    src = np.repeat(np.arange(n1), deg)
    level = np.where(src == 0, 0, (src - 1) // width + 1)
    arcs["ilabel"] = arcs["olabel"] = rng.integers(1, k, off[-1])
    arcs["weight"] = rng.integers(0, 2048, off[-1]) / 512.0
    arcs["nextstate"] = 1 + level * width + rng.integers(0, width, off[-1])
    fin = np.full(n1, np.inf, np.float32)
    fin[1 + (levels - 1) * width:] = 0.0
    q = flat(n1, off, arcs, fin, NOT_I_LABEL_SORTED | NOT_O_LABEL_SORTED | ACCEPTOR)
    # grammar: state s has explicit labels a < b < c (functions of s) into s + 1, and sigma into s + 1 + n / 2 (mod n)
    s = np.arange(n, dtype=np.int64)
    base = (s * 2654435761 % (k - 3)) + 1  # 1 .. k - 3
    ex = np.stack([base, base + 1, base + 2], 1)  # three distinct labels in 1 .. k - 1
    nxt_ex, nxt_sg = (s + 1) % n, (s + 1 + n // 2) % n
    w_ex, w_sg = (s % 7) / 4.0, 1.0 + (s % 5) / 4.0
    g_arcs = np.zeros((n, 4), TR_DTYPE)
    g_arcs["ilabel"][:, :3] = g_arcs["olabel"][:, :3] = ex
    g_arcs["ilabel"][:, 3] = g_arcs["olabel"][:, 3] = k
    g_arcs["weight"][:, :3] = w_ex[:, None]
    g_arcs["weight"][:, 3] = w_sg
    g_arcs["nextstate"][:, :3] = nxt_ex[:, None]
    g_arcs["nextstate"][:, 3] = nxt_sg
    gfin = np.zeros(n, np.float32)
    gprops = synth.I_LABEL_SORTED | synth.O_LABEL_SORTED | ACCEPTOR
    g = flat(n, np.arange(n + 1, dtype=np.int64) * 4, g_arcs.reshape(-1), gfin, gprops)
    # expanded: every label 1 .. k - 1 at every state, the explicit ones as they are, the others the rewritten sigma arc
    e_arcs = np.zeros((n, k - 1), TR_DTYPE)
    e_arcs["ilabel"][:] = e_arcs["olabel"][:] = np.arange(1, k, dtype=np.uint32)[None, :]
    e_arcs["weight"][:] = w_sg[:, None]
    e_arcs["nextstate"][:] = nxt_sg[:, None]
    rows = np.repeat(s, 3)
    cols = (ex - 1).reshape(-1)
    e_arcs["weight"][rows, cols] = np.repeat(w_ex, 3)
    e_arcs["nextstate"][rows, cols] = np.repeat(nxt_ex, 3)
    e = flat(n, np.arange(n + 1, dtype=np.int64) * (k - 1), e_arcs.reshape(-1), gfin, gprops)
    return q, g, e


def run(name, q, g, e, k, ctx, repeats, cpu=False):
    dq, up_q, by_q = upload(q, ctx)
    dg, up_g, by_g = upload(g, ctx)
    de, up_e, by_e = upload(e, ctx)
    sigma_cfg = ComposeConfig(ComposeFilter.SEQUENCEFILTER, False, None, MatcherConfig(k))
    plain_cfg = ComposeConfig(ComposeFilter.SEQUENCEFILTER, False)
    rs, first_s, ms_s = timed(lambda: dq.compose(dg, sigma_cfg), ctx, repeats)
    st = ctx.compose_sigma_stats()
    rp, first_p, ms_p = timed(lambda: dq.compose(de, plain_cfg), ctx, repeats)
    path = ctx.compose_path_stats()
    assert same(rs, rp), name + ": the sigma call and the plain composition of the expanded grammar differ"
    n, a = rs.to_flat()["n_states"], len(rs.to_flat()["arcs"])
    print("| %s | %d / %d | %d | sigma: %.3f ms, %s; %d levels, %d launches, %d grows | plain(expanded): %.3f ms, %s; "
          "switched_wide %d | upload sigma form %d B (%.1f ms), expanded form %d B (%.1f ms), fst1 %d B (%.1f ms) |"
          % (name, n, a, repeats, first_s, fmt(ms_s), st["levels"], st["level_launches"], st["arena_grows"], first_p, fmt(ms_p),
             path["switched_wide"], by_g, up_g, by_e, up_e, by_q, up_q))
    print("  counters:", st)
    if cpu:
        from oracle import oracle_py

        def orc(f):
            return oracle_py.OracleFst.from_flat(f["n_states"], f["start"], f["offsets"], f["arcs"], f["finals"], f["props"])
        oq, oe = orc(q), orc(e)
        ms = []
        for _ in range(repeats + 2):
            t = time.perf_counter()
            oq.compose(oe, connect=False, compose_filter=3)
            ms.append(1e3 * (time.perf_counter() - t))
        print("  one CPU core, C++ oracle, plain composition of the expanded form: first %.3f ms, then %s" % (ms[0], fmt(ms[2:])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grammar-states", type=int, default=1_000_000)
    ap.add_argument("--lattice-levels", type=int, default=100)
    ap.add_argument("--lattice-width", type=int, default=1000)
    ap.add_argument("--labels", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--skip-large", action="store_true")
    a = ap.parse_args()
    assert a.repeats >= 9 and a.labels >= 8
    ctx = rustfst_amd.Context(0)
    rustfst_amd.set_default_context(ctx)
    print("| workload | states / arcs | repeats | sigma call: first, median [min, max] | plain: first, median [min, max] | uploads |")
    print("|---|---|---|---|---|---|")
    run("(a) small", *small(a.labels), a.labels, ctx, a.repeats, cpu=True)
    if not a.skip_large:
        t = time.perf_counter()
        q, g, e = large(a.grammar_states, a.lattice_levels, a.lattice_width, a.labels)
        print("  (built the large inputs on the host in %.1f s)" % (time.perf_counter() - t), flush=True)
        run("(b) large", q, g, e, a.labels, ctx, a.repeats)


if __name__ == "__main__":
    main()
