"""Timing of the fused batch with a sigma matcher (wfst_compose_shortest_path_batch_with_matchers) on resident handles.
usage: python tools/compose_sigma_batch_timing.py [--sizes 64 512 4096] [--length 200] [--grammar-states N] [--labels K]
[--repeats R] [--loop-sample M]

n utterances of `length` labels (uniform over 1..K-1) against a sigma grammar of N states — every state has three explicit
labels into its successor and one sigma arc (sigma = K), all acceptor arcs — three ways in the same run:
  (i)   the new call: compose_shortest_path_batch with the MatcherConfig (one launch of the wave-per-utterance kernel);
  (ii)  the loop a caller had to write before: compose with the MatcherConfig + shortest_path per utterance; beyond
        --loop-sample utterances only that many are run and the figure is SCALED to n (the row says so);
  (iii) the plain fused batch on the explicitly expanded grammar (K - 1 arcs per state).
The results of (i) are compared equal with those of (iii), item by item, and with those of (ii) for the items it ran, before a
figure is printed.  Per way: the first call apart, one thrown away, then the median of R calls with [min, max]; host clock
around the blocking call plus a stream synchronisation.  Uploads are reported with their bytes."""
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

ACCEPTOR = 1 << 16


def flat(n, offsets, arcs, finals, props):
    return dict(n_states=n, start=0, offsets=np.ascontiguousarray(offsets, np.uint32), arcs=arcs,
                finals=np.ascontiguousarray(finals, np.float32), props=int(props))


def grammars(n, k):
    """(sigma form, expanded form): state s has explicit labels a < b < c (functions of s) into s + 1 and sigma = k into
    s + 1 + n / 2 (mod n); the expanded form carries every label 1 .. k - 1 at every state"""
    s = np.arange(n, dtype=np.int64)
    base = (s * 2654435761 % (k - 3)) + 1
    ex = np.stack([base, base + 1, base + 2], 1)
    nxt_ex, nxt_sg = (s + 1) % n, (s + 1 + n // 2) % n
    w_ex, w_sg = (s % 7) / 4.0, 1.0 + (s % 5) / 4.0
    g_arcs = np.zeros((n, 4), TR_DTYPE)
    g_arcs["ilabel"][:, :3] = g_arcs["olabel"][:, :3] = ex
    g_arcs["ilabel"][:, 3] = g_arcs["olabel"][:, 3] = k
    g_arcs["weight"][:, :3] = w_ex[:, None]
    g_arcs["weight"][:, 3] = w_sg
    g_arcs["nextstate"][:, :3] = nxt_ex[:, None]
    g_arcs["nextstate"][:, 3] = nxt_sg
    fin = np.zeros(n, np.float32)
    props = synth.I_LABEL_SORTED | synth.O_LABEL_SORTED | ACCEPTOR
    g = flat(n, np.arange(n + 1, dtype=np.int64) * 4, g_arcs.reshape(-1), fin, props)
    e_arcs = np.zeros((n, k - 1), TR_DTYPE)
    e_arcs["ilabel"][:] = e_arcs["olabel"][:] = np.arange(1, k, dtype=np.uint32)[None, :]
    e_arcs["weight"][:] = w_sg[:, None]
    e_arcs["nextstate"][:] = nxt_sg[:, None]
    rows, cols = np.repeat(s, 3), (ex - 1).reshape(-1)
    e_arcs["weight"][rows, cols] = np.repeat(w_ex, 3)
    e_arcs["nextstate"][rows, cols] = np.repeat(nxt_ex, 3)
    return g, flat(n, np.arange(n + 1, dtype=np.int64) * (k - 1), e_arcs.reshape(-1), fin, props)


def upload(f, ctx):
    t = time.perf_counter()
    d = rustfst_amd.DeviceFst.from_arrays(f["n_states"], f["start"], f["offsets"], f["arcs"], f["finals"], f["props"], ctx)
    ctx.synchronize()
    return d, 1e3 * (time.perf_counter() - t), f["offsets"].nbytes + f["arcs"].nbytes + f["finals"].nbytes


def timed(fn, ctx, repeats):
    """(result of the first call, first call ms, [repeat ms]) after one more call that is thrown away"""
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


def fmt(ms, scale=1.0):
    return "%.3f ms [%.3f, %.3f]" % (scale * statistics.median(ms), scale * min(ms), scale * max(ms))


def same(a, b):
    a, b = a.to_flat(), b.to_flat()
    return (a["n_states"] == b["n_states"] and a["start"] == b["start"] and np.array_equal(a["offsets"], b["offsets"])
            and np.array_equal(a["arcs"], b["arcs"]) and np.array_equal(a["finals"].view(np.uint32), b["finals"].view(np.uint32))
            and a["props"] == b["props"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 512, 4096])
    ap.add_argument("--length", type=int, default=200)
    ap.add_argument("--grammar-states", type=int, default=20000)
    ap.add_argument("--labels", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--loop-sample", type=int, default=512)
    a = ap.parse_args()
    assert a.repeats >= 9 and a.labels >= 8
    ctx = rustfst_amd.Context(0)
    rustfst_amd.set_default_context(ctx)
    g, e = grammars(a.grammar_states, a.labels)
    dg, up_g, by_g = upload(g, ctx)
    de, up_e, by_e = upload(e, ctx)
    print("grammar: %d states; sigma form %d B uploaded in %.1f ms, expanded form %d B in %.1f ms" % (a.grammar_states, by_g, up_g, by_e, up_e))
    sigma_cfg = ComposeConfig(ComposeFilter.SEQUENCEFILTER, True, None, MatcherConfig(a.labels))
    plain_cfg = ComposeConfig(ComposeFilter.SEQUENCEFILTER, True)
    print("| utterances x labels | repeats | (i) new call: first, median [min, max] | (ii) loop of compose + shortest_path | "
          "(iii) plain batch, expanded grammar | (ii) / (i) | (i) / (iii) |")
    print("|---|---|---|---|---|---|---|")
    for n in a.sizes:
        rng = np.random.default_rng(100 + n)
        strs = [synth.linear_acceptor_flat(rng.integers(1, a.labels, a.length)) for _ in range(n)]
        handles = rustfst_amd.DeviceFst.upload_many(strs, ctx)
        ctx.synchronize()
        r1, first1, ms1 = timed(lambda: rustfst_amd.compose_shortest_path_batch(handles, dg, sigma_cfg, ctx=ctx)[0], ctx, a.repeats)
        st = ctx.sigma_batch_stats()
        m = min(n, a.loop_sample)
        r2, first2, ms2 = timed(lambda: [handles[i].compose(dg, sigma_cfg).shortest_path() for i in range(m)], ctx, a.repeats)
        r3, first3, ms3 = timed(lambda: rustfst_amd.compose_shortest_path_batch(handles, de, plain_cfg, ctx=ctx)[0], ctx, a.repeats)
        path = ctx.compose_path_stats()
        assert all(same(r1[i], r3[i]) for i in range(n)), "the new call and the plain batch on the expanded grammar differ"
        assert all(same(r1[i], r2[i]) for i in range(m)), "the new call and the loop differ"
        assert all(r1[i].to_flat()["n_states"] == a.length + 1 for i in range(n))
        scale = n / m
        note = "" if m == n else " (SCALED from a sample of %d)" % m
        med1, med2, med3 = statistics.median(ms1), scale * statistics.median(ms2), statistics.median(ms3)
        print("| %d x %d | %d | %.3f ms, %s | %.3f ms, %s%s | %.3f ms, %s | %.1f | %.2f |"
              % (n, a.length, a.repeats, first1, fmt(ms1), scale * first2, fmt(ms2, scale), note, first3, fmt(ms3), med2 / med1, med1 / med3))
        print("  counters of (i):", st, "; string kernel answered %d of (iii)" % path["string_answered"], flush=True)
        del r1, r2, r3, handles


if __name__ == "__main__":
    main()
