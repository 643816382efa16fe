"""replace on three shapes: a wide expansion (a root whose start state has a few thousand call arcs into some tens of
word-list FSTs), a deep one (nesting depth 10, four states per FST, two calls each) and a thin chain (one call per root
state, every level of the search one state wide).
For each: the first and the median of repeated calls, wall clock around the synchronous call (uploads not included), the
counters of wfst_ctx_get_replace_stats, and the sizes the shape must give by construction, which are checked before anything
is printed.  The level kernels the call queued (la_emit, la_first, la_assign of compose_wide.h, up to eight levels per look
of the host at the control block) are counted by the driver: the tool prints levels, launches per level and levels per
millisecond.
No compiled comparator exists in this repository (the reference is Rust), and the Python restatement of
tests/replace_ref.py is a checker, not a baseline: no CPU figure is given.
python tools/replace_timing.py [wide_calls] [deep_depth] [chain_calls] [repeats]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import rustfst_amd
from rustfst_amd._lib import TR_DTYPE

WIDE = int(sys.argv[1]) if len(sys.argv) > 1 else 4000
DEPTH = int(sys.argv[2]) if len(sys.argv) > 2 else 10
CHAIN = int(sys.argv[3]) if len(sys.argv) > 3 else 10_000
REPEATS = int(sys.argv[4]) if len(sys.argv) > 4 else 5
ctx = rustfst_amd.default_context()


def dev(rows, finals):
    """rows[state] = [(ilabel, olabel, weight, nextstate), ...], start state 0, stored word 0"""
    off = np.zeros(len(rows) + 1, np.uint32)
    off[1:] = np.cumsum([len(r) for r in rows])
    arcs = np.array([a for r in rows for a in r], dtype=TR_DTYPE) if off[-1] else np.zeros(0, TR_DTYPE)
    fin = np.array([np.inf if f is None else f for f in finals], np.float32)
    return rustfst_amd.DeviceFst.from_arrays(len(rows), 0, off, arcs, fin, 0, ctx)


def word_list(n_words, length, seed):
    """n_words linear branches of `length` arcs from the start state into one final state"""
    rows, last = [[]], 1 + n_words * (length - 1)
    for w in range(n_words):
        prev = 0
        for k in range(length):
            nxt = last if k + 1 == length else len(rows)
            if nxt != last:
                rows.append([])
            rows[prev].append((1 + (seed + w + k) % 50, 1 + (seed + w + k) % 50, ((w + k) % 8) / 8, nxt))
            prev = nxt
    rows.append([])
    return dev(rows, [None] * last + [0.0]), last + 1, n_words * length


def wide(n_calls, n_lists=40, n_words=50, length=6):
    keys = [1000 + k for k in range(n_lists)]
    root = dev([[(1 + s % 9, keys[s % n_lists], (s % 8) / 8, 1 + s) for s in range(n_calls)]] + [[] for _ in range(n_calls)],
               [None] + [0.0] * n_calls)
    lists = [word_list(n_words, length, k) for k in range(n_lists)]
    states = 1 + n_calls + sum(lists[s % n_lists][1] for s in range(n_calls))
    arcs = n_calls + sum(lists[s % n_lists][2] + 1 for s in range(n_calls))  # + the return arc of each copy's final state
    return [(999, root)] + [(keys[k], lists[k][0]) for k in range(n_lists)], 999, (states, arcs, n_calls)


def deep(depth):
    """FST d: 0 -a-> 1 -call d+1-> 2 -call d+1-> 3 (final); the last FST has terminals in place of the calls"""
    keys = [1000 + d for d in range(depth + 1)]
    pairs = []
    for d in range(depth + 1):
        ol = keys[d + 1] if d < depth else 7
        pairs.append((keys[d], dev([[(1, 1, 0.125, 1)], [(2, ol, 0.25, 2)], [(3, ol, 0.5, 3)], []], [None, None, None, 0.0])))
    copies = 2 ** (depth + 1) - 1  # 1 + 2 + 4 + .. + 2^depth instances
    states = 4 * copies
    arcs = 3 * copies + (copies - 1)  # + one return arc per called instance
    return pairs, keys[0], (states, arcs, copies - 1)


def chain(n_calls, n_words=50):
    keys = [1000 + k for k in range(n_words)]
    root = dev([[(1, keys[s % n_words], (s % 8) / 8, s + 1)] for s in range(n_calls)] + [[]], [None] * n_calls + [0.5])
    words = []
    for k in range(n_words):
        length = 1 + k % 4
        words.append((dev([[(2, 2, 0.125, s + 1)] for s in range(length)] + [[]], [None] * length + [0.0]), length))
    states = n_calls + 1 + sum(words[s % n_words][1] + 1 for s in range(n_calls))
    arcs = n_calls + sum(words[s % n_words][1] + 1 for s in range(n_calls))
    return [(999, root)] + [(keys[k], words[k][0]) for k in range(n_words)], 999, (states, arcs, n_calls)


def run(name, pairs, root, want):
    times = []
    for _ in range(1 + REPEATS):
        t0 = time.perf_counter()
        out = rustfst_amd.replace(root, pairs, True)
        ctx.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        st = ctx.replace_stats()
        assert (st["states"], st["arcs"], st["prefixes"]) == want, (name, st, want)
        del out
    rep = sorted(times[1:])
    print(f"{name}: first {times[0]:.2f} ms, repeated median {rep[len(rep) // 2]:.2f} ms [{rep[0]:.2f}, {rep[-1]:.2f}] ({len(rep)} calls); "
          f"states {st['states']}, arcs {st['arcs']}, levels {st['levels']} ({st['levels'] / rep[len(rep) // 2]:.1f} per ms), level launches "
          f"{st['level_launches']} ({st['level_launches'] / st['levels']:.2f} per level), prefixes {st['prefixes']}, deepest stack {st['max_depth']}, arena grows {st['arena_grows']}, "
          f"prefix-table reruns {st['prefix_reruns']}", flush=True)


if __name__ == "__main__":
    run(f"wide ({WIDE} call arcs of one state into 40 word lists of 50 words)", *wide(WIDE))
    run(f"deep (depth {DEPTH}, two calls per instance)", *deep(DEPTH))
    run(f"thin chain ({CHAIN} calls, one per root state)", *chain(CHAIN))
