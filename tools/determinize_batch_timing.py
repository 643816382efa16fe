"""determinize of a batch of small lattices: ONE wfst_determinize_batch call (both WFST_DETERMINIZE_BATCH_SCRATCH variants)
against the same items as n wfst_determinize calls in the same process and against the CPU oracle on one core, with and
without out_dist.  Prints a markdown table (profiles/determinize_batch_timing.md).

    python tools/determinize_batch_timing.py [--sizes 64 512 4096] [--runs 20] [--warmup 3] [--long-runs 5]

Inputs: random lattice-like DAG acceptors of 50-500 states (seeded): state s has 1-3 arcs into s+1 .. s+4, labels 1..6,
weights on the 1/512 grid, the last state final.  Every item stays in the batch kernel (levels of a handful of states).
Timed with the host clock around the blocking call, after `warmup` calls: median [min, max] of `runs` calls; the rows that
take seconds per call (n single calls or the oracle at 512 and 4096 items) use `long-runs` calls and say so."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rustfst_amd  # noqa: E402
from rustfst_amd import synth  # noqa: E402
from rustfst_amd._lib import TR_DTYPE  # noqa: E402
from oracle.model.props import ACCEPTOR  # noqa: E402


def lattice(rng):
    n = int(rng.integers(50, 501))
    deg = rng.integers(1, 4, n)
    deg[n - 1] = 0
    off = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint32)
    src = np.repeat(np.arange(n), deg)
    arcs = np.zeros(len(src), TR_DTYPE)
    arcs["ilabel"] = rng.integers(1, 7, len(src))
    arcs["nextstate"] = np.minimum(src + 1 + rng.integers(0, 4, len(src)), n - 1)
    arcs["weight"] = rng.integers(0, 2560, len(src)).astype(np.float32) / np.float32(512)
    order = np.lexsort((arcs["ilabel"], src))  # ilabel-sorted per state
    arcs = arcs[order]
    arcs["olabel"] = arcs["ilabel"]
    fin = np.full(n, np.inf, np.float32)
    fin[n - 1] = 0.0
    return dict(n_states=n, start=0, offsets=off, arcs=arcs, finals=fin, props=ACCEPTOR | synth.I_LABEL_SORTED)


def timed(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts), runs


def cell(r):
    return "%.3f [%.3f, %.3f] (%d)" % r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 512, 4096])
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--long-runs", type=int, default=5)
    ap.add_argument("--no-oracle", action="store_true")
    a = ap.parse_args()
    rng = np.random.default_rng(4242)
    flats = [lattice(rng) for _ in range(max(a.sizes))]
    ctx = rustfst_amd.Context(0)
    devs = rustfst_amd.DeviceFst.upload_many(flats, ctx)
    dists = [d.shortest_distance(reverse=True) for d in devs]
    orc = None
    if not a.no_oracle:
        from oracle import oracle_py
        orc = [oracle_py.OracleFst.from_flat(f["n_states"], f["start"], f["offsets"], f["arcs"], f["finals"], f["props"])
               for f in flats]
    print("ms per call: median [min, max] (runs)\n")
    print("| items | states in / out | batch, lds | batch, global | n single calls | batch + dist, lds | batch + dist, global "
          "| n single calls + dist | oracle, one core |")
    print("|---|---|---|---|---|---|---|---|---|")
    for n in a.sizes:
        ds, dd = rustfst_amd.HandleArray(devs[:n]), dists[:n]
        long_runs = a.runs if n <= 64 else a.long_runs
        row = {}
        for scratch in ("lds", "global"):
            os.environ["WFST_DETERMINIZE_BATCH_SCRATCH"] = scratch
            outs, flags = rustfst_amd.determinize_batch(ds, None, ctx, want_flags=True)
            assert flags.all(), "an item left the batch kernel"
            st = rustfst_amd.determinize_batch_stats(ctx)
            n_out = sum(o.num_states for o in outs)
            del outs
            row[scratch] = timed(lambda: rustfst_amd.determinize_batch(ds, None, ctx), a.runs, a.warmup)
            row[scratch + "_d"] = timed(lambda: rustfst_amd.determinize_with_distance_batch(ds, dd, ctx=ctx), a.runs, a.warmup)
            row[scratch + "_launches"] = st["launches"]
        del os.environ["WFST_DETERMINIZE_BATCH_SCRATCH"]
        row["single"] = timed(lambda: [d.determinize() for d in devs[:n]], long_runs, 1 if n > 64 else a.warmup)
        row["single_d"] = timed(lambda: [rustfst_amd.determinize_with_distance(d, x) for d, x in zip(devs[:n], dd)],
                                long_runs, 1 if n > 64 else a.warmup)
        if orc:
            row["oracle"] = cell(timed(lambda: [o.determinize_fsa() for o in orc[:n]], long_runs, 1))
        else:
            row["oracle"] = "not run"
        n_in = sum(f["n_states"] for f in flats[:n])
        print(f"| {n} | {n_in} / {n_out} | {cell(row['lds'])} | {cell(row['global'])} | {cell(row['single'])} | "
              f"{cell(row['lds_d'])} | {cell(row['global_d'])} | {cell(row['single_d'])} | {row['oracle']} |", flush=True)
        print(f"<!-- n = {n}: launches per batch call: lds {row['lds_launches']}, global {row['global_launches']} -->", flush=True)


if __name__ == "__main__":
    main()
