"""minimize of a batch of small lattices: ONE wfst_minimize_batch call against the same items as a loop of n wfst_minimize
calls in the same process.  Prints a markdown table (profiles/minimize_batch_timing.md).

    python tools/minimize_batch_timing.py [--sizes 64 512 4096] [--runs 20] [--warmup 3] [--long-runs 3] [--step-timeout 600]

Inputs: the random lattice-like DAG acceptors of tools/determinize_batch_timing.py (50-500 states, seeded), determinized
with one determinize_batch call: what a rescoring loop hands to minimize.  Every item stays in the batch kernel.
Every size is one step, run in a child process of its own under `timeout` (a step that fails or runs out of time ends the
tool: nothing more is started on the device).  A step checks first that the batch results equal the single calls' (arrays
bit for bit, start state, property word), then times with the host clock around the blocking calls, after `warmup`
calls: median [min, max] of `runs` calls of the batch; the loop of single calls takes seconds from 512 items on and is
timed over `long-runs` calls after the one of the equality check."""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def same(a, b):
    return (a["n_states"] == b["n_states"] and a["start"] == b["start"] and a["props"] == b["props"]
            and np.array_equal(a["offsets"], b["offsets"]) and a["arcs"].tobytes() == b["arcs"].tobytes()
            and a["finals"].tobytes() == b["finals"].tobytes())


def step(n, a):
    import rustfst_amd
    from determinize_batch_timing import lattice
    rng = np.random.default_rng(4242)
    flats = [lattice(rng) for _ in range(n)]
    ctx = rustfst_amd.Context(0)
    dets = rustfst_amd.determinize_batch(rustfst_amd.DeviceFst.upload_many(flats, ctx), None, ctx)
    arr = rustfst_amd.HandleArray(dets)
    outs, flags = rustfst_amd.minimize_batch(arr, None, ctx, return_in_kernel=True)
    assert flags.all(), "an item left the batch kernel"
    st = rustfst_amd.minimize_batch_stats(ctx)
    singles = [d.minimize() for d in dets]
    for k, (o, s) in enumerate(zip(outs, singles)):
        assert same(o.to_flat(), s.to_flat()), f"item {k}: the batch result differs from the single call's"
    n_in, n_out = sum(d.num_states for d in dets), sum(o.num_states for o in outs)
    del outs, singles
    batch = timed(lambda: rustfst_amd.minimize_batch(arr, None, ctx), a.runs, a.warmup)
    loop = timed(lambda: [d.minimize() for d in dets], a.runs if n <= 64 else a.long_runs, a.warmup if n <= 64 else 0)
    print(f"| {n} | {n_in} / {n_out} | {cell(batch)} | {cell(loop)} | {loop[0] / batch[0]:.1f}x | {st['launches']} |", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 512, 4096])
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--long-runs", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=600, help="seconds one size may take")
    ap.add_argument("--step", type=int, default=0, help=argparse.SUPPRESS)  # (the child: one size)
    a = ap.parse_args()
    if a.step:
        return step(a.step, a)
    print("ms per call: median [min, max] (runs); results equal the single calls' at every size\n")
    print("| items | states in / out | one minimize_batch call | loop of n minimize calls | loop / batch | batch kernel launches |")
    print("|---|---|---|---|---|---|", flush=True)
    for n in a.sizes:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", str(n),
               "--runs", str(a.runs), "--warmup", str(a.warmup), "--long-runs", str(a.long_runs)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"<!-- the step of {n} items ended with status {rc}: stopped -->", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
