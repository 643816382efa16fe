"""top_sort of a batch of small lattices: ONE wfst_top_sort_batch call against the same items as a loop of n wfst_top_sort
calls in the same process; at 64 items also the reference's depth-first search restated in interpreted Python
(tools/top_sort_timing.py host_dfs_order: one core of this host, the order only, no arrays permuted).  Prints a markdown
table (profiles/top_sort_batch_timing.md).

    python tools/top_sort_batch_timing.py [--sizes 64 512 4096] [--runs 20] [--warmup 3] [--long-runs 3] [--step-timeout 600]

Inputs: the random lattice-like DAG acceptors of tools/determinize_batch_timing.py (50-500 states, seeded; arcs lead to
higher state ids, the word does not say so).
Every size is one step, run in a child process of its own under `timeout` (a step that fails or runs out of time ends the
tool: nothing more is started on the device).  A step checks first that the batch results equal the single calls' (arrays
bit for bit, start state, property word), then times with the host clock around the blocking calls, after `warmup` calls:
median [min, max] of `runs` calls of the batch; the loop of single calls is timed over `runs` calls at up to 64 items and
over `long-runs` calls beyond.  No ratio is expected in advance: the comparator is the loop on the same commit in the same
run."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from rm_epsilon_batch_timing import cell, same, timed  # noqa: E402


def step(n, a):
    import rustfst_amd
    from determinize_batch_timing import lattice
    from top_sort_timing import host_dfs_order
    ctx = rustfst_amd.Context(0)
    rng = np.random.default_rng(4242)
    flats = [lattice(rng) for _ in range(n)]
    devs = rustfst_amd.DeviceFst.upload_many(flats, ctx)
    arr = rustfst_amd.HandleArray(devs)
    outs, flags = rustfst_amd.top_sort_batch(arr, ctx, return_in_kernel=True)
    st = rustfst_amd.top_sort_batch_stats(ctx)
    singles = [d.top_sort() for d in devs]
    for k, (o, s) in enumerate(zip(outs, singles)):
        assert same(o.to_flat(), s.to_flat()), f"item {k}: the batch result differs from the single call's"
    states, arcs = sum(f["n_states"] for f in flats), sum(len(f["arcs"]) for f in flats)
    del outs, singles
    batch = timed(lambda: rustfst_amd.top_sort_batch(arr, ctx), a.runs, a.warmup)
    loop = timed(lambda: [d.top_sort() for d in devs], a.runs if n <= 64 else a.long_runs, a.warmup if n <= 64 else 0)
    host = cell(timed(lambda: [host_dfs_order(f) for f in flats], a.long_runs, 0)) if n <= 64 else "-"
    print(f"| {n} | {states} | {arcs} | {cell(batch)} | {cell(loop)} | {loop[0] / batch[0]:.1f}x | {host} | {st['launches']} | "
          f"{100.0 * flags.mean():.1f} % |", flush=True)


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
    print("| items | states | arcs | one top_sort_batch call | loop of n top_sort calls | loop / batch | "
          "host search, interpreted Python (order only) | batch kernel launches | items in the kernel |\n"
          "|---|---|---|---|---|---|---|---|---|", flush=True)
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
