"""rm_epsilon of a batch of small lattices: ONE wfst_rm_epsilon_batch call against the same items as a loop of n wfst_rm_epsilon
calls in the same process.  Prints a markdown table (profiles/rm_epsilon_batch_timing.md).

    python tools/rm_epsilon_batch_timing.py [--sizes 64 512 4096] [--runs 20] [--warmup 3] [--long-runs 3] [--step-timeout 600]

Inputs: the random lattice-like DAG acceptors of tools/determinize_batch_timing.py (50-500 states, seeded) with about a
fifth of their arcs relabelled epsilon:epsilon by a seeded generator: what union_list / project hand to rm_epsilon.
Every size is one step, run in a child process of its own under `timeout` (a step that fails or runs out of time ends the
tool: nothing more is started on the device).  A step checks first that the batch results equal the single calls' (arrays
bit for bit, start state, property word), then times with the host clock around the blocking calls, after `warmup`
calls: median [min, max] of `runs` calls of the batch; the loop of single calls takes seconds from 512 items on and is
timed over `long-runs` calls after the one of the equality check.  The table also gives the launches of the batch kernel
and the share of the items it finished itself (in_kernel == 1)."""
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


def lattice_with_epsilons(rng, eps_rng):
    """determinize_batch_timing's lattice with about a fifth of its arcs relabelled 0:0 (the word keeps ACCEPTOR only: the
    label order is gone)"""
    from determinize_batch_timing import ACCEPTOR, lattice
    f = lattice(rng)
    eps = eps_rng.random(len(f["arcs"])) < 0.2
    f["arcs"]["ilabel"][eps] = 0
    f["arcs"]["olabel"][eps] = 0
    f["props"] = ACCEPTOR
    return f


def step(n, a):
    import rustfst_amd
    rng, eps_rng = np.random.default_rng(4242), np.random.default_rng(2424)
    flats = [lattice_with_epsilons(rng, eps_rng) for _ in range(n)]
    ctx = rustfst_amd.Context(0)
    devs = rustfst_amd.DeviceFst.upload_many(flats, ctx)
    arr = rustfst_amd.HandleArray(devs)
    outs, flags = rustfst_amd.rm_epsilon_batch(arr, ctx, return_in_kernel=True)
    st = rustfst_amd.rm_epsilon_batch_stats(ctx)
    singles = [d.rm_epsilon() for d in devs]
    for k, (o, s) in enumerate(zip(outs, singles)):
        assert same(o.to_flat(), s.to_flat()), f"item {k}: the batch result differs from the single call's"
    n_in, n_out = sum(d.num_states for d in devs), sum(o.num_states for o in outs)
    e_in, e_out = sum(len(f["arcs"]) for f in flats), sum(o.num_arcs for o in outs)
    del outs, singles
    batch = timed(lambda: rustfst_amd.rm_epsilon_batch(arr, ctx), a.runs, a.warmup)
    loop = timed(lambda: [d.rm_epsilon() for d in devs], a.runs if n <= 64 else a.long_runs, a.warmup if n <= 64 else 0)
    print(f"| {n} | {n_in} / {n_out} | {e_in} / {e_out} | {cell(batch)} | {cell(loop)} | {loop[0] / batch[0]:.1f}x | "
          f"{st['launches']} | {100.0 * flags.mean():.1f} % |", flush=True)


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
    print("| items | states in / out | arcs in / out | one rm_epsilon_batch call | loop of n rm_epsilon calls | loop / batch | "
          "batch kernel launches | items in the kernel |")
    print("|---|---|---|---|---|---|---|---|", flush=True)
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
