"""optimize of a batch of small lattices: ONE wfst_optimize_batch call against the same items as a loop of n wfst_optimize
calls in the same process, and ONE wfst_tr_sum_batch call against its loop.  Prints two markdown tables
(profiles/optimize_batch_timing.md).

    python tools/optimize_batch_timing.py [--sizes 64 512 4096] [--runs 20] [--warmup 3] [--long-runs 3] [--step-timeout 600]

Inputs: the items of tools/rm_epsilon_batch_timing.py (the random lattice-like DAG acceptors of
tools/determinize_batch_timing.py, 50-500 states, seeded, about a fifth of their arcs relabelled epsilon:epsilon) with
ACCEPTOR | ACYCLIC | INITIAL_ACYCLIC | TOP_SORTED in the word (arcs lead to higher state ids): optimize branches on ACYCLIC
after rm_epsilon, which keeps it only next to TOP_SORTED.  The tr_sum table runs on what optimize hands to that stage: the
results of rm_epsilon_batch over the same items.
Every size of either table is one step, run in a child process of its own under `timeout` (a step that fails or runs out of
time ends the tool: nothing more is started on the device).  A step checks first that the batch results equal the single
calls' (arrays bit for bit, start state, property word), then times with the host clock around the blocking calls, after
`warmup` calls: median [min, max] of `runs` calls of the batch; the loop of single calls is timed over `runs` calls at up to
64 items and over `long-runs` calls, after the one of the equality check, beyond.  Where optimize runs on more than 512
items a call takes minutes: there the two calls of the equality check are the measurement, one each and the first of
their process, and the step says on stderr how far it is.  No ratio is expected in advance: the
comparator is the loop on the same commit in the same run."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from rm_epsilon_batch_timing import cell, lattice_with_epsilons, same, timed  # noqa: E402

ACYCLIC, INITIAL_ACYCLIC, TOP_SORTED = 1 << 35, 1 << 37, 1 << 38
# the lattices' arcs lead to higher state ids: the word may say so, and rm_epsilon keeps ACYCLIC only next to TOP_SORTED
WORD = ACYCLIC | INITIAL_ACYCLIC | TOP_SORTED


def items(n, ctx):
    import rustfst_amd
    from determinize_batch_timing import ACCEPTOR
    rng, eps_rng = np.random.default_rng(4242), np.random.default_rng(2424)
    flats = [dict(lattice_with_epsilons(rng, eps_rng), props=ACCEPTOR | WORD) for _ in range(n)]
    return flats, rustfst_amd.DeviceFst.upload_many(flats, ctx)


def check_equal(outs, singles):
    for k, (o, s) in enumerate(zip(outs, singles)):
        assert same(o.to_flat(), s.to_flat()), f"item {k}: the batch result differs from the single call's"


def note(text):
    """progress on stderr: a step of thousands of items runs for minutes between its table rows"""
    print(f"<!-- {text} -->", file=sys.stderr, flush=True)


def clocked(fn):
    t0 = time.perf_counter()
    res = fn()
    ms = (time.perf_counter() - t0) * 1e3
    return res, (ms, ms, ms, 1)


def step_optimize(n, a):
    import rustfst_amd
    ctx = rustfst_amd.Context(0)
    flats, devs = items(n, ctx)
    arr = rustfst_amd.HandleArray(devs)
    note(f"optimize, {n} items: uploaded")
    (outs, flags), first_batch = clocked(lambda: rustfst_amd.optimize_batch(arr, ctx, return_in_kernel=True))
    st = rustfst_amd.optimize_batch_stats(ctx)
    note(f"optimize, {n} items: the first batch call took {first_batch[0]:.0f} ms")
    singles, first_loop = clocked(lambda: [d.optimize() for d in devs])
    note(f"optimize, {n} items: the first loop took {first_loop[0]:.0f} ms")
    check_equal(outs, singles)
    n_in, n_out = sum(d.num_states for d in devs), sum(o.num_states for o in outs)
    e_in, e_out = sum(len(f["arcs"]) for f in flats), sum(o.num_arcs for o in outs)
    del outs, singles
    if n <= 512:
        batch = timed(lambda: rustfst_amd.optimize_batch(arr, ctx), a.runs, a.warmup)
        loop = timed(lambda: [d.optimize() for d in devs], a.runs if n <= 64 else a.long_runs, a.warmup if n <= 64 else 0)
    else:  # a call takes minutes: the calls of the equality check are the measurement (one each, the first of the process)
        batch, loop = first_batch, first_loop
    launches = " / ".join(str(st["launches"][k]) for k in ("rm_epsilon", "tr_sum", "determinize", "minimize"))
    print(f"| {n} | {n_in} / {n_out} | {e_in} / {e_out} | {cell(batch)} | {cell(loop)} | {loop[0] / batch[0]:.1f}x | "
          f"{launches} | {100.0 * flags.mean():.1f} % |", flush=True)


def step_tr_sum(n, a):
    import rustfst_amd
    ctx = rustfst_amd.Context(0)
    _, lattices = items(n, ctx)
    devs = rustfst_amd.rm_epsilon_batch(rustfst_amd.HandleArray(lattices), ctx)
    arr = rustfst_amd.HandleArray(devs)
    outs, flags = rustfst_amd.tr_sum_batch(arr, ctx, return_in_kernel=True)
    st = rustfst_amd.tr_sum_batch_stats(ctx)
    check_equal(outs, [d.tr_sum() for d in devs])
    e_in, e_out = sum(d.num_arcs for d in devs), sum(o.num_arcs for o in outs)
    del outs
    batch = timed(lambda: rustfst_amd.tr_sum_batch(arr, ctx), a.runs, a.warmup)
    loop = timed(lambda: [d.tr_sum() for d in devs], a.runs if n <= 64 else a.long_runs, a.warmup if n <= 64 else 0)
    print(f"| {n} | {e_in} / {e_out} | {cell(batch)} | {cell(loop)} | {loop[0] / batch[0]:.1f}x | {st['launches']} | "
          f"{100.0 * flags.mean():.1f} % |", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 512, 4096])
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--long-runs", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=600, help="seconds one size may take")
    ap.add_argument("--step", type=int, default=0, help=argparse.SUPPRESS)  # (the child: one size ...
    ap.add_argument("--what", choices=("optimize", "tr_sum"), default="optimize", help=argparse.SUPPRESS)  # ... of one table)
    a = ap.parse_args()
    if a.step:
        return (step_optimize if a.what == "optimize" else step_tr_sum)(a.step, a)
    print("ms per call: median [min, max] (runs); results equal the single calls' at every size\n")
    heads = {"optimize": "| items | states in / out | arcs in / out | one optimize_batch call | loop of n optimize calls | loop / batch | "
                         "batch kernel launches (rm_epsilon / tr_sum / determinize / minimize) | items in the kernels |\n"
                         "|---|---|---|---|---|---|---|---|",
             "tr_sum": "\n| items | arcs in / out | one tr_sum_batch call | loop of n tr_sum calls | loop / batch | batch kernel launches | "
                       "items in the kernel |\n|---|---|---|---|---|---|---|"}
    for what in ("optimize", "tr_sum"):
        print(heads[what], flush=True)
        for n in a.sizes:
            cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", str(n),
                   "--what", what, "--runs", str(a.runs), "--warmup", str(a.warmup), "--long-runs", str(a.long_runs)]
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                print(f"<!-- the {what} step of {n} items ended with status {rc}: stopped -->", flush=True)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
