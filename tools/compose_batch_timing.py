"""compose of a batch of small lattices: ONE wfst_compose_batch call against the same pairs as a loop of n wfst_compose calls
in the same process.  Prints markdown tables (profiles/compose_batch_timing.md).

    python tools/compose_batch_timing.py [--sizes 64 512 4096] [--runs 20] [--warmup 3] [--long-runs 3] [--pipeline-max 512] [--step-timeout 600]

Inputs: the random lattice-like DAG acceptors of tools/determinize_batch_timing.py (50-500 states, seeded), relabelled by a
walk through the grammar they are composed with, so that every lattice has paths the grammar accepts, and sorted on output
labels.  Three forms per size:
  one grammar   n lattices against ONE ilabel-sorted grammar of --grammar-states states over 6 labels (n2 = 1);
  n grammars    the pair form: every lattice against a grammar of its own (--pair-grammar-states states);
  pipeline      the one-grammar call followed by top_sort_batch and optimize_batch, against the loop of compose, top_sort
                and optimize per item (up to --pipeline-max items: optimize_batch's share makes a call take seconds).
Every size is one step, run in a child process of its own under `timeout` (a step that fails or runs out of time ends the
tool: nothing more is started on the device).  A step checks first that the batch results equal the single calls' (arrays
bit for bit, start state, property word), then times with the host clock around the blocking calls, after `warmup` calls:
median [min, max] of `runs` calls of the batch; the loops are timed over `runs` calls at up to 64 items and over
`long-runs` calls beyond.  No ratio is expected in advance: the comparator is the loop on the same commit in the same run."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from rm_epsilon_batch_timing import cell, same, timed  # noqa: E402

LABELS = 6


def grammar(rng, n_states):
    """every state final, arcs on 3 of the 6 labels to random states: ilabel-sorted, deterministic.  Returns the FST and its
    transition table (state, label - 1) -> next state or -1"""
    from rustfst_amd import synth
    from rustfst_amd._lib import TR_DTYPE
    per = LABELS // 2
    labels = np.sort(np.argsort(rng.random((n_states, LABELS)), axis=1)[:, :per], axis=1)
    arcs = np.zeros(n_states * per, TR_DTYPE)
    arcs["ilabel"] = arcs["olabel"] = labels.reshape(-1) + 1
    arcs["nextstate"] = rng.integers(0, n_states, len(arcs))
    arcs["weight"] = rng.integers(0, 64, len(arcs)).astype(np.float32) / np.float32(8)
    fin = (rng.integers(0, 16, n_states) / 8).astype(np.float32)
    delta = np.full((n_states, LABELS), -1, np.int64)
    delta[np.repeat(np.arange(n_states), per), labels.reshape(-1)] = arcs["nextstate"]
    f = dict(n_states=n_states, start=0, offsets=np.arange(0, len(arcs) + 1, per, dtype=np.uint32), arcs=arcs, finals=fin,
             props=synth.I_LABEL_SORTED | synth.O_LABEL_SORTED)
    return f, delta


def relabel(rng, lat, delta):
    """the lattice's arcs relabelled by a walk through the grammar: the first arc into a state fixes the grammar state it is
    met in; a later arc takes the label that leads there where the grammar has one (the paths join) and a label the
    grammar state lacks otherwise (that arc matches nothing); then sorted on output labels.  Every lattice state keeps a
    path from the start that the grammar accepts, so the composition is never empty."""
    from rustfst_amd import synth
    n, off, arcs = lat["n_states"], lat["offsets"].astype(np.int64), lat["arcs"].copy()
    at = np.full(n, -1, np.int64)
    at[0] = 0
    for s in range(n):
        if at[s] < 0:  # (no arc leads here: the generator leaves a few such states)
            continue
        have, lack = np.flatnonzero(delta[at[s]] >= 0), np.flatnonzero(delta[at[s]] < 0)
        for k in range(off[s], off[s + 1]):
            t = int(arcs["nextstate"][k])
            if at[t] < 0:
                l = int(rng.choice(have))
                at[t] = delta[at[s], l]
            else:
                hit = np.flatnonzero(delta[at[s]] == at[t])
                l = int(hit[0]) if len(hit) else int(rng.choice(lack))
            arcs["ilabel"][k] = arcs["olabel"][k] = l + 1
        row = arcs[off[s]:off[s + 1]]
        arcs[off[s]:off[s + 1]] = row[np.argsort(row["olabel"], kind="stable")]
    return dict(lat, arcs=arcs, props=lat["props"] | synth.O_LABEL_SORTED)


def step(n, a):
    import rustfst_amd
    from determinize_batch_timing import lattice
    ctx = rustfst_amd.Context(0)
    rng = np.random.default_rng(4242)
    g, delta = grammar(rng, a.grammar_states)
    raw = [lattice(rng) for _ in range(n)]
    lats = [relabel(rng, lat, delta) for lat in raw]
    gds = [grammar(rng, a.pair_grammar_states) for _ in range(n)]
    gs = [gk for gk, _ in gds]
    pair_lats = [relabel(rng, lat, dk) for lat, (_, dk) in zip(raw, gds)]
    dg = rustfst_amd.DeviceFst.upload_many([g], ctx)[0]
    dl = rustfst_amd.HandleArray(rustfst_amd.DeviceFst.upload_many(lats, ctx))
    dgs = rustfst_amd.HandleArray(rustfst_amd.DeviceFst.upload_many(gs, ctx))
    dpl = rustfst_amd.HandleArray(rustfst_amd.DeviceFst.upload_many(pair_lats, ctx))
    loop_runs, loop_warm = (a.runs, a.warmup) if n <= 64 else (a.long_runs, 0)

    def check(outs, singles, what):
        for k, (o, s) in enumerate(zip(outs, singles)):
            assert same(o.to_flat(), s.to_flat()), f"{what} item {k}: the batch result differs from the single call's"

    # ---- one grammar
    outs, flags = rustfst_amd.compose_batch(dl, dg, None, ctx, return_in_kernel=True)
    st = rustfst_amd.compose_batch_stats(ctx)
    singles = [d.compose(dg) for d in dl._keep]
    check(outs, singles, "one grammar")
    states, arcs = sum(o.num_states for o in outs), sum(o.num_arcs for o in outs)
    nonempty = sum(o.num_states > 0 for o in outs)
    del outs, singles
    batch = timed(lambda: rustfst_amd.compose_batch(dl, dg, None, ctx), a.runs, a.warmup)
    loop = timed(lambda: [d.compose(dg) for d in dl._keep], loop_runs, loop_warm)
    print(f"| one grammar ({a.grammar_states} states) | {n} | {states} / {arcs} ({nonempty} non-empty) | {cell(batch)} | {cell(loop)} | "
          f"{loop[0] / batch[0]:.1f}x | {st} | {100.0 * flags.mean():.1f} % |", flush=True)
    # ---- n grammars
    outs, flags = rustfst_amd.compose_batch(dpl, dgs, None, ctx, return_in_kernel=True)
    st = rustfst_amd.compose_batch_stats(ctx)
    singles = [d.compose(h) for d, h in zip(dpl._keep, dgs._keep)]
    check(outs, singles, "n grammars")
    states, arcs = sum(o.num_states for o in outs), sum(o.num_arcs for o in outs)
    nonempty = sum(o.num_states > 0 for o in outs)
    del outs, singles
    batch = timed(lambda: rustfst_amd.compose_batch(dpl, dgs, None, ctx), a.runs, a.warmup)
    loop = timed(lambda: [d.compose(h) for d, h in zip(dpl._keep, dgs._keep)], loop_runs, loop_warm)
    print(f"| n grammars ({a.pair_grammar_states} states each) | {n} | {states} / {arcs} ({nonempty} non-empty) | {cell(batch)} | {cell(loop)} | "
          f"{loop[0] / batch[0]:.1f}x | {st} | {100.0 * flags.mean():.1f} % |", flush=True)

    # ---- pipeline
    if n > a.pipeline_max:
        print(f"| compose_batch, top_sort_batch, optimize_batch | {n} | - | not run (--pipeline-max {a.pipeline_max}) | - | - | - | - |", flush=True)
        return

    def pipeline():
        return rustfst_amd.optimize_batch(rustfst_amd.top_sort_batch(rustfst_amd.compose_batch(dl, dg, None, ctx), ctx), ctx)

    def pipeline_loop():
        return [d.compose(dg).top_sort().optimize() for d in dl._keep]
    check(pipeline(), pipeline_loop(), "pipeline")
    batch = timed(pipeline, loop_runs, loop_warm)  # (optimize_batch's share makes this call as long as a loop)
    loop = timed(pipeline_loop, loop_runs, loop_warm)
    print(f"| compose_batch, top_sort_batch, optimize_batch | {n} | - | {cell(batch)} | {cell(loop)} | {loop[0] / batch[0]:.1f}x | - | - |",
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 512, 4096])
    ap.add_argument("--grammar-states", type=int, default=3000)
    ap.add_argument("--pair-grammar-states", type=int, default=200)
    ap.add_argument("--pipeline-max", type=int, default=512, help="largest size at which the pipeline rows are run")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--long-runs", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=600, help="seconds one size may take")
    ap.add_argument("--step", type=int, default=0, help=argparse.SUPPRESS)  # (the child: one size)
    a = ap.parse_args()
    if a.step:
        return step(a.step, a)
    print("ms per call: median [min, max] (runs); results equal the single calls' at every size\n")
    print("| form | items | composed states / arcs | one call | loop of single calls | loop / batch | counters of the call | "
          "items in the kernel |\n|---|---|---|---|---|---|---|---|", flush=True)
    for n in a.sizes:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", str(n),
               "--runs", str(a.runs), "--warmup", str(a.warmup), "--long-runs", str(a.long_runs),
               "--pipeline-max", str(a.pipeline_max), "--grammar-states", str(a.grammar_states), "--pair-grammar-states", str(a.pair_grammar_states)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"<!-- the step of {n} items ended with status {rc}: stopped -->", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
