"""paths on the device against what a user does today.  Prints markdown tables (profiles/paths_timing.md).

    python tools/paths_timing.py [--sizes 64 512 4096] [--runs 10] [--warmup 2] [--step-timeout 420]

Two kinds of input, each step in a child process of its own under `timeout` (a step that fails or runs out of time ends the
tool: nothing more is started on the device):
  n-best    the lattices of tools/compose_batch_timing.py (one grammar), composed by compose_batch and searched by
            shortest_path_batch(nshortest = 10): n handles, at most 10 paths each.  ONE paths_batch call, table download
            included, against today's route: download of every handle, then PathsIterator on the host — the line-by-line
            Python restatement (tests/paths_ref.py, one core) and the same loop compiled (tools/paths_host_loop.cpp, -O2).
            Every timed run gets fresh handles, made outside the timed window: a handle caches its host copy.
  wide      ONE DAG of three fully connected layers of 100 states behind a start state: 10^6 paths of three arcs.
            DeviceFst.paths against download + the two host loops.
The three routes' rows are compared before a line is printed: labels, offsets, order and weight bits.  Host clock around
blocking calls; the first call alone, then median [min, max] of `runs` calls after `warmup` more.  No ratio is expected in
advance."""
import argparse
import ctypes as C
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from rm_epsilon_batch_timing import cell, timed  # noqa: E402

NSHORTEST = 10


def host_loop_lib():
    """tools/paths_host_loop.cpp as a shared object in a temporary folder (None without a host compiler)"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        return None
    so = os.path.join(tempfile.mkdtemp(prefix="paths_host_loop_"), "paths_host_loop.so")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "paths_host_loop.cpp")])
    lib = C.CDLL(so)
    lib.paths_host_run.restype = C.c_void_p
    lib.paths_host_run.argtypes = [C.c_uint32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    lib.paths_host_sizes.argtypes = [C.c_void_p] + [C.POINTER(C.c_uint64)] * 3
    lib.paths_host_copy.argtypes = [C.c_void_p] * 6
    lib.paths_host_free.argtypes = [C.c_void_p]
    return lib


def compiled_rows(lib, flat):
    """(weights, ilabel_off, ilabels, olabel_off, olabels) of one flat FST by the compiled loop"""
    off, arcs, fin = np.ascontiguousarray(flat["offsets"]), np.ascontiguousarray(flat["arcs"]), np.ascontiguousarray(flat["finals"])
    h = lib.paths_host_run(flat["n_states"], -1 if flat["start"] is None else int(flat["start"]), off.ctypes.data, arcs.ctypes.data,
                           fin.ctypes.data, 1 << 26)
    assert h, "the compiled loop did not end"
    try:
        sizes = [C.c_uint64() for _ in range(3)]
        lib.paths_host_sizes(h, *[C.byref(s) for s in sizes])
        P, n_il, n_ol = (int(s.value) for s in sizes)
        w, iloff, il = np.zeros(P, np.float32), np.zeros(P + 1, np.uint64), np.zeros(n_il, np.uint32)
        oloff, ol = np.zeros(P + 1, np.uint64), np.zeros(n_ol, np.uint32)
        lib.paths_host_copy(h, w.ctypes.data, iloff.ctypes.data, il.ctypes.data, oloff.ctypes.data, ol.ctypes.data)
    finally:
        lib.paths_host_free(h)
    return w, iloff, il, oloff, ol


def same_arrays(table, rows):
    w, iloff, il, oloff, ol = rows
    return (table.weights.tobytes() == w.tobytes() and np.array_equal(table.ilabel_off, iloff) and np.array_equal(table.ilabels, il)
            and np.array_equal(table.olabel_off, oloff) and np.array_equal(table.olabels, ol))


def step_nbest(n, a):
    import paths_ref
    import rustfst_amd
    from compose_batch_timing import grammar, relabel
    from determinize_batch_timing import lattice
    ctx = rustfst_amd.Context(0)
    rng = np.random.default_rng(4242)
    g, delta = grammar(rng, a.grammar_states)
    lats = [relabel(rng, lattice(rng), delta) for _ in range(n)]
    dg = rustfst_amd.DeviceFst.upload_many([g], ctx)[0]
    dl = rustfst_amd.HandleArray(rustfst_amd.DeviceFst.upload_many(lats, ctx))
    composed = rustfst_amd.compose_batch(dl, dg, None, ctx)
    cfg = rustfst_amd.ShortestPathConfig(nshortest=NSHORTEST)

    def fresh():
        return rustfst_amd.shortest_path_batch(composed, cfg, ctx)

    lib = host_loop_lib()
    # ---- equality of the three routes
    nbest = fresh()
    table, flags = rustfst_amd.paths_batch(nbest, ctx=ctx, return_in_kernel=True)
    counters = ctx.paths_counters()
    flats = [d.to_flat() for d in nbest]
    for i, f in enumerate(flats):
        part = table.item(i)
        paths_ref.assert_rows_equal(paths_ref.table_rows(part), paths_ref.paths_iter(f), "item %d" % i)
        if lib is not None:
            assert same_arrays(part, compiled_rows(lib, f)), "item %d: the compiled loop differs" % i
    states, arcs = sum(f["n_states"] for f in flats), sum(len(f["arcs"]) for f in flats)

    # ---- timings: fresh handles for every run, made outside the window
    def window(fn, runs, warmup):
        ts = []
        for k in range(warmup + runs):
            hs = fresh()
            ctx.synchronize()
            t0 = time.perf_counter()
            fn(hs)
            if k >= warmup:
                ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        return ts[len(ts) // 2], ts[0], ts[-1], runs

    hs = fresh()
    ctx.synchronize()
    t0 = time.perf_counter()
    rustfst_amd.paths_batch(hs, ctx=ctx)
    first = (time.perf_counter() - t0) * 1e3
    dev = window(lambda hs: rustfst_amd.paths_batch(hs, ctx=ctx), a.runs, a.warmup)
    host_runs = a.runs if n <= 512 else max(1, a.runs // 5)
    down = window(lambda hs: [d.to_flat() for d in hs], host_runs, 1)
    py = window(lambda hs: [paths_ref.paths_iter(d.to_flat()) for d in hs], max(1, host_runs // 3), 0)
    cc = window(lambda hs: [compiled_rows(lib, d.to_flat()) for d in hs], host_runs, 1) if lib is not None else None
    print(f"| {n} n-best results (n = {NSHORTEST}) | {states} / {arcs} | {len(table)} | {first:.3f} | {cell(dev)} | {cell(down)} | "
          f"{cell(py)} | {cell(cc) if cc else 'no host compiler'} | {counters['launches']} | {100.0 * flags.mean():.1f} % | "
          f"{counters['levels']} / {counters['max_path_arcs']} |", flush=True)


def wide_dag(width=100, layers=3):
    from rustfst_amd._lib import TR_DTYPE
    rng = np.random.default_rng(99)
    n = 1 + width * layers
    rows = [[(1 + j % 50, 1 + j % 50, float(rng.integers(0, 64)) / 8, 1 + j) for j in range(width)]]
    for layer in range(layers - 1):
        nxt = 1 + width * (layer + 1)
        for _ in range(width):
            rows.append([(1 + j % 50, 0 if j % 7 == 0 else 1 + j % 50, float(rng.integers(0, 64)) / 8, nxt + j) for j in range(width)])
    rows += [[] for _ in range(width)]
    off = np.zeros(n + 1, np.uint32)
    off[1:] = np.cumsum([len(r) for r in rows])
    arcs = np.array([t for r in rows for t in r], dtype=TR_DTYPE)
    fin = np.full(n, np.inf, np.float32)
    fin[-width:] = (rng.integers(0, 16, width) / 8).astype(np.float32)
    return dict(n_states=n, start=0, offsets=off, arcs=arcs, finals=fin, props=0)


def step_wide(a):
    import paths_ref
    import rustfst_amd
    ctx = rustfst_amd.Context(0)
    f = wide_dag()
    lib = host_loop_lib()

    def fresh():
        return rustfst_amd.DeviceFst.from_arrays(f["n_states"], f["start"], f["offsets"], f["arcs"], f["finals"], f["props"], ctx)

    d = fresh()
    t0 = time.perf_counter()
    table = d.paths(max_paths=1 << 21)
    first = (time.perf_counter() - t0) * 1e3
    counters = ctx.paths_counters()
    if lib is not None:
        assert same_arrays(table, compiled_rows(lib, f)), "the compiled loop differs"
    t0 = time.perf_counter()
    ref = paths_ref.paths_iter(f, max_steps=1 << 26)
    py_ms = (time.perf_counter() - t0) * 1e3
    paths_ref.assert_rows_equal(paths_ref.table_rows(table), ref, "wide")
    dev = timed(lambda: d.paths(max_paths=1 << 21), a.runs, a.warmup)
    ctx_only = timed(lambda: d.count_paths(), a.runs, a.warmup)
    down = timed(lambda: fresh().to_flat(), a.runs, 1)
    cc = timed(lambda: compiled_rows(lib, fresh().to_flat()), max(1, a.runs // 3), 1) if lib is not None else None
    print(f"| one wide DAG | {f['n_states']} / {len(f['arcs'])} | {len(table)} | {first:.3f} | {cell(dev)} | {cell(down)} (upload included) | "
          f"{py_ms:.0f} (1, without the download) | {cell(cc) if cc else 'no host compiler'} | {counters['launches']} | single call | "
          f"{counters['levels']} / {counters['max_path_arcs']} |", flush=True)
    print(f"\ncount_paths of the wide DAG alone: {cell(ctx_only)} ms\n", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 512, 4096])
    ap.add_argument("--grammar-states", type=int, default=3000)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds one step may take")
    ap.add_argument("--no-wide", action="store_true")
    ap.add_argument("--step", type=int, default=0, help=argparse.SUPPRESS)  # (the child: one size; -1: the wide DAG)
    a = ap.parse_args()
    if a.step > 0:
        return step_nbest(a.step, a)
    if a.step < 0:
        return step_wide(a)
    print("ms per call: median [min, max] (runs); the rows of the three routes are equal at every size\n")
    print("| input | states / arcs | paths | device, first call | device, repeated call (table download included) | download alone | "
          "download + PathsIterator restated in Python | download + PathsIterator compiled | launches of the call | items in the kernel | "
          "deepest peel / longest path |\n|---|---|---|---|---|---|---|---|---|---|---|", flush=True)
    steps = list(a.sizes) + ([] if a.no_wide else [-1])
    for n in steps:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", str(n),
               "--runs", str(a.runs), "--warmup", str(a.warmup), "--grammar-states", str(a.grammar_states)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"<!-- the step {n} ended with status {rc}: stopped -->", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
