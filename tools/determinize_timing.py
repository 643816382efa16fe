"""determinize on three shapes: the twin-copy graph (2n states, wide levels), a chain of diamonds (deep and thin) and a
lattice (one acceptor o T, projected to the outputs).  First call and median of repeated calls, wall clock around the
synchronous call, then the oracle's single-thread time on the same host.
python tools/determinize_timing.py [twin_n] [diamond_levels]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import rustfst_amd
from rustfst_amd import synth
from oracle import oracle_py
from inputs import diamond_chain, twin_copy  # the inputs the tests use

TWIN = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
DIAMONDS = int(sys.argv[2]) if len(sys.argv) > 2 else 20_000
ctx = rustfst_amd.default_context()


def dev(f):
    return rustfst_amd.DeviceFst.from_arrays(f["n_states"], f["start"], f["offsets"], f["arcs"], f["finals"], f["props"], ctx)


def timed(fn, reps=5):
    t0 = time.perf_counter(); out = fn(); ctx.synchronize(); first = (time.perf_counter() - t0) * 1e3
    rep = []
    for _ in range(reps):
        t0 = time.perf_counter(); out = fn(); ctx.synchronize(); rep.append((time.perf_counter() - t0) * 1e3)
    return first, float(np.median(rep)), out


def report(name, flat, oracle=True):
    d = dev(flat)
    first, rep, out = timed(lambda: d.determinize())
    line = (f"{name:10s} in {flat['n_states']:>8d} states / {len(flat['arcs']):>9d} arcs -> {out.num_states:>8d} states"
            f"   first {first:9.2f} ms   repeated {rep:9.2f} ms")
    if oracle:
        o = oracle_py.OracleFst.from_flat(flat["n_states"], flat["start"], flat["offsets"], flat["arcs"], flat["finals"],
                                          flat["props"])
        t0 = time.perf_counter(); o.determinize_fsa(); line += f"   oracle {(time.perf_counter() - t0) * 1e3:9.2f} ms"
    print(line, flush=True)


report("twin-copy", twin_copy(TWIN)[0])
report("diamonds", diamond_chain(DIAMONDS))
t = synth.make_transducer(1_000_000)
acc = synth.make_acceptors(t, 1, 25, seed0=1000)[0]
lat = dev(acc).compose(dev(t)).project(rustfst_amd.ProjectType.PROJECT_OUTPUT).to_flat()
report("lattice", lat)
