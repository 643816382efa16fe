"""minimize on three shapes: the closed-form blow-up of a small minimal DAG (>= 1 M states, wide heights), a deep thin
chain (20 000 heights of two states) and a determinized lattice.  First call and median of repeated calls, wall clock
around the synchronous call, then the Python restatement of oracle/model/minimize.py on the same host where it finishes
within a minute (it is a literal sequential restatement, not an optimised CPU implementation).
python tools/minimize_timing.py [blow_up_states] [chain_heights]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import rustfst_amd
from rustfst_amd._lib import TR_DTYPE
from oracle.model import ACCEPTOR, minimize_ref
from minimize_cases import blow_up, closed_form_base  # the inputs the tests use

STATES = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
HEIGHTS = int(sys.argv[2]) if len(sys.argv) > 2 else 20_000
REF_LIMIT = 200_000  # states up to which the restatement is timed
ctx = rustfst_amd.default_context()


def dev(f):
    return rustfst_amd.DeviceFst.from_arrays(f["n_states"], f["start"], f["offsets"], f["arcs"], f["finals"], f["props"], ctx)


def timed(fn, reps=5):
    t0 = time.perf_counter(); out = fn(); ctx.synchronize(); first = (time.perf_counter() - t0) * 1e3
    rep = []
    for _ in range(reps):
        t0 = time.perf_counter(); out = fn(); ctx.synchronize(); rep.append((time.perf_counter() - t0) * 1e3)
    return first, float(np.median(rep)), out


def thin_chain(h):
    """h heights of two states: state 2i and 2i+1 both go to 2i+2 (label 1) and 2i+3 (label 2) with weights that
    become equal after pushing, so the pair of every height merges"""
    n = 2 * h + 1
    arcs = np.zeros(4 * (h - 1) + 2, dtype=TR_DTYPE)
    s = np.repeat(np.arange(2 * (h - 1)), 2)
    k = np.arange(len(s))
    arcs["ilabel"][:len(s)] = arcs["olabel"][:len(s)] = 1 + k % 2
    arcs["weight"][:len(s)] = (s % 2) * 1.0 + (k % 2) * 2.0
    arcs["nextstate"][:len(s)] = (s // 2) * 2 + 2 + k % 2
    arcs[len(s):] = [(1, 1, 0.0, n - 1), (1, 1, 3.0, n - 1)]
    off = np.zeros(n + 1, dtype=np.uint32)
    off[1:2 * (h - 1) + 1] = 2 * np.arange(1, 2 * (h - 1) + 1)
    off[2 * (h - 1) + 1:] = [len(s) + 1, len(s) + 2, len(s) + 2]
    fin = np.full(n, np.inf, dtype=np.float32)
    fin[n - 1] = 0.0
    return dict(n_states=n, start=0, offsets=off, arcs=arcs, finals=fin, props=ACCEPTOR)


def report(name, flat):
    d = dev(flat)
    first, rep, out = timed(lambda: d.minimize())
    line = (f"{name:12s} in {flat['n_states']:>8d} states / {len(flat['arcs']):>9d} arcs -> {out.num_states:>8d} states"
            f"   first {first:9.2f} ms   repeated {rep:9.2f} ms")
    if flat["n_states"] <= REF_LIMIT:
        t0 = time.perf_counter(); r = minimize_ref(flat); dt = (time.perf_counter() - t0) * 1e3
        assert r["n_states"] == out.num_states
        line += f"   restatement {dt:9.2f} ms"
    print(line, flush=True)


rng = np.random.default_rng(33)
m = closed_form_base(rng)
report("blow-up", blow_up(rng, m, STATES // m["n_states"] + 1))
report("thin chain", thin_chain(HEIGHTS))
from rustfst_amd import synth
t = synth.make_transducer(1_000_000)
accs = synth.make_acceptors(t, 1, 25, seed0=1000)
lat = dev(accs[0]).compose(dev(t)).project(rustfst_amd.ProjectType.PROJECT_OUTPUT).determinize()
report("det. lattice", lat.to_flat())
