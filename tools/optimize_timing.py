"""tr_sum and optimize on the shapes of profiles/optimize_timing.md.  First call and median of repeated calls, wall clock
around the synchronous call.
  1. tr_sum / tr_unique of the benchmark transducer (1 M states / ~10 M arcs) and of a copy with every arc duplicated;
     yardstick: the device tr_sort of the same arcs (a fresh upload per repetition: tr_sort works in place and returns at
     once on a sorted handle)
  2. optimize of a wide acyclic input: the twin-copy construction of tests/inputs.py on a layered DAG (twin_copy
     itself sits on the cyclic benchmark transducer), with parallel and eps:eps arcs added, as an acceptor and as the same
     machine with pair labels; yardstick: the separately timed stages on handles
  3. optimize of one deep, thin lattice (diamond_chain)
python tools/optimize_timing.py [transducer_states] [layer_width] [chain_levels]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import rustfst_amd
from rustfst_amd import synth
from rustfst_amd._lib import TR_DTYPE
from oracle.model import ACCEPTOR, ACYCLIC, INITIAL_ACYCLIC, NO_EPSILONS, TOP_SORTED
from inputs import diamond_chain  # the input the tests use

T_STATES = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
WIDTH = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000
LEVELS = int(sys.argv[3]) if len(sys.argv) > 3 else 5_000
ctx = rustfst_amd.default_context()


def dev(f):
    return rustfst_amd.DeviceFst.from_arrays(f["n_states"], f["start"], f["offsets"], f["arcs"], f["finals"], f["props"], ctx)


def timed(fn, reps=5, setup=None):
    times = []
    out = None
    for _ in range(reps + 1):
        arg = setup() if setup else None
        ctx.synchronize()
        t0 = time.perf_counter()
        out = fn(arg) if setup else fn()
        ctx.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return times[0], float(np.median(times[1:])), out


def duplicated(flat):
    off = flat["offsets"].astype(np.int64)
    deg = np.diff(off)
    src = np.repeat(np.arange(flat["n_states"]), deg)
    order = np.argsort(np.concatenate([src, src]), kind="stable")
    return dict(flat, offsets=(2 * off).astype(np.uint32), arcs=np.concatenate([flat["arcs"], flat["arcs"]])[order], props=0)


def layered_twin(layers, width, fanout=8, seed=5):
    """D: `layers` layers of `width` states, every state with `fanout` arcs (labels 1..fanout, integer weights) into random
    states of the next layer, the last layer final.  N as in twin_copy: every state has a copy, and both carry, per arc
    (a, w, r) of D, (a, w, r) and (a, w + 0.5, copy of r); det(N) has D's states.  State (layer l, copy c, i) has id
    l * 2 * width + c * width + i: every arc goes to a higher id (TOP_SORTED)."""
    rng = np.random.default_rng(seed)
    inner = (layers - 1) * width  # D states with arcs, in (layer, i) order
    src = np.repeat(np.arange(inner), fanout)
    da = np.zeros(inner * fanout, TR_DTYPE)
    da["ilabel"] = da["olabel"] = np.tile(np.arange(1, fanout + 1), inner)
    da["weight"] = rng.integers(0, 4, len(da)).astype(np.float32)
    da["nextstate"] = (src // width + 1) * 2 * width + rng.integers(0, width, len(da))  # the first copy of the target
    one = np.repeat(da, 2)
    one["weight"][1::2] += np.float32(0.5)
    one["nextstate"][1::2] += width
    # per layer: the arcs of its `width` states, once for each copy
    per_layer = one.reshape(layers - 1, width * 2 * fanout)
    arcs = np.concatenate([per_layer, per_layer], axis=1).reshape(-1)
    n = 2 * layers * width
    deg = np.concatenate([np.full(2 * inner, 2 * fanout), np.zeros(2 * width, np.int64)])
    off = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint32)
    fin = np.full(n, np.inf, np.float32)
    fin[n - 2 * width:] = 0.0
    return dict(n_states=n, start=0, offsets=off, arcs=arcs, finals=fin, props=0)


def with_eps_and_parallel(flat, width, seed=1):
    """layered_twin's N with work for rm_epsilon and tr_sum: every 8th first-copy state gains an eps:eps arc (weight 1) to its
    own copy, whose arcs rm_epsilon then adds to it as parallel arcs of the state's own; every 4th state a copy of its first
    arc (weight + 1).  Both kinds of new arcs go to higher ids, like the old ones."""
    rng = np.random.default_rng(seed)
    off = flat["offsets"].astype(np.int64)
    n = flat["n_states"]
    ids = np.arange(n)
    has = np.diff(off) > 0
    first = flat["arcs"][np.minimum(off[:-1], len(flat["arcs"]) - 1)]
    eps = has & ((ids // width) % 2 == 0) & (rng.random(n) < 0.125)
    par = has & (rng.random(n) < 0.25)
    e = np.zeros(int(eps.sum()), TR_DTYPE); e["weight"] = 1.0; e["nextstate"] = ids[eps] + width
    p = first[par].copy(); p["weight"] += np.float32(1.0)
    src = np.concatenate([np.repeat(ids, np.diff(off)), ids[eps], ids[par]])
    arcs = np.concatenate([flat["arcs"], e, p])
    order = np.argsort(src, kind="stable")
    noff = np.zeros(n + 1, np.int64)
    np.add.at(noff, src + 1, 1)
    return dict(flat, offsets=np.cumsum(noff).astype(np.uint32), arcs=arcs[order])


def pair_labels(flat):
    """the same machine as a transducer: olabel = 3 * ilabel + (nextstate mod 3), never 0"""
    arcs = flat["arcs"].copy()
    nz = arcs["ilabel"] != 0
    arcs["olabel"][nz] = 3 * arcs["ilabel"][nz] + arcs["nextstate"][nz] % 3 + 1
    return dict(flat, arcs=arcs, props=flat["props"] & ~ACCEPTOR)


def report_arc_lists(name, flat):
    d = dev(flat)
    for op in ("tr_sum", "tr_unique"):
        first, rep, out = timed(getattr(d, op))
        print(f"{name:12s} {op:9s} {flat['n_states']:>8d} states / {len(flat['arcs']):>9d} arcs -> {out.num_arcs:>9d} arcs"
              f"   first {first:8.2f} ms   repeated {rep:8.2f} ms", flush=True)
    first, rep, _ = timed(lambda h: h.tr_sort(True), setup=lambda: dev(dict(flat, props=0)))
    print(f"{name:12s} {'tr_sort':9s} (yardstick, fresh upload outside the clock)   first {first:8.2f} ms   repeated {rep:8.2f} ms", flush=True)


def report_optimize(name, flat, acceptor):
    d = dev(flat)
    first, rep, out = timed(d.optimize, reps=3)
    print(f"{name:14s} optimize {flat['n_states']:>8d} states / {len(flat['arcs']):>8d} arcs -> {out.num_states:>8d} states / "
          f"{out.num_arcs:>8d} arcs   first {first:9.2f} ms   repeated {rep:9.2f} ms", flush=True)
    if not acceptor:
        return  # the encode / decode stages have no public handle: only the acceptor's stages can be timed one by one
    stages, cur = [], d
    for op in ("rm_epsilon", "tr_sum", "determinize", "minimize"):
        if op == "rm_epsilon" and flat["props"] & NO_EPSILONS:
            continue  # optimize skips it as well
        _, t, cur = timed(getattr(cur, op), reps=3)
        stages.append((op, t))
    assert cur.num_states == out.num_states
    print(f"{'':14s} stages   " + "   ".join(f"{op} {t:.2f} ms" for op, t in stages) + f"   sum {sum(t for _, t in stages):.2f} ms",
          flush=True)


t = synth.make_transducer(T_STATES)
report_arc_lists("transducer", t)
report_arc_lists("duplicated", duplicated(t))
word = ACYCLIC | INITIAL_ACYCLIC
wide = with_eps_and_parallel(dict(layered_twin(10, WIDTH), props=ACCEPTOR | word | TOP_SORTED), WIDTH)
report_optimize("wide acceptor", wide, True)
report_optimize("wide pairs", pair_labels(wide), False)
chain = diamond_chain(LEVELS)
report_optimize("thin chain", dict(chain, props=ACCEPTOR | word | TOP_SORTED | NO_EPSILONS), True)
