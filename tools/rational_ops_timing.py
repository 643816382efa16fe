"""union_list and closure on the shapes of profiles/rational_ops_timing.md.  First call and median of repeated calls, wall
clock around the synchronous call, operands resident on the device (uploaded with one wfst_fst_upload_many).
  1. union_list of 64 / 512 / 4096 path FSTs (strings of 8-40 arcs): the hypotheses of a decoding batch
  2. union_list of 512 random lattice-like DAGs of 50-500 states
  3. closure(union_list(...)) of the same lists
Each as ONE list call and as n - 1 pairwise calls (the left fold, every step a new handle).  Next to the absolute times: the
bytes the result is made of, 32 E + 12 N (an arc read and written, per state an offset read and written and a final weight),
over the time, as a share of the 8 TB/s HBM peak (for the lattices; the path lists are too small for the figure to mean anything).  Nothing here is a gate: the project has no compiled comparator for these
operations.
python tools/rational_ops_timing.py [repetitions]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import rustfst_amd
from rustfst_amd._lib import TR_DTYPE

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
PEAK = 8e12  # bytes / s
ACYCLIC, INITIAL_ACYCLIC = 1 << 35, 1 << 37
ctx = rustfst_amd.default_context()


def path_fst(rng):
    k = int(rng.integers(8, 41))
    arcs = np.zeros(k, dtype=TR_DTYPE)
    arcs["ilabel"] = arcs["olabel"] = rng.integers(1, 5000, k)
    arcs["weight"] = rng.integers(0, 64, k) / 8
    arcs["nextstate"] = np.arange(1, k + 1)
    fin = np.full(k + 1, np.inf, dtype=np.float32)
    fin[k] = 0.0
    return dict(n_states=k + 1, start=0, offsets=np.minimum(np.arange(k + 2), k).astype(np.uint32), arcs=arcs, finals=fin)


def lattice_fst(rng):
    n = int(rng.integers(50, 501))
    deg = np.minimum(rng.integers(1, 5, n), n - 1 - np.arange(n))
    off = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint32)
    src = np.repeat(np.arange(n), deg)
    arcs = np.zeros(int(off[-1]), dtype=TR_DTYPE)
    arcs["ilabel"] = arcs["olabel"] = rng.integers(1, 5000, len(arcs))
    arcs["weight"] = rng.integers(0, 64, len(arcs)) / 8
    arcs["nextstate"] = src + 1 + rng.integers(0, 8, len(arcs)) % (n - 1 - src)
    fin = np.full(n, np.inf, dtype=np.float32)
    fin[n - 1] = 0.0
    return dict(n_states=n, start=0, offsets=off, arcs=arcs, finals=fin)


def upload_many(flats):
    return rustfst_amd.DeviceFst.upload_many([dict(f, props=ACYCLIC | INITIAL_ACYCLIC) for f in flats], ctx)


def timed(fn):
    times = []
    out = None
    for _ in range(REPS + 1):
        ctx.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ctx.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return times[0], float(np.median(times[1:])), out


def pairwise(handles):
    acc = handles[0]
    for h in handles[1:]:
        acc = acc.union(h)
    return acc


def report(name, handles, bandwidth=False):
    arr = rustfst_amd.HandleArray(handles)
    first, rep, u = timed(lambda: rustfst_amd.union_list(arr))
    n_states, n_arcs = u.num_states, u.num_arcs
    model = 32 * n_arcs + 12 * n_states
    pfirst, prep, _ = timed(lambda: pairwise(handles))
    cfirst, crep, _ = timed(lambda: rustfst_amd.union_list(arr).closure(rustfst_amd.ClosureType.CLOSURE_STAR))

    def share(ms):
        return 100.0 * model / (ms * 1e-3) / PEAK
    print(f"{name}: result {n_states} states / {n_arcs} arcs, model {model / 1e6:.3f} MB")
    tail = f"  ({share(rep):6.3f} % of peak)" if bandwidth else ""  # (kilobyte-sized results: launch latency, no bandwidth figure)
    print(f"  union_list, one call          first {first:9.3f} ms  repeated {rep:9.3f} ms{tail}")
    print(f"  union, {len(handles) - 1:5d} pairwise calls  first {pfirst:9.3f} ms  repeated {prep:9.3f} ms  ({rep and prep / rep:8.1f} x the list call)")
    print(f"  closure(union_list)           first {cfirst:9.3f} ms  repeated {crep:9.3f} ms")
    qfirst, qrep, _ = timed(lambda: pairwise(handles).closure(rustfst_amd.ClosureType.CLOSURE_STAR))
    print(f"  closure(pairwise unions)      first {qfirst:9.3f} ms  repeated {qrep:9.3f} ms")


def main():
    rng = np.random.default_rng(18)
    for n in (64, 512, 4096):
        report(f"{n} path FSTs", upload_many([path_fst(rng) for _ in range(n)]))
    report("512 lattices of 50-500 states", upload_many([lattice_fst(rng) for _ in range(512)]), bandwidth=True)


if __name__ == "__main__":
    main()
