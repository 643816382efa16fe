"""The one-wavefront path kernels: input families and the n-best routing restatement that more than one module uses."""
import functools
import heapq

import numpy as np

from helpers import _flat

INF = float("inf")
NB_MAX_STATES, NB_MAX_ARCS, NB_MAX_PATHS = 4096, 8192, 64  # the limits of nbest_batch.hip's n-best kernel (include/wfst.h)


def ring_with_chords(rng, n, e, grid, max_w=None):
    """a ring s -> s + 1 mod n plus e - n random chords, eight random final states; weights on the 1/grid grid; the arcs of
    a state sorted by input label"""
    assert e >= n >= 8
    max_w = max_w or (12 if grid <= 4 else 2560)
    rows = [[(int(rng.integers(1, 6)), int(rng.integers(1, 6)), float(rng.integers(0, max_w)) / grid, (s + 1) % n)] for s in range(n)]
    for s in rng.integers(0, n, e - n):
        rows[int(s)].append((int(rng.integers(1, 6)), int(rng.integers(1, 6)), float(rng.integers(0, max_w)) / grid, int(rng.integers(0, n))))
    for r in rows:
        r.sort(key=lambda a: a[0])
    finals = np.full(n, np.inf, dtype=np.float32)
    finals[rng.choice(n, 8, replace=False)] = rng.integers(0, max_w, 8) / grid
    return _flat(n, 0, rows, finals)


def forward_distances(flat):
    """d[s] = the least sum of arc weights over the paths start -> s, Dijkstra over Python floats (arc weights >= 0; a +inf
    arc never improves, -0.0 counts as 0)"""
    n, off, arcs = flat["n_states"], flat["offsets"], flat["arcs"]
    d = [INF] * n
    if flat["start"] is None or flat["start"] < 0 or n == 0:
        return d
    w, nx = arcs["weight"].astype(np.float64).tolist(), arcs["nextstate"].tolist()
    d[flat["start"]] = 0.0
    heap = [(0.0, flat["start"])]
    while heap:
        ds, s = heapq.heappop(heap)
        if ds > d[s]:
            continue
        for k in range(int(off[s]), int(off[s + 1])):
            c = ds + w[k] + 0.0
            if c < d[nx[k]]:
                d[nx[k]] = c
                heapq.heappush(heap, (c, nx[k]))
    return d


def has_start(f):
    return f["start"] is not None and f["start"] >= 0


def n_arcs(f):
    return len(f["arcs"])


def has_negative(f):
    """what the upload works out: some ARC weight < 0 (final weights are not looked at; -0.0 < 0 is false)"""
    return bool((f["arcs"]["weight"] < 0).any())


def tree_capacity(nshortest, max_n):
    return min(16384, max(2048, 2 * nshortest * (max_n + 8)))


def nbest_tree_entries(flat, nshortest, stop_at=1 << 20):
    """The entries the n-best search creates in its tree (shortest_path.rs:409-518 on the reversed FST, as
    shortest_path.rs:139-155 calls it): the start and final state of the output, then one per arc followed backwards and
    one per completed path.  Python's heap orders tied keys by (Some before None, creation) where the reference's own heap
    orders them by its sift order, and keys within 1/1024 are ties there: the count moves a little with that, the margins
    asked of it below do not.  0 when no final state is reachable (the kernel answers that before the search)."""
    n, off, arcs, start = flat["n_states"], flat["offsets"], flat["arcs"], flat["start"]
    d = forward_distances(flat)
    finals = [(s, float(w)) for s, w in enumerate(flat["finals"]) if w != np.inf]
    d0 = min([INF] + [w + d[s] + 0.0 for s, w in finals])
    if not d0 < INF:
        return 0
    into = [[] for _ in range(n)]  # the arcs of the reversed FST: state t + 1 -> s + 1 for every arc s -> t
    src = np.repeat(np.arange(n), np.diff(off.astype(np.int64))).tolist()
    for s, w, t in zip(src, arcs["weight"].astype(np.float64).tolist(), arcs["nextstate"].tolist()):
        into[t].append((s + 1, w))
    d2 = [d0] + d
    tree, seq, r = 2, 0, {}
    heap = [(d2[0], 0, 0, 0, 0.0)]  # (key, None after Some, creation, state of the reversed FST or None, weight so far)
    while heap and tree < stop_at:
        _, _, _, st, w = heapq.heappop(heap)
        idx = 0 if st is None else st + 1
        r[idx] = r.get(idx, 0) + 1
        if st is None and r[idx] == nshortest:
            break
        if r[idx] > nshortest or st is None:
            continue
        out = [(s + 1, fw) for s, fw in finals] if st == 0 else into[st - 1]
        for nxt, aw in out:
            seq, tree = seq + 1, tree + 1
            heapq.heappush(heap, (d2[nxt] + (w + aw + 0.0), 0, seq, nxt, w + aw + 0.0))
        if st == start + 1:  # the reversed FST's only final state: the image of the start state, weight One
            seq, tree = seq + 1, tree + 1
            heapq.heappush(heap, (w, 1, seq, None, w))
    return tree


def nbest_offered(flats, nshortest):
    if nshortest > NB_MAX_PATHS:
        return []
    return [f for f in flats if has_start(f) and 0 < f["n_states"] <= NB_MAX_STATES and n_arcs(f) <= NB_MAX_ARCS and not has_negative(f)]


@functools.lru_cache(maxsize=None)
def _entries(key, nshortest):
    return nbest_tree_entries(_BY_ID[key], nshortest, stop_at=1 << 16)


_BY_ID = {}


def predict_nbest(flats, nshortest, check_margins=True):
    """shortest_path_batch(nshortest > 1): (counters, per offered item whether the search fits T).  With check_margins every
    item's tree must be clear of T: at least 2 x T where it overflows, at most 0.8 x T where it fits."""
    items = nbest_offered(flats, nshortest)
    if not items:
        return dict(nbest_in_kernel=0, nbest_tree_full=0, nbest_out_full=0, nbest_tree_capacity=0)
    T = tree_capacity(nshortest, max(f["n_states"] for f in items))
    full = 0
    for f in items:
        _BY_ID[id(f)] = f
        e = _entries(id(f), nshortest)
        if check_margins:
            assert e >= 2 * T or e <= 0.8 * T, "%d tree entries against T = %d: too close to call" % (e, T)
        full += e > T
    return dict(nbest_in_kernel=len(items) - full, nbest_tree_full=full, nbest_out_full=0, nbest_tree_capacity=T)
