"""The reference's PathsIterator (rustfst/src/fst_traits/paths_iterator.rs:24-62) restated line by line over a flat FST,
with FstPath::add_to_path / add_weight (fst_path.rs:35-50) and TropicalWeight's times_assign (tropical_weight.rs:60-70) in
np.float32.  What the device tables are compared with, bit for bit.  A test module is nobody's library: this one is."""
from collections import deque

import numpy as np

F32 = np.float32
INF = F32(np.inf)


def times(a, b):
    """times_assign: inf absorbs, else the f32 sum"""
    if a == INF:
        return a
    if b == INF:
        return b
    return F32(a + b)


def paths_iter(flat, max_steps=2_000_000):
    """[(ilabels, olabels, weight)] in the order the iterator yields them.  max_steps bounds the pops: the reference does
    not return on a cycle that the start state reaches, this restatement raises instead."""
    out = []
    queue = deque()
    if flat["start"] is not None and flat["n_states"]:
        queue.append((int(flat["start"]), ((), (), F32(0.0))))  # FstPath::default(): no labels, W::one()
    off, arcs, fin = flat["offsets"], flat["arcs"], flat["finals"]
    steps = 0
    while queue:
        steps += 1
        if steps > max_steps:
            raise RuntimeError("paths_iter: the queue does not drain")
        state_id, (il, ol, w) = queue.popleft()
        for tr in arcs[int(off[state_id]):int(off[state_id + 1])]:
            # add_to_path
            n_il = il + (int(tr["ilabel"]),) if int(tr["ilabel"]) != 0 else il
            n_ol = ol + (int(tr["olabel"]),) if int(tr["olabel"]) != 0 else ol
            queue.append((int(tr["nextstate"]), (n_il, n_ol, times(w, F32(tr["weight"])))))
        final_weight = fin[state_id]
        if not (np.isinf(final_weight) and final_weight > 0):  # Some(final_weight): +inf is the flat form's None
            out.append((il, ol, times(w, F32(final_weight))))  # add_weight
    return out


def table_rows(table):
    """the rows of a rustfst_amd.PathTable in the same form, from its arrays"""
    rows = []
    for k in range(len(table)):
        rows.append((tuple(int(x) for x in table.ilabels[int(table.ilabel_off[k]):int(table.ilabel_off[k + 1])]),
                     tuple(int(x) for x in table.olabels[int(table.olabel_off[k]):int(table.olabel_off[k + 1])]),
                     F32(table.weights[k])))
    return rows


def assert_rows_equal(got, exp, what=""):
    """labels, order and weight bits"""
    assert len(got) == len(exp), f"{what}: {len(got)} paths, the reference yields {len(exp)}"
    for k, (g, e) in enumerate(zip(got, exp)):
        assert g[0] == e[0] and g[1] == e[1], f"{what}: path {k}: labels {g[:2]} != {e[:2]}"
        assert F32(g[2]).view(np.uint32) == F32(e[2]).view(np.uint32), f"{what}: path {k}: weight {g[2]!r} != {e[2]!r}"
