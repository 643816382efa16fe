"""The two forms the restatements work on: the rows form (dict(rows=[[[il, ol, w, ns], ...], ...], finals=[w | None],
start, props), the shape of a VectorFst) and the flat CSR form the oracle and the device exchange; the facts of a
graph that rustfst decides by depth-first search, and compute_fst_properties."""
import copy

import numpy as np
from ..oracle_py import TR_DTYPE

from .weight import F32, INF, is_one, is_zero
from .props import (ACCEPTOR, ALL, CYCLIC, DFS_BITS, EPSILONS, INITIAL_ACYCLIC, I_DETERMINISTIC, I_EPSILONS,
                    I_LABEL_SORTED, NOT_ACCEPTOR, NOT_I_DETERMINISTIC, NOT_I_LABEL_SORTED, NOT_O_LABEL_SORTED,
                    NOT_STRING, NOT_TOP_SORTED, NO_EPSILONS, NO_I_EPSILONS, NO_O_EPSILONS, O_DETERMINISTIC, O_EPSILONS,
                    O_LABEL_SORTED, STRING, TOP_SORTED, UNWEIGHTED, UNWEIGHTED_CYCLES, WEIGHTED, WEIGHTED_CYCLES,
                    dfs_bits, known, p_add_state, p_add_tr, p_set_final, p_set_start)


# ---------------------------------------------------------------- graph facts (what SccVisitor's DFS decides)
def csr_next(flat):
    return np.asarray(flat["offsets"], dtype=np.int64), np.asarray(flat["arcs"]["nextstate"], dtype=np.int64)


def reach(n, off, nxt, seeds, mark_seeds=True):
    """states reachable from `seeds` (vectorised frontier search); the seeds count only when mark_seeds"""
    vis = np.zeros(n, dtype=bool)
    fr = np.asarray(seeds, dtype=np.int64)
    if mark_seeds:
        vis[fr] = True
    while fr.size:
        cnt = off[fr + 1] - off[fr]
        idx = np.repeat(off[fr] - np.cumsum(np.r_[0, cnt[:-1]]), cnt) + np.arange(cnt.sum())
        t = np.unique(nxt[idx])
        t = t[~vis[t]]
        vis[t] = True
        fr = t
    return vis


def transpose(n, off, nxt):
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(off))
    order = np.argsort(nxt, kind="stable")
    roff = np.zeros(n + 1, dtype=np.int64)
    np.add.at(roff, nxt + 1, 1)
    return np.cumsum(roff), src[order]


def graph_facts(flat):
    """(accessible, coaccessible, cyclic, initial_cyclic) of the graph: every state reachable from the start, every state
    reaches a final state, a cycle anywhere, the start on a cycle — the four DFS pairs compute_fst_properties fills in
    (visitors/scc_visitors.rs: a new DFS tree for an unreachable state, back arcs, back arcs into the start, SCCs without
    a final state)."""
    n, s0 = flat["n_states"], flat["start"]
    off, nxt = csr_next(flat)
    accessible = bool(reach(n, off, nxt, [s0]).all())
    roff, rsrc = transpose(n, off, nxt)
    finals = np.nonzero(np.isfinite(flat["finals"]))[0]
    coaccessible = bool(reach(n, roff, rsrc, finals).all()) if finals.size else n == 0
    indeg = np.bincount(nxt, minlength=n)
    fr, removed = np.nonzero(indeg == 0)[0], 0
    while fr.size:
        removed += fr.size
        cnt = off[fr + 1] - off[fr]
        idx = np.repeat(off[fr] - np.cumsum(np.r_[0, cnt[:-1]]), cnt) + np.arange(cnt.sum())
        t = nxt[idx]
        np.subtract.at(indeg, t, 1)
        t = np.unique(t)
        fr = t[indeg[t] == 0]
    cyclic = removed != n
    initial_cyclic = bool(reach(n, off, nxt, nxt[off[s0]:off[s0 + 1]])[s0])
    return accessible, coaccessible, cyclic, initial_cyclic


def to_flat(fst):
    """restatement output -> flat arrays as the device stores them (+inf = None: Some(zero) reads as not final)"""
    rows = fst["rows"]
    off = np.zeros(fst["n_states"] + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(r) for r in rows]) if rows else []
    arcs = np.array([tuple(a) for r in rows for a in r], dtype=TR_DTYPE) if off[-1] else np.zeros(0, dtype=TR_DTYPE)
    finals = np.array([INF if f is None else f for f in fst["finals"]], dtype=np.float32)
    return dict(n_states=fst["n_states"], start=fst["start"], offsets=off, arcs=arcs, finals=finals,
                props=fst["props"] & ALL)


class Unsupported(Exception):
    """what the device answers with KO (the message in args[0])"""


def fst_to_flat(fst):
    rows = fst["rows"]
    n = len(rows)
    off = np.zeros(n + 1, dtype=np.uint32)
    if n:
        off[1:] = np.cumsum([len(r) for r in rows])
    arcs = np.array([tuple(a) for r in rows for a in r], dtype=TR_DTYPE) if off[-1] else np.zeros(0, dtype=TR_DTYPE)
    finals = np.array([INF if f is None else f for f in fst["finals"]], dtype=np.float32)
    return dict(n_states=n, start=fst["start"], offsets=off, arcs=arcs, finals=finals, props=fst["props"] & ALL)


def flat_to_fst(flat):
    off, arcs = flat["offsets"], flat["arcs"]
    rows = [[[int(a["ilabel"]), int(a["olabel"]), F32(a["weight"]), int(a["nextstate"])] for a in arcs[off[s]:off[s + 1]]]
            for s in range(flat["n_states"])]
    finals = [None if not np.isfinite(f) else F32(f) for f in flat["finals"]]
    return dict(rows=rows, finals=finals, start=flat["start"], props=int(flat["props"]) & ALL)


def dfs_facts(fst):
    """(accessible, coaccessible, cyclic, initial_cyclic) as the SccVisitor finds them (every state is visited)"""
    n = len(fst["rows"])
    if n == 0:
        return True, True, False, False
    flat = fst_to_flat(fst)
    if flat["start"] is None:
        flat = dict(flat, start=0)
        a, c, cy, ic = graph_facts(flat)
        return False, c, cy, False
    return graph_facts(flat)


def compute_and_update(fst, mask):
    """compute_and_update_properties(mask) (mutable_fst.rs:435-441, compute_fst_properties.rs:13-207); returns the word & mask"""
    p = fst["props"]
    if known(p) & mask == mask:  # use_stored
        return p & mask
    comp = 0
    dfs = DFS_BITS
    want_dfs = bool(mask & (dfs | WEIGHTED_CYCLES | UNWEIGHTED_CYCLES))
    if want_dfs:
        comp |= dfs_bits(dfs_facts(fst))
    if mask & ~dfs:
        comp |= ACCEPTOR | NO_EPSILONS | NO_I_EPSILONS | NO_O_EPSILONS | I_LABEL_SORTED | O_LABEL_SORTED | UNWEIGHTED | \
            TOP_SORTED | STRING
        want_idet = bool(mask & (I_DETERMINISTIC | NOT_I_DETERMINISTIC))
        want_odet = bool(mask & (O_DETERMINISTIC | (O_DETERMINISTIC << 1)))
        if want_idet:
            comp |= I_DETERMINISTIC
        if want_odet:
            comp |= O_DETERMINISTIC
        if want_dfs:
            comp |= UNWEIGHTED_CYCLES
        nfinal = 0
        for s, row in enumerate(fst["rows"]):
            ils, ols, prev = set(), set(), None
            for il, ol, w, ns in row:
                if want_idet and il in ils:
                    comp = (comp | NOT_I_DETERMINISTIC) & ~I_DETERMINISTIC
                if want_odet and ol in ols:
                    comp = (comp | (O_DETERMINISTIC << 1)) & ~O_DETERMINISTIC
                if il != ol:
                    comp = (comp | NOT_ACCEPTOR) & ~ACCEPTOR
                if il == 0 and ol == 0:
                    comp = (comp | EPSILONS) & ~NO_EPSILONS
                if il == 0:
                    comp = (comp | I_EPSILONS) & ~NO_I_EPSILONS
                if ol == 0:
                    comp = (comp | O_EPSILONS) & ~NO_O_EPSILONS
                if prev is not None:
                    if il < prev[0]:
                        comp = (comp | NOT_I_LABEL_SORTED) & ~I_LABEL_SORTED
                    if ol < prev[1]:
                        comp = (comp | NOT_O_LABEL_SORTED) & ~O_LABEL_SORTED
                if not is_one(w) and not is_zero(w):
                    comp = (comp | WEIGHTED) & ~UNWEIGHTED
                    if comp & CYCLIC and comp & UNWEIGHTED_CYCLES:
                        raise Unsupported("cyclic inputs are not supported")  # (the SCC test is not restated)
                if ns <= s:
                    comp = (comp | NOT_TOP_SORTED) & ~TOP_SORTED
                if ns != s + 1:
                    comp = (comp | NOT_STRING) & ~STRING
                prev = (il, ol)
                ils.add(il)
                ols.add(ol)
            if nfinal > 0:
                comp = (comp | NOT_STRING) & ~STRING
            if fst["finals"][s] is not None:
                if not is_one(fst["finals"][s]):
                    comp = (comp | WEIGHTED) & ~UNWEIGHTED
                nfinal += 1
            elif len(row) != 1:
                comp = (comp | NOT_STRING) & ~STRING
        if fst["start"] is not None and fst["start"] != 0:
            comp = (comp | NOT_STRING) & ~STRING
    k = known(comp)
    fst["props"] = (p & ~k) | (comp & k)
    return comp & mask


def is_cyclic(flat):
    return graph_facts(dict(flat, start=0))[2] if flat["n_states"] else False


def make_flat(n, start, rows, finals, props=0):
    off = np.zeros(n + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(r) for r in rows]) if n else []
    arcs = np.array([tuple(a) for r in rows for a in r], dtype=TR_DTYPE) if n and off[-1] else np.zeros(0, dtype=TR_DTYPE)
    return dict(n_states=n, start=start, offsets=off, arcs=arcs, finals=np.array(finals, dtype=np.float32), props=props)


def content_word_of_flat(flat):
    """the word compute_fst_properties finds on the content: every trinary pair known"""
    fst = flat_to_fst(dict(flat, props=0))
    compute_and_update(fst, ALL)
    return fst["props"]


def rows_flat(rows, finals, start=0, props=0):
    return make_flat(len(rows), start, rows, finals, props)


def dfs_facts_ref(fst):
    """the SccVisitor's facts; without a start state dfs_visit returns before it visits anything (dfs_visit.rs:104-110),
    which leaves the visitor's initial word: all four positive bits"""
    if fst["start"] is None:
        return True, True, False, False
    return dfs_facts(fst)


def compute_initial_acyclic(fst):
    """compute_and_update_properties(INITIAL_ACYCLIC) (fst_traits/mutable_fst.rs:435-441, compute_fst_properties.rs:13-58)"""
    p = fst["props"]
    if known(p) & INITIAL_ACYCLIC:  # use_stored
        return bool(p & INITIAL_ACYCLIC)
    comp = dfs_bits(dfs_facts_ref(fst))
    k = known(comp)
    fst["props"] = (p & ~k) | (comp & k)
    return bool(comp & INITIAL_ACYCLIC)


# ---------------------------------------------------------------- the restatement: VectorFst mutations (vector_fst/mutable_fst.rs)
def m_add_state(f):  # :80-85
    f["rows"].append([])
    f["finals"].append(None)
    f["props"] = p_add_state(f["props"])
    return len(f["rows"]) - 1


def m_set_final(f, s, w):  # :66-78; w None = delete_final_weight_unchecked (:293-297)
    f["props"] = p_set_final(f["props"], f["finals"][s], w)
    f["finals"][s] = w


def m_add_tr(f, s, tr):  # :247-252, data_structure.rs:80-91
    row = f["rows"][s]
    prev = row[-1] if row else None
    row.append(list(tr))
    f["props"] = p_add_tr(f["props"], s, tr, prev)


def m_set_start(f, s):  # :46-49
    f["start"] = s
    f["props"] = p_set_start(f["props"])


def m_set_props(f, props, mask=ALL):  # :411-414
    f["props"] = (f["props"] & ~mask) | (props & mask)


def content_word(fst):
    """the word compute_fst_properties finds on the content: every trinary pair known"""
    f = dict(copy.deepcopy(fst), props=0)
    compute_and_update(f, ALL)
    return f["props"]


def to_oracle(oracle, flat):
    return oracle.OracleFst.from_flat(flat["n_states"], flat["start"], flat["offsets"], flat["arcs"], flat["finals"],
                                      flat["props"])
