"""union, concat, closure and the list folds (union_static.rs, concat_static.rs, closure_static.rs), restated."""
import copy
import numpy as np

from .fst import compute_initial_acyclic, m_add_state, m_add_tr, m_set_final, m_set_props, m_set_start
from .props import closure_properties, concat_properties, union_properties
from .weight import F32


ONE = F32(0.0)
STAR, PLUS = 0, 1  # closure/mod.rs:9-12


def union_ref(f1, f2):  # union/union_static.rs:55-118
    ia1 = compute_initial_acyclic(f1)
    props1, props2 = f1["props"], f2["props"]
    n1 = len(f1["rows"])
    start2 = f2["start"]
    if start2 is None:
        return f1
    for s2 in range(len(f2["rows"])):
        s1 = m_add_state(f1)
        if f2["finals"][s2] is not None:
            m_set_final(f1, s1, f2["finals"][s2])
        for il, ol, w, ns in f2["rows"][s2]:
            m_add_tr(f1, s1, [il, ol, w, ns + n1])
    start1 = f1["start"]
    if start1 is None:
        m_set_start(f1, start2)  # (:89) without the offset
        m_set_props(f1, props2)  # copy_properties() holds every trinary bit (properties.rs:130-163)
        return f1
    if ia1:
        m_add_tr(f1, start1, [0, 0, ONE, start2 + n1])
    else:
        nstart = m_add_state(f1)
        m_set_start(f1, nstart)
        m_add_tr(f1, nstart, [0, 0, ONE, start1])
        m_add_tr(f1, nstart, [0, 0, ONE, start2 + n1])
    m_set_props(f1, union_properties(props1, props2))
    return f1


def concat_ref(f1, f2):  # concat/concat_static.rs:53-109
    props1, props2 = f1["props"], f2["props"]
    if f1["start"] is None:
        return f1
    n1 = len(f1["rows"])
    for s2 in range(len(f2["rows"])):
        s1 = m_add_state(f1)
        if f2["finals"][s2] is not None:
            m_set_final(f1, s1, f2["finals"][s2])
        for il, ol, w, ns in f2["rows"][s2]:
            m_add_tr(f1, s1, [il, ol, w, ns + n1])
    start2 = f2["start"]
    for s1 in range(n1):
        w = f1["finals"][s1]
        if w is not None:
            if start2 is not None:
                m_add_tr(f1, s1, [0, 0, w, start2 + n1])
            m_set_final(f1, s1, None)
    if start2 is not None:
        m_set_props(f1, concat_properties(props1, props2))
    return f1


def closure_ref(f, closure_type):  # closure/closure_static.rs:25-73
    props = f["props"]
    if f["start"] is not None:
        for s, w in [(s, w) for s, w in enumerate(f["finals"]) if w is not None]:
            m_add_tr(f, s, [0, 0, w, f["start"]])
    if closure_type == STAR:
        nstart = m_add_state(f)
        if f["start"] is not None:
            m_add_tr(f, nstart, [0, 0, ONE, f["start"]])
        m_set_start(f, nstart)
        m_set_final(f, nstart, ONE)
    m_set_props(f, closure_properties(props))
    return f


def fold_ref(op, fsts):  # rustfst-python union_list / concat_list (algorithms/union.py:47-64, concat.py)
    if not fsts:
        raise ValueError("fsts must be at least of len 1")
    acc = copy.deepcopy(fsts[0])
    for f in fsts[1:]:
        acc = op(acc, f)
    return acc


def union_list_closed(fsts):
    """fsts[0] has a start state: states i_0, i_1, the new state if fsts[0] is not initial-acyclic, i_2, ...; the root's
    row = (its own arcs | 0:0/One -> start(i_0)) + 0:0/One -> base_k + start(i_k)"""
    first = copy.deepcopy(fsts[0])
    ia = compute_initial_acyclic(first)
    items = [fsts[0]] + [f for f in fsts[1:] if f["start"] is not None]
    if len(items) == 1:
        return first["rows"], first["finals"], first["start"]
    rows, finals, bases = [], [], []
    new_state = None
    for k, f in enumerate(items):
        if not ia and k == 2:
            new_state = len(rows)
            rows.append(None)
            finals.append(None)
        bases.append(len(rows))
        rows += [[[il, ol, w, ns + bases[k]] for il, ol, w, ns in row] for row in f["rows"]]
        finals += list(f["finals"])
    if not ia and new_state is None:
        new_state = len(rows)
        rows.append(None)
        finals.append(None)
    extra = [[0, 0, ONE, bases[k] + items[k]["start"]] for k in range(1, len(items))]
    if ia:
        root = items[0]["start"]
        rows[root] = rows[root] + extra
    else:
        root = new_state
        rows[root] = [[0, 0, ONE, items[0]["start"]]] + extra
    return rows, finals, root


def concat_list_closed(fsts):
    """every item has a start state: all states one after the other; a final state of item k < n - 1 gets
    0:0/w -> base_{k+1} + start_{k+1} and loses its final weight"""
    bases = np.concatenate([[0], np.cumsum([len(f["rows"]) for f in fsts])]).tolist()
    rows, finals = [], []
    for k, f in enumerate(fsts):
        for s, row in enumerate(f["rows"]):
            row = [[il, ol, w, ns + bases[k]] for il, ol, w, ns in row]
            w = f["finals"][s]
            if w is not None and k + 1 < len(fsts):
                row.append([0, 0, w, bases[k + 1] + fsts[k + 1]["start"]])
                w = None
            rows.append(row)
            finals.append(w)
    return rows, finals, fsts[0]["start"]
