"""rustfst's algorithms restated in sequential Python, each with the lines of the reference it follows: what the
device results are compared with, bit for bit, where the C++ oracle has no such operation.  Here the passes that more
than one restatement runs (connect, tr_map, tr_unique, rm_final_epsilon); the drivers are in the modules beside this one
(determinize.py, push.py, minimize.py, optimize.py, rational.py, top_sort.py)."""
from .weight import F32, INF, approx_eq, is_zero, times
from .props import (ACCESSIBLE, ARCSORT, COACCESSIBLE, DELETE_ARCS, DELETE_STATES, NOT_ACCESSIBLE, NOT_COACCESSIBLE,
                    NULL_PROPS, p_set_final)


# ================================================================ minimize
def connect(fst):  # connect.rs:51-66, del_states (vector_fst/mutable_fst.rs:132-189)
    rows, finals = fst["rows"], fst["finals"]
    n = len(rows)
    access, co = [False] * n, [False] * n
    if fst["start"] is not None:
        stack = [fst["start"]]
        access[fst["start"]] = True
        while stack:
            s = stack.pop()
            for tr in rows[s]:
                if not access[tr[3]]:
                    access[tr[3]] = True
                    stack.append(tr[3])
    pred = [[] for _ in range(n)]
    for s, row in enumerate(rows):
        for tr in row:
            pred[tr[3]].append(s)
    stack = [s for s in range(n) if finals[s] is not None]
    for s in stack:
        co[s] = True
    while stack:
        s = stack.pop()
        for q in pred[s]:
            if not co[q]:
                co[q] = True
                stack.append(q)
    new_id, k = [-1] * n, 0
    for s in range(n):
        if access[s] and co[s]:
            new_id[s] = k
            k += 1
    fst["rows"] = [[[il, ol, w, new_id[ns]] for il, ol, w, ns in rows[s] if new_id[ns] != -1] for s in range(n) if new_id[s] != -1]
    fst["finals"] = [finals[s] for s in range(n) if new_id[s] != -1]
    if fst["start"] is not None:
        fst["start"] = new_id[fst["start"]] if new_id[fst["start"]] != -1 else None
    fst["props"] = (fst["props"] & DELETE_STATES & ~(ACCESSIBLE | NOT_ACCESSIBLE | COACCESSIBLE | NOT_COACCESSIBLE)) | \
        ACCESSIBLE | COACCESSIBLE


def tr_map(fst, arc_fn, final_fn, superfinal, props_fn):  # tr_map.rs:80-181 (MapNoSuperfinal / MapRequireSuperfinal)
    if fst["start"] is None:
        return
    inprops = fst["props"]
    sf = None
    if superfinal:
        sf = len(fst["rows"])
        fst["rows"].append([])
        fst["finals"].append(F32(0.0))
    for s in range(len(fst["rows"])):
        for tr in fst["rows"][s]:
            arc_fn(tr)
        w = fst["finals"][s]
        if w is not None:
            ftr = [0, 0, w]
            final_fn(ftr)
            if not superfinal:
                assert ftr[0] == 0 and ftr[1] == 0
                fst["finals"][s] = ftr[2]
            elif s != sf and (ftr[0] != 0 or ftr[1] != 0 or not is_zero(ftr[2])):
                fst["rows"][s].append([ftr[0], ftr[1], ftr[2], sf])
                fst["finals"][s] = None
    fst["props"] = props_fn(inprops)


# tr_unique.rs:8-51: stable sort on (ilabel, olabel, nextstate) by tr_compare (:8-34), then unique_trs_unchecked
# (vector_fst/mutable_fst.rs:358-377): Vec::dedup with Tr's == (weight: approximate), which compares with the last KEPT arc
def tr_unique(fst):
    for s, row in enumerate(fst["rows"]):
        row.sort(key=lambda t: (t[0], t[1], t[3]))
        out = []
        for t in row:
            if out and out[-1][0] == t[0] and out[-1][1] == t[1] and out[-1][3] == t[3] and approx_eq(out[-1][2], t[2]):
                continue
            out.append(t)
        fst["rows"][s] = out
    p = fst["props"] & ARCSORT & DELETE_ARCS
    if not fst["rows"]:
        p |= NULL_PROPS
    fst["props"] = p


# ================================================================ tr_sum, tr_unique, optimize
def rm_final_epsilon(fst):  # rm_final_epsilon.rs:20-78
    rows, finals = fst["rows"], fst["finals"]
    n = len(rows)
    pred = [[] for _ in range(n)]
    for s, row in enumerate(rows):
        for tr in row:
            pred[tr[3]].append(s)
    co = [f is not None for f in finals]
    stack = [s for s in range(n) if co[s]]
    while stack:
        s = stack.pop()
        for q in pred[s]:
            if not co[q]:
                co[q] = True
                stack.append(q)
    fin_set = {s for s in range(n) if finals[s] is not None and not any(co[tr[3]] for tr in rows[s])}
    p = fst["props"]
    for s in range(n):
        weight, dele = None, []
        for i, tr in enumerate(rows[s]):
            if tr[3] in fin_set and tr[0] == 0 and tr[1] == 0:
                if weight is None:
                    weight = finals[s] if finals[s] is not None else INF
                v = times(finals[tr[3]], tr[2])
                weight = v if v < weight else weight
                dele.append(i)
        if dele:
            if not is_zero(weight):
                p = p_set_final(p, finals[s], weight)
                finals[s] = weight
            rows[s] = [tr for i, tr in enumerate(rows[s]) if i not in dele]
            p &= DELETE_ARCS
    fst["props"] = p
    connect(fst)
