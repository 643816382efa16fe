"""reweight and push_weights (reweight.rs, push.rs), restated."""
import numpy as np

from .fst import csr_next, graph_facts, reach, transpose
from .props import (COACCESSIBLE, DFS_BITS, INITIAL_ACYCLIC, INITIAL_CYCLIC, WEIGHT_INVARIANT, dfs_bits, p_add_state,
                    p_add_tr, p_set_final, p_set_start, p_set_weight)
from .weight import F32, INF, divide, is_one, is_zero, times


def reweight_ref(flat, potentials, to_final, facts=None):
    """reweight(fst, potentials, type) (reweight.rs:29-154), statement by statement; finals as Option (None / value).
    Returns a mutable dict: n_states, start, rows (list of [ilabel, olabel, weight, nextstate] lists per state), finals,
    props."""
    n, start = flat["n_states"], flat["start"]
    off, arcs = flat["offsets"], flat["arcs"]
    rows = [[[int(a["ilabel"]), int(a["olabel"]), F32(a["weight"]), int(a["nextstate"])] for a in arcs[off[s]:off[s + 1]]]
            for s in range(n)]
    finals = [None if not np.isfinite(f) else F32(f) for f in flat["finals"]]
    pot = [F32(x) for x in potentials]
    p = int(flat["props"])
    fst = dict(n_states=n, start=start, rows=rows, finals=finals)
    if n == 0:
        fst["props"] = p
        return fst
    zero = INF
    for state in range(n):
        if state >= len(pot):  # :42-53
            if to_final and finals[state] is not None:
                new = times(zero, finals[state])
                p = p_set_final(p, finals[state], new)
                finals[state] = new
            continue
        d_s = pot[state]
        if is_zero(d_s):  # :57-59
            continue
        for tr in rows[state]:  # :61-86
            d_ns = pot[tr[3]] if tr[3] < len(pot) else zero
            if is_zero(d_ns):
                continue
            w = divide(times(d_s, tr[2]), d_ns) if to_final else divide(times(tr[2], d_ns), d_s)
            p = p_set_weight(p, tr[2], w)
            tr[2] = w
    for s in range(n):  # :88-103
        fw = finals[s]
        if fw is None:
            continue
        d_s = pot[s] if s < len(pot) else zero
        if to_final:
            fw = times(fw, d_s)
        else:
            if is_zero(d_s):
                continue
            fw = divide(fw, d_s)
        p = p_set_final(p, finals[s], fw)
        finals[s] = fw
    if start is not None:  # :105-146
        d_s = pot[start] if start < len(pot) else zero
        if not is_one(d_s) and not is_zero(d_s):
            if not (p & (INITIAL_CYCLIC | INITIAL_ACYCLIC)):  # compute_and_update_properties(INITIAL_ACYCLIC)
                p = (p & ~DFS_BITS) | dfs_bits(facts if facts is not None else graph_facts(flat))
            if p & INITIAL_ACYCLIC:
                for tr in rows[start]:
                    w = times(divide(0.0, d_s), tr[2]) if to_final else times(d_s, tr[2])
                    p = p_set_weight(p, tr[2], w)
                    tr[2] = w
                if finals[start] is not None:
                    fw = times(divide(0.0, d_s), finals[start]) if to_final else times(d_s, finals[start])
                    p = p_set_final(p, finals[start], fw)
                    finals[start] = fw
            else:
                s = n
                rows.append([])
                finals.append(None)
                p = p_add_state(p)
                w = divide(0.0, d_s) if to_final else d_s
                p = p_add_tr(p, s, (0, 0, w, start))
                rows[s].append([0, 0, w, start])
                p = p_set_start(p)
                fst["start"] = s
                fst["n_states"] = n + 1
    fst["props"] = p & WEIGHT_INVARIANT & ~COACCESSIBLE  # reweight_properties (mutate_properties.rs:640-644)
    return fst


def remove_weight_ref(fst, weight, at_final):  # push.rs:147-170
    if is_one(weight) or is_zero(weight):
        return fst
    p = fst["props"]
    if at_final:
        for s in range(fst["n_states"]):
            if fst["finals"][s] is not None:
                fw = divide(fst["finals"][s], weight)
                p = p_set_final(p, fst["finals"][s], fw)
                fst["finals"][s] = fw
    elif fst["start"] is not None:
        st = fst["start"]
        for tr in fst["rows"][st]:
            w = divide(tr[2], weight)
            p = p_set_weight(p, tr[2], w)
            tr[2] = w
        if fst["finals"][st] is not None:
            fw = divide(fst["finals"][st], weight)
            p = p_set_final(p, fst["finals"][st], fw)
            fst["finals"][st] = fw
    fst["props"] = p
    return fst


def push_ref(flat, dist, to_final, remove_total=False, facts=None):
    """push_weights_with_config (push.rs:89-118) given the Vec shortest_distance_with_config returns (reverse distances
    for ToInitial)."""
    total = None
    if remove_total:  # compute_total_weight (push.rs:120-142), on the FST before reweight
        if not to_final:
            s0 = flat["start"]
            total = F32(dist[s0]) if s0 is not None and s0 < len(dist) else INF
        else:
            total = INF
            for s, d in enumerate(dist):
                f = flat["finals"][s]
                total = min(total, times(d, f if np.isfinite(f) else INF))
    fst = reweight_ref(flat, dist, to_final, facts)
    if remove_total:
        fst = remove_weight_ref(fst, total, to_final)
    return fst


def reverse_len_rule(flat):
    """rdistance.len() - 1 (shortest_distance.rs:322-334): the reversed search dequeues every state reachable from the
    super-initial state (the states that reach a final state, + 1) and grows its Vec to the largest of them."""
    n = flat["n_states"]
    off, nxt = csr_next(flat)
    roff, rsrc = transpose(n, off, nxt)
    finals = np.nonzero(np.isfinite(flat["finals"]))[0]
    if not finals.size:
        return 0
    return int(np.nonzero(reach(n, roff, rsrc, finals))[0].max()) + 1
