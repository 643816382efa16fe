"""minimize_with_config for deterministic acyclic acceptors (minimize.rs, partition.rs), restated."""
from .algorithms import connect, rm_final_epsilon, tr_map, tr_unique
from .fst import Unsupported, compute_and_update, flat_to_fst, fst_to_flat, is_cyclic
from .props import (ACCEPTOR, ACYCLIC, ADD_SUPER_FINAL, ALL, ARCSORT, ARC_RELEVANT, CYCLIC, I_DETERMINISTIC,
                    I_LABEL_INVARIANT, I_LABEL_SORTED, O_LABEL_INVARIANT, O_LABEL_SORTED, RM_SUPER_FINAL, UNWEIGHTED,
                    WEIGHTED, WEIGHT_INVARIANT, known, p_add_tr, p_set_start)
from .push import push_ref, reverse_len_rule
from .weight import F32, INF, KSHORTESTDELTA, quantize, times, wkey


MSG_NONDET = "Refusing to minimize a non-deterministic FST with allow_nondet = false"


class Partition:  # partition.rs:6-92
    def __init__(self, n):
        self.cls = [None] * n
        self.nxt = [-1] * n
        self.prv = [-1] * n
        self.head = []

    def add_class(self):
        self.head.append(-1)
        return len(self.head) - 1

    def add(self, e, c):
        h = self.head[c]
        if h >= 0:
            self.prv[h] = e
        self.head[c] = e
        self.cls[e] = c
        self.nxt[e] = h
        self.prv[e] = -1

    def move_element(self, e, c):
        p, nx, old = self.prv[e], self.nxt[e], self.cls[e]
        if p >= 0:
            self.nxt[p] = nx
        else:
            self.head[old] = nx
        if nx >= 0:
            self.prv[nx] = p
        self.add(e, c)

    def members(self, c):
        e = self.head[c]
        while e >= 0:
            yield e
            e = self.nxt[e]


def fst_depth(fst):  # minimize.rs:269-304 (an explicit stack in place of the recursion; same post-order)
    rows = fst["rows"]
    heights = []
    visited = set()
    stack = [(fst["start"], 0)]
    visited.add(fst["start"])
    while stack:
        s, i = stack[-1]
        while len(heights) <= s:
            heights.append(-1)
        if i < len(rows[s]):
            stack[-1] = (s, i + 1)
            t = rows[s][i][3]
            if t not in visited:
                visited.add(t)
                stack.append((t, 0))
        else:
            stack.pop()
            heights[s] = max([0] + [1 + heights[tr[3]] for tr in rows[s]])
    return heights


def acyclic_partition(fst):
    """AcyclicMinimizer::new (minimize.rs:306-387): classes by height, refined height by height; two states compare Equal
    when StateComparator finds neither below the other (:389-456): final weight (exact), arc count, positionally
    (ilabel, class of nextstate)."""
    heights = fst_depth(fst)
    part = Partition(len(heights))
    for _ in range(max(heights) + 1):
        part.add_class()
    for s, h in enumerate(heights):
        part.add(s, h)
    n_height = len(part.head)
    for h in range(n_height):
        def key(s):
            f = fst["finals"][s]
            return (float(INF if f is None else f), len(fst["rows"][s]), tuple((tr[0], part.cls[tr[3]]) for tr in fst["rows"][s]))
        members = list(part.members(h))
        equiv = {key(members[0]): h}
        for e in members[1:]:
            k = key(e)
            if k not in equiv:
                equiv[k] = part.add_class()
        target = {s: equiv[key(s)] for s in members}  # (the keys read the partition before any move of this height)
        for s in members:
            if part.cls[s] != target[s]:
                part.move_element(s, target[s])
    return part


def merge_states(part, fst):  # minimize.rs:213-266
    rows = fst["rows"]
    state_map = [next(part.members(c)) for c in range(len(part.head))]
    p = fst["props"]
    for c in range(len(part.head)):
        for s in part.members(c):
            if s == state_map[c]:
                for tr in rows[s]:
                    p &= ARC_RELEVANT  # set_nextstate_unchecked (trs_iter_mut.rs:222-225, 293-305)
                    tr[3] = state_map[part.cls[tr[3]]]
            else:
                for tr in [list(t) for t in rows[s]]:
                    tr[3] = state_map[part.cls[tr[3]]]
                    dst = rows[state_map[c]]
                    dst.append(tr)
                    p = p_add_tr(p, state_map[c], tr, dst[-2] if len(dst) > 1 else None)
    fst["start"] = state_map[part.cls[fst["start"]]]
    fst["props"] = p_set_start(p)
    connect(fst)


def acceptor_minimize(fst, seen=None):  # minimize.rs:181-211
    """seen (a dict): receives T, a copy of the connected, label-sorted machine the partition is computed on (what
    minimize.hip's run_core refines), and part, its Partition"""
    props = compute_and_update(fst, ACCEPTOR | UNWEIGHTED | ACYCLIC)
    if props & (ACCEPTOR | UNWEIGHTED) != ACCEPTOR | UNWEIGHTED:
        raise Unsupported("FST is not an unweighted acceptor")
    if not props & ACYCLIC:
        raise Unsupported("cyclic inputs are not supported")  # (this project: a cycle anywhere, before connect)
    connect(fst)
    if not fst["rows"]:
        return
    for row in fst["rows"]:  # tr_sort(ILabelCompare): stable
        row.sort(key=lambda t: t[0])
    p = (fst["props"] & ARCSORT) | I_LABEL_SORTED
    if fst["props"] & ACCEPTOR:
        p |= O_LABEL_SORTED
    fst["props"] = p
    part = acyclic_partition(fst)
    if seen is not None:
        seen["T"] = dict(rows=[[list(tr) for tr in row] for row in fst["rows"]], finals=list(fst["finals"]),
                         start=fst["start"], props=fst["props"])
        seen["part"] = part
    merge_states(part, fst)
    tr_unique(fst)


def rdist_dag(flat):
    """reverse shortest distances of an acyclic FST in f32: d[s] = min(final[s], min over arcs (w + d[next])), the value the
    relaxation converges to (f32 addition is monotone); +inf for a state that reaches no final state"""
    n = flat["n_states"]
    off, arcs, fin = flat["offsets"], flat["arcs"], flat["finals"]
    d = [None] * n
    for root in range(n):
        if d[root] is not None:
            continue
        stack = [(root, 0)]
        while stack:
            s, i = stack[-1]
            b, e = int(off[s]), int(off[s + 1])
            if b + i < e:
                stack[-1] = (s, i + 1)
                t = int(arcs["nextstate"][b + i])
                if d[t] is None and all(t != q for q, _ in stack):
                    stack.append((t, 0))
            else:
                stack.pop()
                best = F32(fin[s])
                for a in arcs[b:e]:
                    v = times(F32(a["weight"]), d[int(a["nextstate"])])
                    best = v if v < best else best
                d[s] = best
    return d


def minimize_ref(flat, delta=KSHORTESTDELTA, allow_nondet=False, partition_out=None):
    """minimize_with_config (minimize.rs:92-176), statement by statement, for the branch this project supports; raises
    Unsupported with the KO message otherwise.  Returns flat arrays.  partition_out (a dict): see acceptor_minimize (in the
    weighted branch T is the encoded machine with its superfinal state)."""
    fst = flat_to_fst(flat)
    props = compute_and_update(fst, ACCEPTOR | I_DETERMINISTIC | WEIGHTED | UNWEIGHTED)
    if not props & I_DETERMINISTIC and not allow_nondet:
        raise Unsupported(MSG_NONDET)
    if not props & ACCEPTOR:
        raise Unsupported("transducers are not supported")
    if not props & I_DETERMINISTIC:
        raise Unsupported("non-deterministic inputs are not supported")
    if not known(fst["props"]) & ACYCLIC:
        if is_cyclic(flat):
            raise Unsupported("cyclic inputs are not supported")
    elif fst["props"] & CYCLIC:
        raise Unsupported("cyclic inputs are not supported")
    if props & WEIGHTED:
        # (without a start state push still reweights, every tr_map below returns at once, and acceptor_minimize decides
        # from the pushed content: the empty FST, or "FST is not an unweighted acceptor")
        # push_weights_with_config(ToInitial, default.with_delta(delta)) (push.rs:89-118)
        cur = fst_to_flat(fst)
        dist = rdist_dag(cur)[:reverse_len_rule(cur)]
        fst = push_ref(cur, dist, False, False)
        fst["props"] &= ALL
        # tr_map(QuantizeMapper(delta)) (quantize_mapper.rs)
        def q_arc(tr):
            tr[2] = quantize(tr[2], delta)

        def q_fin(ftr):
            ftr[2] = quantize(ftr[2], delta)
        tr_map(fst, q_arc, q_fin, False, lambda p: p & WEIGHT_INVARIANT)
        # encode(EncodeWeightsAndLabels) (encode_static.rs): one table for arc and final tuples, in scan order
        table, tuples = {}, []

        def enc(il, ol, w):
            k = (il, ol, wkey(w))
            if k not in table:
                table[k] = len(tuples) + 1
                tuples.append((il, ol, F32(w)))
            return table[k]

        def e_arc(tr):
            lab = enc(tr[0], tr[1], tr[2])
            tr[0], tr[1], tr[2] = lab, lab, F32(0.0)

        def e_fin(ftr):
            lab = enc(ftr[0], ftr[1], ftr[2])
            ftr[0], ftr[1], ftr[2] = lab, lab, F32(0.0)
        enc_mask = I_LABEL_INVARIANT & O_LABEL_INVARIANT & WEIGHT_INVARIANT & ADD_SUPER_FINAL
        tr_map(fst, e_arc, e_fin, True, lambda p: p & enc_mask)
        acceptor_minimize(fst, partition_out)
        # decode (decode_static.rs): labels and weights back, then rm_final_epsilon
        def d_arc(tr):
            il, ol, w = tuples[tr[0] - 1]
            tr[0], tr[1], tr[2] = il, ol, w
        dec_mask = I_LABEL_INVARIANT & O_LABEL_INVARIANT & WEIGHT_INVARIANT & RM_SUPER_FINAL
        tr_map(fst, d_arc, lambda ftr: None, False, lambda p: p & dec_mask)
        rm_final_epsilon(fst)
    else:
        acceptor_minimize(fst, partition_out)
    return fst_to_flat(fst)
