"""tr_sum, the label encoding and optimize (tr_sum.rs, encode_static.rs, optimize.rs), restated."""
from .algorithms import rm_final_epsilon, tr_map, tr_unique
from .determinize import determinize_ref
from .fst import Unsupported, flat_to_fst, fst_to_flat, to_oracle
from .minimize import minimize_ref
from .props import (ACCEPTOR, ACYCLIC, ALL, ARCSORT, DELETE_ARCS, I_DETERMINISTIC, LABEL_INVARIANT, NO_EPSILONS,
                    NULL_PROPS, UNWEIGHTED, UNWEIGHTED_CYCLES, WEIGHT_INVARIANT, determinize_props)
from .weight import F32


MSG_ACYCLIC = "optimize: inputs whose property word does not hold ACYCLIC are not supported"


def tr_key(t):  # tr_compare (tr_unique.rs:8-34): ilabel, olabel, nextstate; the weight is not in the key
    return (t[0], t[1], t[3])


def tr_sum(fst):  # tr_sum.rs:7-22, sum_trs_unchecked (vector_fst/mutable_fst.rs:380-405)
    props = fst["props"]
    for s, row in enumerate(fst["rows"]):
        row = sorted(row, key=tr_key)  # stable
        out = []
        for t in row:
            if out and tr_key(out[-1]) == tr_key(t):
                if F32(t[2]) < F32(out[-1][2]):  # plus_assign (tropical_weight.rs:53-58)
                    out[-1][2] = F32(t[2])
            else:
                out.append(list(t))
        fst["rows"][s] = out
    p = props & ARCSORT & DELETE_ARCS & WEIGHT_INVARIANT
    if not fst["rows"]:
        p |= NULL_PROPS
    fst["props"] = p


def encode_labels(fst):  # encode(EncodeLabels): encode_static.rs, table.rs; MapNoSuperfinal, weights untouched
    table, pairs = {}, []

    def arc(tr):
        k = (tr[0], tr[1])
        if k not in table:
            pairs.append(k)
            table[k] = len(pairs)
        tr[0] = tr[1] = table[k]
    tr_map(fst, arc, lambda ftr: None, False, lambda p: p & LABEL_INVARIANT)
    return pairs


def decode_labels(fst, pairs):  # decode (decode_static.rs): the pair back, the same mask, rm_final_epsilon
    def arc(tr):
        tr[0], tr[1] = pairs[tr[0] - 1]
    tr_map(fst, arc, lambda ftr: None, False, lambda p: p & LABEL_INVARIANT)
    rm_final_epsilon(fst)


def norm(flat):
    start = flat["start"]
    return dict(flat, start=None if start is None or start < 0 else int(start), props=int(flat["props"]) & ALL)


def determinize_encoded(flat):
    """determinize of a label-encoded machine (ilabel == olabel >= 1, the word without ACCEPTOR): the acceptor
    construction, the word of the gallic call (determinize_static.rs:177-192)"""
    out = determinize_ref(dict(flat, props=flat["props"] | ACCEPTOR))
    out["props"] = determinize_props(flat["props"], True)
    return out


def det_min(flat, encoded):
    det = determinize_encoded(flat) if encoded else determinize_ref(flat)
    return minimize_ref(norm(det))


def optimize_ref(flat, oracle):
    """optimize (optimize.rs:11-128) for the tropical semiring; raises Unsupported (or determinize_ref's ValueError) with the
    KO message"""
    flat = norm(flat)
    acceptor = bool(flat["props"] & ACCEPTOR)
    cur = flat
    if not cur["props"] & NO_EPSILONS:
        cur = norm(to_oracle(oracle, cur).rm_epsilon().to_flat())
    fst = flat_to_fst(cur)
    tr_sum(fst)
    cur = fst_to_flat(fst)
    p = cur["props"]
    if p & I_DETERMINISTIC:
        return minimize_ref(cur)
    if not p & ACYCLIC:  # intersects(ACYCLIC | UNWEIGHTED | UNWEIGHTED_CYCLES): tr_sum's mask left neither of the others
        assert not p & (UNWEIGHTED | UNWEIGHTED_CYCLES)
        raise Unsupported(MSG_ACYCLIC)
    if acceptor:
        return det_min(cur, False)
    pairs = encode_labels(fst)
    mini = flat_to_fst(det_min(fst_to_flat(fst), True))
    decode_labels(mini, pairs)
    return fst_to_flat(mini)


def apply_op(op, flat, oracle=None):
    if op == "optimize":
        return optimize_ref(flat, oracle)
    fst = flat_to_fst(norm(flat))
    (tr_sum if op == "tr_sum" else tr_unique)(fst)
    return fst_to_flat(fst)


def branch_of(flat, oracle):
    cur = norm(flat)
    if not cur["props"] & NO_EPSILONS:
        cur = norm(to_oracle(oracle, cur).rm_epsilon().to_flat())
    fst = flat_to_fst(cur)
    tr_sum(fst)
    if fst["props"] & I_DETERMINISTIC:
        return "min"
    if not fst["props"] & ACYCLIC:
        return "ko"
    return "det-min" if flat["props"] & ACCEPTOR else "encode"
