"""determinize of an acceptor (determinize_fsa_op.rs, state_table.rs), restated."""
import numpy as np

from ..oracle_py import TR_DTYPE
from .props import ACCEPTOR, determinize_props
from .weight import F32, INF, KDELTA, approx_eq, plus, quantize, times


def determinize_ref(flat, delta=KDELTA, det_type=0, max_states=1 << 20):
    """DeterminizeFsa with DefaultCommonDivisor in LazyFst::compute's FIFO first-touch order; subsets in ascending state
    order; a candidate joins the lowest-id state with the same states and approx_eq weights."""
    if not flat["props"] & ACCEPTOR:
        raise ValueError("transducers are not supported")
    props = determinize_props(flat["props"], det_type != 1)
    if flat["start"] is None or flat["n_states"] == 0:
        return dict(n_states=0, start=None, offsets=np.zeros(1, np.uint32), arcs=np.zeros(0, TR_DTYPE),
                    finals=np.zeros(0, np.float32), props=props)
    off, arcs, fin = flat["offsets"], flat["arcs"], flat["finals"]
    tuples = [((int(flat["start"]), F32(0.0)),)]
    by_states = {(int(flat["start"]),): [0]}
    rows, finals, offsets = [], [], [0]

    def find(t):
        ids = by_states.setdefault(tuple(s for s, _ in t), [])
        for i in ids:
            if all(approx_eq(w, v) for (_, w), (_, v) in zip(t, tuples[i])):
                return i
        ids.append(len(tuples))
        tuples.append(t)
        if len(tuples) > max_states:
            raise RuntimeError("does not determinize")
        return len(tuples) - 1

    s = 0
    while s < len(tuples):
        cand = [(int(a["ilabel"]), int(a["nextstate"]), times(w, F32(a["weight"])))
                for q, w in tuples[s] for a in arcs[off[q]:off[q + 1]]]
        cand.sort(key=lambda c: (c[0], c[1]))  # stable
        fw = INF
        for q, w in tuples[s]:
            fw = plus(fw, times(w, F32(fin[q])))
        i = 0
        while i < len(cand):
            j, weight = i, INF
            while j < len(cand) and cand[j][0] == cand[i][0]:
                weight = plus(weight, cand[j][2])
                j += 1
            merged = []
            for _, q, w in cand[i:j]:
                if merged and merged[-1][0] == q:
                    merged[-1][1] = plus(merged[-1][1], w)
                else:
                    merged.append([q, w])
            t = tuple((q, quantize(F32(w - weight), delta)) for q, w in merged)
            rows.append((cand[i][0], cand[i][0], weight, find(t)))
            i = j
        offsets.append(len(rows))
        finals.append(fw)
        s += 1
    a = np.zeros(len(rows), TR_DTYPE)
    for k, r in enumerate(rows):
        a[k] = r
    return dict(n_states=len(tuples), start=0, offsets=np.array(offsets, np.uint32), arcs=a,
                finals=np.array(finals, np.float32), props=props)
