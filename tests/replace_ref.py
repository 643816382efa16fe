"""rustfst's `replace` restated in sequential Python, line by line: what the device results of tests/test_replace.py are
compared with, bit for bit.  ReplaceFst::new + compute() (algorithms/replace/replace_fst.rs:29-47, replace_static.rs:44-58)
= LazyFst::compute (algorithms/lazy/lazy_fst.rs:226-269) over ReplaceFstOp (algorithms/replace/replace_fst_op.rs), with
the two state tables as dicts in find_id order (lazy/state_table.rs:49-59).  FSTs are in the rows form of oracle.model
(dict(rows, finals, start, props)); `pairs` is the reference's Vec<(Label, fst)>.

The reference does not terminate on a grammar whose expansion reaches a recursive call; `step_cap` bounds the states
taken from the queue (Diverged is raised beyond it), and `info`, a dict, receives what the tests count: the prefix table,
the deepest prefix, the levels of the queue, the arcs by kind."""
from collections import deque

from oracle.model import (ACCEPTOR, ACCESSIBLE, ACYCLIC, COACCESSIBLE, CYCLIC, EPSILONS, INITIAL_ACYCLIC, INITIAL_CYCLIC,
                          I_DETERMINISTIC, I_EPSILONS, I_LABEL_SORTED, NOT_ACCEPTOR, NOT_I_DETERMINISTIC, NOT_STRING,
                          NOT_TOP_SORTED, NO_I_EPSILONS, NULL_PROPS, O_EPSILONS, O_LABEL_SORTED, STRING, UNWEIGHTED, WEIGHTED,
                          WEIGHTED_CYCLES, m_set_props)

NOT_O_DETERMINISTIC = 1 << 21  # (oracle.model.props names the pair by O_DETERMINISTIC << 1)
NEITHER, INPUT, OUTPUT, BOTH = range(4)  # ReplaceLabelType, replace/config.rs:3-10


class ReplaceError(Exception):
    """the reference's Err (the message in args[0])"""


class Diverged(Exception):
    """more than step_cap states were expanded: the reference would go on (for ever, if the grammar recurses)"""


def epsilon_on_input(t):  # replace/utils.rs:4-6
    return t in (NEITHER, OUTPUT)


def epsilon_on_output(t):  # replace/utils.rs:8-10
    return t in (NEITHER, INPUT)


def replace_transducer(call_t, return_t, call_output_label):  # replace_fst_op.rs:188-198
    return call_t in (INPUT, OUTPUT) or (call_t == BOTH and call_output_label is not None) or return_t in (INPUT, OUTPUT)


def mutate_replace_properties(inprops, root, epsilon_on_call, epsilon_on_return, out_epsilon_on_call, out_epsilon_on_return,
                              transducer, no_empty_fsts, all_ilabel_sorted, all_olabel_sorted, all_negative_or_dense):
    """fst_properties/mutate_properties.rs:496-620"""
    if not inprops:  # :510-512
        return NULL_PROPS
    outprops = 0
    access_props = (ACCESSIBLE | COACCESSIBLE) if no_empty_fsts else 0  # :514-518
    for p in inprops:  # :520-522
        access_props &= p & (ACCESSIBLE | COACCESSIBLE)
    if access_props == (ACCESSIBLE | COACCESSIBLE):  # :524-556
        outprops |= access_props
        if inprops[root] & INITIAL_CYCLIC:
            outprops |= INITIAL_CYCLIC
        props, string = 0, True
        for p in inprops:
            if transducer:
                props |= NOT_ACCEPTOR & p
            props |= (NOT_I_DETERMINISTIC | NOT_O_DETERMINISTIC | EPSILONS | I_EPSILONS | O_EPSILONS | WEIGHTED |
                      WEIGHTED_CYCLES | CYCLIC | NOT_TOP_SORTED | NOT_STRING) & p
            if not p & STRING:
                string = False
        outprops |= props
        if string:
            outprops |= STRING
    acceptor = not transducer  # :557-561
    ideterministic = (not epsilon_on_call) and epsilon_on_return
    no_iepsilons = (not epsilon_on_call) and (not epsilon_on_return)
    acyclic = unweighted = True
    for i, p in enumerate(inprops):  # :562-581
        if not p & ACCEPTOR:
            acceptor = False
        if not p & I_DETERMINISTIC:
            ideterministic = False
        if not p & NO_I_EPSILONS:
            no_iepsilons = False
        if not p & ACYCLIC:
            acyclic = False
        if not p & UNWEIGHTED:
            unweighted = False
        if i != root and not p & NO_I_EPSILONS:
            ideterministic = False
    if acceptor:  # :582-599
        outprops |= ACCEPTOR
    if ideterministic:
        outprops |= I_DETERMINISTIC
    if no_iepsilons:
        outprops |= NO_I_EPSILONS
    if acyclic:
        outprops |= ACYCLIC
    if unweighted:
        outprops |= UNWEIGHTED
    if inprops[root] & INITIAL_ACYCLIC:
        outprops |= INITIAL_ACYCLIC
    if all_ilabel_sorted and epsilon_on_return and ((not epsilon_on_call) or all_negative_or_dense):  # :608-610
        outprops |= I_LABEL_SORTED
    if all_olabel_sorted and out_epsilon_on_return and ((not out_epsilon_on_call) or all_negative_or_dense):  # :617-620
        outprops |= O_LABEL_SORTED
    return outprops


def replace_properties(root_label, pairs, call_t, return_t, call_output_label):
    """replace_fst_op.rs:120-186, over the STORED words (fst.properties())"""
    inprops = []
    all_ilabel_sorted = all_olabel_sorted = all_non_empty = True
    all_negative = False  # (labels are unsigned)
    dense_range = True
    root_fst_idx = 0
    for i, (label, fst) in enumerate(pairs):
        if label > len(pairs):
            dense_range = False
        if label == root_label:
            root_fst_idx = i
        if fst["start"] is None:
            all_non_empty = False
        if not fst["props"] & I_LABEL_SORTED:
            all_ilabel_sorted = False
        if not fst["props"] & O_LABEL_SORTED:
            all_olabel_sorted = False
        inprops.append(fst["props"])
    return mutate_replace_properties(inprops, root_fst_idx, epsilon_on_input(call_t), epsilon_on_input(return_t),
                                     epsilon_on_output(call_t), epsilon_on_output(return_t),
                                     replace_transducer(call_t, return_t, call_output_label), all_non_empty,
                                     all_ilabel_sorted, all_olabel_sorted, all_negative or dense_range)


class StateTable:  # lazy/state_table.rs:49-59: ids in the order of first find_id
    def __init__(self):
        self.ids, self.tuples = {}, []

    def find_id(self, t):
        if t not in self.ids:
            self.ids[t] = len(self.tuples)
            self.tuples.append(t)
        return self.ids[t]

    def find_tuple(self, i):
        return self.tuples[i]


def replace_ref(pairs, root, epsilon_on_replace, step_cap=None, info=None):
    """replace(fst_list, root, epsilon_on_replace): the result in rows form (rows, finals, start, props, n_states)"""
    pairs = list(pairs)
    # ReplaceFstOptions::new, replace/config.rs:22-36
    call_t = NEITHER if epsilon_on_replace else INPUT
    return_t = NEITHER
    call_output_label = 0 if epsilon_on_replace else None
    return_label = 0
    # ReplaceFstOp::new, replace_fst_op.rs:201-256
    properties = replace_properties(root, pairs, call_t, return_t, call_output_label)
    if call_output_label is not None and call_output_label == 0:  # :227-231
        call_t = NEITHER
    if return_label == 0:  # :233-235
        return_t = NEITHER
    fst_array, nonterminal_set, nonterminal_hash = [], set(), {}
    for label, fst in pairs:  # :237-243: insert overwrites
        nonterminal_hash[label] = len(fst_array)
        nonterminal_set.add(label)
        fst_array.append(fst)
    if root not in nonterminal_hash:  # :245-253
        raise ReplaceError(f"ReplaceFstImpl: No FST corresponding to root label {root} in the input tuple vector")
    root_idx = nonterminal_hash[root]
    prefix_table, tuple_table = StateTable(), StateTable()  # of tuples of frames (fst_id, nextstate) / (prefix_id, fst_id, state)
    counts = dict(call_arcs=0, dropped_calls=0, return_arcs=0, max_depth=0)

    def get_prefix_id(prefix):  # :304-306
        counts["max_depth"] = max(counts["max_depth"], len(prefix))
        return prefix_table.find_id(prefix)

    def compute_final_tr(state):  # :258-302
        prefix_id, fst_id, fst_state = tuple_table.find_tuple(state)
        if fst_array[fst_id]["finals"][fst_state] is not None and prefix_id > 0:
            ilabel = 0 if epsilon_on_input(return_t) else return_label
            olabel = 0 if epsilon_on_output(return_t) else return_label
            stack = prefix_table.find_tuple(prefix_id)
            top = stack[-1]
            popped = get_prefix_id(stack[:-1])  # pop_prefix :308-311
            nextstate = tuple_table.find_id((popped, top[0], top[1]))
            weight = fst_array[fst_id]["finals"][fst_state]
            if weight is not None:
                counts["return_arcs"] += 1
                return [ilabel, olabel, weight, nextstate]
        return None

    def compute_tr(tup, tr):  # :323-370
        prefix_id, fst_id, _ = tup
        il, ol, w, ns = tr
        if ol == 0 or ol < min(nonterminal_set) or ol > max(nonterminal_set):
            return [il, ol, w, tuple_table.find_id((prefix_id, fst_id, ns))]
        if ol in nonterminal_hash:
            nonterminal = nonterminal_hash[ol]
            p = prefix_table.find_tuple(prefix_id)
            nt_prefix = get_prefix_id(p + ((fst_id, ns),))  # push_prefix :313-321
            nt_start = fst_array[nonterminal]["start"]
            if nt_start is not None:
                nt_nextstate = tuple_table.find_id((nt_prefix, nonterminal, nt_start))
                ilabel = 0 if epsilon_on_input(call_t) else il
                olabel = 0 if epsilon_on_output(call_t) else (call_output_label if call_output_label is not None else ol)
                counts["call_arcs"] += 1
                return [ilabel, olabel, w, nt_nextstate]
            counts["dropped_calls"] += 1
            return None
        return [il, ol, w, tuple_table.find_id((prefix_id, fst_id, ns))]

    def compute_trs(state):  # :76-100
        tup = tuple_table.find_tuple(state)
        trs = []
        tr = compute_final_tr(state)
        if tr is not None:
            trs.append(tr)
        for tr in fst_array[tup[1]]["rows"][tup[2]]:
            new_tr = compute_tr(tup, tr)
            if new_tr is not None:
                trs.append(new_tr)
        return trs

    def compute_final_weight(state):  # :102-113
        prefix_id, fst_id, fst_state = tuple_table.find_tuple(state)
        return fst_array[fst_id]["finals"][fst_state] if prefix_id == 0 else None

    # compute_start, :60-74
    start = None
    if fst_array and fst_array[root_idx]["start"] is not None:
        prefix = get_prefix_id(())
        start = tuple_table.find_id((prefix, root_idx, fst_array[root_idx]["start"]))
    # LazyFst::compute, lazy_fst.rs:226-269
    out = dict(rows=[], finals=[], start=None, props=NULL_PROPS)  # VectorFst::new()
    levels = 0
    if start is not None:
        out["rows"] = [[] for _ in range(start + 1)]
        out["finals"] = [None] * (start + 1)
        out["start"] = start
        queue, visited = deque([start]), {start}
        level_end, steps = start, 0  # (the last state of the level being expanded: the tests count levels)
        levels = 1
        while queue:
            s = queue.popleft()
            steps += 1
            if step_cap is not None and steps > step_cap:
                if info is not None:
                    info.update(counts, prefixes=len(prefix_table.tuples) - 1, diverged=True)
                raise Diverged(f"more than {step_cap} states expanded")
            trs = compute_trs(s)
            for tr in trs:
                if tr[3] not in visited:
                    queue.append(tr[3])
                    visited.add(tr[3])
                while tr[3] >= len(out["rows"]):
                    out["rows"].append([])
                    out["finals"].append(None)
            out["rows"][s] = trs
            out["finals"][s] = compute_final_weight(s)
            if s == level_end and queue:
                levels += 1
                level_end = queue[-1]
        m_set_props(out, properties, ~0)  # set_properties stores the word as it is (vector_fst/mutable_fst.rs:407-409)
    out["n_states"] = len(out["rows"])
    if info is not None:
        info.update(counts, prefixes=len(prefix_table.tuples) - 1 if start is not None else 0, levels=levels,
                    prefix_table=prefix_table.tuples, tuple_table=tuple_table.tuples)
    return out
