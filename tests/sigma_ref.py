"""rustfst's compose_with_config with SigmaMatcher configs restated in sequential Python, line by line: what the device
results of tests/test_compose_sigma*.py are compared with, bit for bit.  compose_with_config
(algorithms/compose/compose_static.rs:166-266) = ComposeFst::new_with_options + compute() = LazyFst::compute
(algorithms/lazy/lazy_fst.rs:226-269) over ComposeFstOp (compose/compose_fst_op.rs), the state table a dict in find_id order
(lazy/state_table.rs:49-59), the matchers SortedMatcher (compose/matchers/sorted_matcher.rs) and SigmaMatcher
(compose/matchers/sigma_matcher.rs), the six filters of compose/compose_filters/.  FSTs are in the rows form of oracle.model
(dict(rows, finals, start, props)).  A matcher config is None or (sigma_label, rewrite_mode, allowed): rewrite_mode 0 Auto,
1 Always, 2 Never; allowed None or empty = no restriction (rustfst-ffi/src/algorithms/compose.rs:199-211).

`info`, a dict, receives what the tests count (the counters of wfst_ctx_get_compose_sigma_counters)."""
from oracle.model import (ACCEPTOR, ACCESSIBLE, ACYCLIC, INITIAL_ACYCLIC, I_DETERMINISTIC, I_LABEL_SORTED, NO_I_EPSILONS,
                          NULL_PROPS, O_LABEL_SORTED)
from oracle.model.algorithms import connect as model_connect
from oracle.model.weight import times

NO_EPSILONS, NO_O_EPSILONS, O_DETERMINISTIC = 1 << 23, 1 << 27, 1 << 20  # (properties.rs:22-103)
NOT_I_LABEL_SORTED, NOT_O_LABEL_SORTED = I_LABEL_SORTED << 1, O_LABEL_SORTED << 1
EPS_LABEL, NO_LABEL = 0, 0xFFFFFFFF
NO_STATE = None  # FilterState::new_no_state()
AUTO, NULL, TRIVIAL, SEQUENCE, ALT_SEQUENCE, MATCH, NO_MATCH = range(7)  # ComposeFilterEnum, compose_static.rs:19-28
MATCH_INPUT, MATCH_OUTPUT, MATCH_BOTH, MATCH_NONE, MATCH_UNKNOWN = "input", "output", "both", "none", "unknown"
EPS_LOOP = "loop"  # IterItemMatcher::EpsLoop
COUNTERS = ("levels", "states", "arcs", "require1_states", "require2_states", "exact_items", "sigma_items", "sigma_arcs",
            "refused_items")


class SigmaError(Exception):
    """the reference's Err (the message in args[0])"""


class SortedMatcher:  # sorted_matcher.rs:36-98
    def __init__(self, fst, match_type):
        self.fst, self.match_type = fst, match_type
        self.sigma_label = NO_LABEL  # (not a sigma matcher)

    def label_of(self, tr):  # :157-163
        return tr[0] if self.match_type == MATCH_INPUT else tr[1]

    def iter(self, state, label):  # IteratorSortedMatcher, :124-184
        trs = self.fst["rows"][state]
        current_loop = label == EPS_LABEL  # :126
        match_label = EPS_LABEL if label == NO_LABEL else label  # :130-134
        if current_loop:  # :137-145
            pos = 0
        else:  # lower_bound_by
            lo, hi = 0, len(trs)
            while lo < hi:
                mid = (lo + hi) // 2
                if self.label_of(trs[mid]) < match_label:
                    lo = mid + 1
                else:
                    hi = mid
            pos = lo
        out = []
        if current_loop:  # :170-173
            out.append(EPS_LOOP)
        while pos < len(trs) and self.label_of(trs[pos]) == match_label:  # :174-183
            out.append(list(trs[pos]))
            pos += 1
        return out

    def test_match_type(self, test):  # :56-85 (properties_check fails on an unknown pair: the caller decides what that means)
        true_prop = I_LABEL_SORTED if self.match_type == MATCH_INPUT else O_LABEL_SORTED
        props = self.fst["props"]
        if props & true_prop:
            return self.match_type
        if props & (true_prop << 1):
            return MATCH_NONE
        return MATCH_UNKNOWN

    def require_match(self):  # flags(), :87-89
        return False

    def priority(self, state):  # :91-93
        return len(self.fst["rows"][state])


class SigmaMatcher:  # sigma_matcher.rs:47-149
    def __init__(self, match_type, sigma_label, rewrite_mode, matcher, allowed):
        if sigma_label == EPS_LABEL:  # :64-66
            raise SigmaError("SigmaMatcher: 0 cannot be used as sigma_label")
        self.match_type, self.sigma_label, self.matcher = match_type, sigma_label, matcher
        self.fst = matcher.fst
        self.rewrite_both = {0: bool(matcher.fst["props"] & ACCEPTOR), 1: True, 2: False}[rewrite_mode]  # :67-75
        self.allowed = set(allowed) if allowed else None
        self.counts = dict(exact_items=0, sigma_items=0, sigma_arcs=0, refused_items=0)

    def has_sigma(self, state):  # :33-45
        if self.sigma_label != NO_LABEL:
            return len(self.matcher.iter(state, self.sigma_label)) > 0
        return False

    def iter(self, state, label):  # IteratorSigmaMatcher::new :190-239, next :296-306
        if label == self.sigma_label and self.sigma_label != NO_LABEL:  # :199-201
            raise SigmaError("SigmaMatcher::Find: bad label (sigma)")
        has_sigma = self.has_sigma(state)  # :204
        exact = self.matcher.iter(state, label)  # :206
        if exact:  # :207-208: sigma_match = NO_LABEL, values pass through (:243-244); next_openfst's branch :272-283 is dead
            if self.sigma_label != NO_LABEL:
                self.counts["exact_items"] += 1
            return exact
        sigma_trs = self.matcher.iter(state, self.sigma_label)  # :210
        if has_sigma and label != EPS_LABEL and label != NO_LABEL:
            if (self.allowed is None or label in self.allowed) and sigma_trs:  # :211-217
                out = []
                for tr in sigma_trs:  # value_openfst :246-266
                    tr = list(tr)
                    if self.rewrite_both:
                        if tr[0] == self.sigma_label:
                            tr[0] = label
                        if tr[1] == self.sigma_label:
                            tr[1] = label
                    elif self.match_type == MATCH_INPUT:
                        tr[0] = label
                    else:
                        tr[1] = label
                    out.append(tr)
                self.counts["sigma_items"] += 1
                self.counts["sigma_arcs"] += len(out)
                return out
            self.counts["refused_items"] += 1
        return []  # find_empty :218-223

    def test_match_type(self, test):  # :122-124
        return self.matcher.test_match_type(test)

    def require_match(self):  # flags(), :126-132
        return self.sigma_label != NO_LABEL

    def priority(self, state):  # :134-144
        if self.sigma_label != NO_LABEL and self.has_sigma(state):
            return "require"
        return self.matcher.priority(state)


def create_matcher(config, fst, match_type):  # compose_static.rs:78-109
    m = SortedMatcher(fst, match_type)
    if config is None:
        return m
    sigma_label, rewrite_mode, allowed = config
    return SigmaMatcher(match_type, sigma_label, rewrite_mode, m, allowed)


def match_type_of(m1, m2):  # ComposeFstOp::match_type, compose_fst_op.rs:169-197
    def known(m, which):  # properties_check on an unknown bit pair: the device's message (compose.hip decide_match_mode)
        t = m.test_match_type(True)
        if t == MATCH_UNKNOWN:
            raise SigmaError("ComposeFst: %s argument: label-sortedness properties are not known (sort?)" % which)
        return t
    if m1.require_match() and known(m1, "1st") != MATCH_OUTPUT:  # :170-174
        raise SigmaError("ComposeFst: 1st argument cannot perform required matching (sort?)")
    if m2.require_match() and known(m2, "2nd") != MATCH_INPUT:  # :175-179
        raise SigmaError("ComposeFst: 2nd argument cannot perform required matching (sort?)")
    type1, type2 = m1.test_match_type(False), m2.test_match_type(False)  # :181-182
    if type1 == MATCH_OUTPUT and type2 == MATCH_INPUT:
        return MATCH_BOTH
    if type1 == MATCH_OUTPUT:
        return MATCH_OUTPUT
    if type2 == MATCH_INPUT:
        return MATCH_INPUT
    if known(m1, "1st") == MATCH_OUTPUT:  # :189-192 (never: test = true reads the same stored word)
        return MATCH_OUTPUT
    if known(m2, "2nd") == MATCH_INPUT:
        return MATCH_INPUT
    raise SigmaError("ComposeFst: 1st argument cannot match on output labels and 2nd argument cannot match on input labels (sort?).")


def set_state(fst1, fst2, s1, s2):  # the epsilon facts every filter's set_state collects (e.g. match_compose_filter.rs:136-161)
    r1, r2 = fst1["rows"][s1], fst2["rows"][s2]
    ne1, ne2 = sum(1 for t in r1 if t[1] == 0), sum(1 for t in r2 if t[0] == 0)
    f1, f2 = fst1["finals"][s1] is not None, fst2["finals"][s2] is not None
    return dict(alleps1=len(r1) == ne1 and not f1, noeps1=ne1 == 0, alleps2=len(r2) == ne2 and not f2, noeps2=ne2 == 0)


def filter_tr(kind, st, fs, arc1, arc2):
    o1, i2 = arc1[1], arc2[0]
    if kind == NULL:  # null_compose_filter.rs:122-129
        return NO_STATE if o1 == NO_LABEL or i2 == NO_LABEL else 0
    if kind == TRIVIAL:  # trivial_compose_filter.rs:122-124
        return 0
    if kind == NO_MATCH:  # no_match_compose_filter.rs:122-126
        return NO_STATE if o1 == EPS_LABEL and i2 == EPS_LABEL else 0
    if kind == SEQUENCE:  # sequence_compose_filter.rs:150-171
        if o1 == NO_LABEL:
            return NO_STATE if st["alleps1"] else (0 if st["noeps1"] else 1)
        if i2 == NO_LABEL:
            return NO_STATE if fs != 0 else 0
        return NO_STATE if o1 == EPS_LABEL else 0
    if kind == ALT_SEQUENCE:  # alt_sequence_compose_filter.rs:159-180
        if i2 == NO_LABEL:
            return NO_STATE if st["alleps2"] else (0 if st["noeps2"] else 1)
        if o1 == NO_LABEL:
            return NO_STATE if fs == 1 else 0
        return NO_STATE if o1 == EPS_LABEL else 0
    assert kind == MATCH  # match_compose_filter.rs:163-206
    if i2 == NO_LABEL:
        if fs == 0:
            return 0 if st["noeps2"] else (NO_STATE if st["alleps2"] else 1)
        return 1 if fs == 1 else NO_STATE
    if o1 == NO_LABEL:
        if fs == 0:
            return 0 if st["noeps1"] else (NO_STATE if st["alleps1"] else 2)
        return 2 if fs == 2 else NO_STATE
    if o1 == EPS_LABEL:
        return 0 if fs == 0 else NO_STATE
    return 0


def compose_properties(p1, p2):  # fst_properties/mutate_properties.rs:151-184
    out = 0
    if p1 & ACCEPTOR and p2 & ACCEPTOR:
        out |= ACCEPTOR | ACCESSIBLE
        out |= (NO_EPSILONS | NO_I_EPSILONS | NO_O_EPSILONS | ACYCLIC | INITIAL_ACYCLIC) & p1 & p2
        if p1 & NO_I_EPSILONS and p2 & NO_I_EPSILONS:
            out |= (I_DETERMINISTIC | O_DETERMINISTIC) & p1 & p2
    else:
        out |= ACCESSIBLE
        out |= (ACCEPTOR | NO_I_EPSILONS | ACYCLIC | INITIAL_ACYCLIC) & p1 & p2
        if p1 & NO_I_EPSILONS and p2 & NO_I_EPSILONS:
            out |= I_DETERMINISTIC & p1 & p2
    return out


def into_tr(item, state, match_type):  # IterItemMatcher::into_tr, matchers/mod.rs:98-105
    if item is EPS_LOOP or item == EPS_LOOP:
        return [NO_LABEL, EPS_LABEL, 0.0, state] if match_type == MATCH_INPUT else [EPS_LABEL, NO_LABEL, 0.0, state]
    return list(item)


def compose_sigma(fst1, fst2, compose_filter=SEQUENCE, connect=True, m1=None, m2=None, info=None):
    """compose_with_config(fst1, fst2, ComposeConfig{compose_filter, matcher1_config: m1, matcher2_config: m2, connect})"""
    matcher1 = create_matcher(m1, fst1, MATCH_OUTPUT)  # compose_static.rs:178-183
    matcher2 = create_matcher(m2, fst2, MATCH_INPUT)
    if compose_filter == AUTO:  # :186-191
        if m1 is None and m2 is None:
            compose_filter = SEQUENCE  # new_auto without look-ahead: compose_fst.rs:58-92
        else:
            raise SigmaError("Custom MatcherConfig not supported with AutoFilter")
    match_type = match_type_of(matcher1, matcher2)  # ComposeFstOp::new, compose_fst_op.rs:152
    # the filters hand the word on (e.g. sequence_compose_filter.rs:193-195): compose_fst_op.rs:154-157
    properties = compose_properties(fst1["props"], fst2["props"])
    counts = dict.fromkeys(COUNTERS, 0)
    out = dict(rows=[], finals=[], start=None, props=NULL_PROPS)  # F2::new(), lazy_fst.rs:227
    if fst1["start"] is not None and fst2["start"] is not None:  # compute_start, compose_fst_op.rs:389-404
        table = {(0, fst1["start"], fst2["start"]): 0}
        tuples = [(0, fst1["start"], fst2["start"])]

        def find_id(t):
            if t not in table:
                table[t] = len(tuples)
                tuples.append(t)
            return table[t]

        level_end, q = 1, 0
        counts["levels"] = 1
        while q < len(tuples):  # lazy_fst.rs:235-259: FIFO, so ids in order
            if q == level_end:
                level_end = len(tuples)
                counts["levels"] += 1
            fs, s1, s2 = tuples[q]
            st = set_state(fst1, fst2, s1, s2)
            # match_input, compose_fst_op.rs:199-219
            if match_type == MATCH_INPUT:
                mi = True
            elif match_type == MATCH_OUTPUT:
                mi = False
            else:
                p1, p2 = matcher1.priority(s1), matcher2.priority(s2)
                if p1 == "require" and p2 == "require":
                    raise SigmaError("Both sides can't require match")
                mi = False if p1 == "require" else (True if p2 == "require" else p1 <= p2)
            counts["require1_states"] += isinstance(matcher1, SigmaMatcher) and matcher1.has_sigma(s1)
            counts["require2_states"] += isinstance(matcher2, SigmaMatcher) and matcher2.has_sigma(s2)
            # ordered_expand :221-265
            sa, sb = (s2, s1) if mi else (s1, s2)
            matcher, it_fst = (matcher2, fst1) if mi else (matcher1, fst2)
            mt = MATCH_INPUT if mi else MATCH_OUTPUT
            tr_loop = [EPS_LABEL, NO_LABEL, 0.0, sb] if mi else [NO_LABEL, EPS_LABEL, 0.0, sb]
            trs = []
            for tr in [tr_loop] + [list(t) for t in it_fst["rows"][sb]]:
                label = tr[1] if mi else tr[0]  # match_tr :333
                for item in matcher.iter(sa, label):  # match_tr_selected :287-322
                    arca, arcb = into_tr(item, sa, mt), list(tr)
                    arc1, arc2 = (arcb, arca) if mi else (arca, arcb)
                    nfs = filter_tr(compose_filter, st, fs, arc1, arc2)
                    if nfs is not NO_STATE:  # add_tr :267-285
                        trs.append([arc1[0], arc2[1], times(arc1[2], arc2[2]), find_id((nfs, arc1[3], arc2[3]))])
            out["rows"].append(trs)
            # compute_final_weight :420-449 (no filter touches the weights)
            w1, w2 = fst1["finals"][s1], fst2["finals"][s2]
            out["finals"].append(None if w1 is None or w2 is None else times(w1, w2))
            q += 1
        out["start"] = 0
        out["props"] = properties
        counts["states"] = len(out["rows"])
        counts["arcs"] = sum(len(r) for r in out["rows"])
        for m in (matcher1, matcher2):
            if isinstance(m, SigmaMatcher):
                for k, v in m.counts.items():
                    counts[k] += v
    if info is not None:
        info.update(counts)
    if connect:  # compose_static.rs:261-263
        model_connect(out)
    return out


def expand_sigma(g, sigma_label, rewrite_mode, allowed, labels):
    """g (the sigma operand on side 2, ilabel-sorted) with every sigma arc replaced by its rewritten copies, in order, for
    every non-zero label of `labels` (ascending) that the allowed set admits and the state does not carry explicitly on its
    input tape; then stably ilabel-sorted.  What the plain composition needs in place of the matcher."""
    rewrite_both = {0: bool(g["props"] & ACCEPTOR), 1: True, 2: False}[rewrite_mode]
    allowed = set(allowed) if allowed else None
    rows = []
    for row in g["rows"]:
        explicit = {t[0] for t in row}
        new = []
        for t in row:
            if t[0] != sigma_label:
                new.append(list(t))
                continue
            for lab in sorted(set(labels)):
                if lab in (EPS_LABEL, NO_LABEL) or lab == sigma_label or lab in explicit or (allowed is not None and lab not in allowed):
                    continue
                il, ol = lab, t[1]
                if rewrite_both and ol == sigma_label:
                    ol = lab
                new.append([il, ol, t[2], t[3]])
        new.sort(key=lambda t: t[0])  # (stable)
        rows.append(new)
    return dict(rows=rows, finals=list(g["finals"]), start=g["start"], props=g["props"])
