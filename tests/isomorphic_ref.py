"""rustfst's isomorphic_with_config, tr_compare, invert and invert_properties restated in sequential Python, line by line:
what the device results of tests/test_isomorphic*.py and tests/test_invert_gpu.py are compared with.  isomorphic
(algorithms/isomorphic.rs:11-158, 200-212) is the FIFO search itself: a deque, state_pairs indexed by the states of fst1, the
non_det flag.  FSTs are in the rows form of oracle.model (dict(rows, finals, start, props)); weights are float32.

One convention is the handle's, not the reference's: a final weight of +inf is "not final" (None), as everywhere in the
library under test, so the reference's (Some(inf), Some(inf)) case does not occur.

`info`, a dict, receives what the tests count: pairs popped, levels of the search, the widest level, arc slots of the popped
pairs' fst1 states (the counters of wfst_ctx_get_isomorphic_counters that do not depend on the route), and the times the mark
was set (the device's nondet_marks where the verdict is 1; a failing level is run to its end there)."""
import functools
import math
from collections import deque

from oracle.model import F32, INF, KDELTA
from oracle.model.props import ALL, B

globals().update({k: 1 << v for k, v in B.items()})  # the property bits by name (fst_properties/properties.rs:22-103)


class IsomorphicError(Exception):
    """the reference's Err (the message in args[0])"""


def approx_equal(a, b, delta):
    """TropicalWeight::approx_equal (semirings/tropical_weight.rs): |a - b| <= delta in f32; false for inf against inf"""
    with _quiet():
        return bool(abs(F32(F32(a) - F32(b))) <= F32(delta))


def _quiet():
    import numpy as np
    return np.errstate(invalid="ignore", over="ignore")


def ordered_float_cmp(a, b):
    """OrderedFloat's Ord: -0.0 == +0.0, NaN greatest and equal to itself"""
    a, b = float(a), float(b)
    if math.isnan(a) or math.isnan(b):
        return (1 if math.isnan(a) else 0) - (1 if math.isnan(b) else 0)
    return -1 if a < b else (1 if a > b else 0)


def tr_compare(tr_1, tr_2):  # isomorphic.rs:22-48
    if tr_1[0] < tr_2[0]:
        return -1
    if tr_1[0] > tr_2[0]:
        return 1
    if tr_1[1] < tr_2[1]:
        return -1
    if tr_1[1] > tr_2[1]:
        return 1
    c = ordered_float_cmp(tr_1[2], tr_2[2])
    if c:
        return c
    if tr_1[3] < tr_2[3]:
        return -1
    if tr_1[3] > tr_2[3]:
        return 1
    return 0


def _final(fst, s):
    w = fst["finals"][s]
    return None if w is None or F32(w) == INF else F32(w)


class Isomorphism:  # isomorphic.rs:11-19, 50-61
    def __init__(self, fst_1, fst_2, delta, info):
        self.fst_1, self.fst_2, self.delta = fst_1, fst_2, delta
        self.state_pairs = [None] * len(fst_1["rows"])
        self.queue = deque()
        self.non_det = False
        self.info = info
        self.depth = {}  # (tests) the level of every queued pair

    def pair_state(self, s1, s2, level):  # :64-73
        if self.state_pairs[s1] == s2:
            return True  # already seen this pair
        if self.state_pairs[s1] is not None:
            return False  # s1 already paired with another s2
        self.state_pairs[s1] = s2
        self.queue.append((s1, s2))
        self.depth[(s1, s2)] = level
        return True

    def ismorphic_state(self, s1, s2):  # :75-132
        fw1, fw2 = _final(self.fst_1, s1), _final(self.fst_2, s2)
        if fw1 is not None and fw2 is not None:
            fw_equal = approx_equal(fw1, fw2, self.delta)
        else:
            fw_equal = fw1 is None and fw2 is None
        if not fw_equal:
            return False
        if len(self.fst_1["rows"][s1]) != len(self.fst_2["rows"][s2]):
            return False
        key = functools.cmp_to_key(tr_compare)
        trs1 = sorted(self.fst_1["rows"][s1], key=key)  # (sort_by is stable, like sorted)
        trs2 = sorted(self.fst_2["rows"][s2], key=key)
        level = self.depth[(s1, s2)] + 1
        for i in range(len(trs1)):
            arc1, arc2 = trs1[i], trs2[i]
            if arc1[0] != arc2[0]:
                return False
            if arc1[1] != arc2[1]:
                return False
            if not approx_equal(arc1[2], arc2[2], self.delta):
                return False
            if not self.pair_state(arc1[3], arc2[3], level):
                return False
            if i > 0:
                arc0 = trs1[i - 1]
                if arc1[0] == arc0[0] and arc1[1] == arc0[1] and approx_equal(arc1[2], arc0[2], self.delta):
                    self.non_det = True
                    self.info["nondet_marks"] = self.info.get("nondet_marks", 0) + 1
        return True

    def isomorphic(self):  # :134-158
        if self.fst_1["start"] is None and self.fst_2["start"] is None:
            return True
        if self.fst_1["start"] is None or self.fst_2["start"] is None:
            return False
        self.pair_state(self.fst_1["start"], self.fst_2["start"], 1)
        widths = {}
        while self.queue:
            s1, s2 = self.queue.popleft()
            lvl = self.depth[(s1, s2)]
            widths[lvl] = widths.get(lvl, 0) + 1
            self.info["pairs"] = self.info.get("pairs", 0) + 1
            self.info["events"] = self.info.get("events", 0) + len(self.fst_1["rows"][s1])
            self.info["levels"], self.info["max_level_width"] = max(widths), max(widths.values())
            if not self.ismorphic_state(s1, s2):
                # (the device runs the failing level to its end: what is queued on that level counts there)
                rest = [p for p in self.queue if self.depth[p] == lvl]
                self.info["pairs"] += len(rest)
                self.info["events"] += sum(len(self.fst_1["rows"][p[0]]) for p in rest)
                self.info["max_level_width"] = max(self.info["max_level_width"], widths[lvl] + len(rest))
                if self.non_det:
                    raise IsomorphicError("Isomorphic: Non-determinism as an unweighted automaton. state1 = %d state2 = %d" % (s1, s2))
                return False
        return True


def isomorphic(fst_1, fst_2, delta=KDELTA, info=None):
    """isomorphic_with_config (isomorphic.rs:200-212): True / False, or raises IsomorphicError"""
    return Isomorphism(fst_1, fst_2, delta, {} if info is None else info).isomorphic()


def verdict(fst_1, fst_2, delta=KDELTA, info=None):
    """1, 0 or the error's message"""
    try:
        return 1 if isomorphic(fst_1, fst_2, delta, info) else 0
    except IsomorphicError as e:
        return e.args[0]


def invert_properties(inprops):  # fst_properties/mutate_properties.rs:302-363
    outprops = (ACCEPTOR | NOT_ACCEPTOR | EPSILONS | NO_EPSILONS | WEIGHTED | UNWEIGHTED | WEIGHTED_CYCLES | UNWEIGHTED_CYCLES
                | CYCLIC | ACYCLIC | INITIAL_CYCLIC | INITIAL_ACYCLIC | TOP_SORTED | NOT_TOP_SORTED | ACCESSIBLE | NOT_ACCESSIBLE
                | COACCESSIBLE | NOT_COACCESSIBLE | STRING | NOT_STRING) & inprops
    if inprops & I_DETERMINISTIC:
        outprops |= O_DETERMINISTIC
    if inprops & NOT_I_DETERMINISTIC:
        outprops |= NOT_O_DETERMINISTIC
    if inprops & O_DETERMINISTIC:
        outprops |= I_DETERMINISTIC
    if inprops & NOT_O_DETERMINISTIC:
        outprops |= NOT_I_DETERMINISTIC
    if inprops & I_EPSILONS:
        outprops |= O_EPSILONS
    if inprops & NO_I_EPSILONS:
        outprops |= NO_O_EPSILONS
    if inprops & O_EPSILONS:
        outprops |= I_EPSILONS
    if inprops & NO_O_EPSILONS:
        outprops |= NO_I_EPSILONS
    if inprops & I_LABEL_SORTED:
        outprops |= O_LABEL_SORTED
    if inprops & NOT_I_LABEL_SORTED:
        outprops |= NOT_O_LABEL_SORTED
    if inprops & O_LABEL_SORTED:
        outprops |= I_LABEL_SORTED
    if inprops & NOT_O_LABEL_SORTED:
        outprops |= NOT_I_LABEL_SORTED
    return outprops


def invert(fst):  # algorithms/inversion.rs:32-48: a new FST in the rows form (the reference works in place)
    return dict(rows=[[[tr[1], tr[0], tr[2], tr[3]] for tr in row] for row in fst["rows"]], finals=list(fst["finals"]),
                start=fst["start"], props=invert_properties(fst["props"] & ALL))
