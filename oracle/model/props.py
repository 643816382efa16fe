"""The property word: the bit table (fst_properties/properties.rs), the masks and the rules by which every
mutation and every operation of rustfst updates it (mutate_properties.rs)."""
from .weight import weighted


# ---------------------------------------------------------------- property bits (fst_properties/properties.rs:22-103)
B = dict(ACCEPTOR=16, NOT_ACCEPTOR=17, I_DETERMINISTIC=18, NOT_I_DETERMINISTIC=19, O_DETERMINISTIC=20,
         NOT_O_DETERMINISTIC=21, EPSILONS=22, NO_EPSILONS=23, I_EPSILONS=24, NO_I_EPSILONS=25, O_EPSILONS=26,
         NO_O_EPSILONS=27, I_LABEL_SORTED=28, NOT_I_LABEL_SORTED=29, O_LABEL_SORTED=30, NOT_O_LABEL_SORTED=31,
         WEIGHTED=32, UNWEIGHTED=33, CYCLIC=34, ACYCLIC=35, INITIAL_CYCLIC=36, INITIAL_ACYCLIC=37, TOP_SORTED=38,
         NOT_TOP_SORTED=39, ACCESSIBLE=40, NOT_ACCESSIBLE=41, COACCESSIBLE=42, NOT_COACCESSIBLE=43, STRING=44,
         NOT_STRING=45, WEIGHTED_CYCLES=46, UNWEIGHTED_CYCLES=47)
globals().update({k: 1 << v for k, v in B.items()})


def _m(*names):
    return sum(1 << B[n] for n in names)


LABEL_BITS = ("ACCEPTOR", "NOT_ACCEPTOR", "I_DETERMINISTIC", "NOT_I_DETERMINISTIC", "O_DETERMINISTIC",
              "NOT_O_DETERMINISTIC", "EPSILONS", "NO_EPSILONS", "I_EPSILONS", "NO_I_EPSILONS", "O_EPSILONS",
              "NO_O_EPSILONS", "I_LABEL_SORTED", "NOT_I_LABEL_SORTED", "O_LABEL_SORTED", "NOT_O_LABEL_SORTED")
# properties.rs:166-300 / 436-465
SET_START_MASK = _m(*LABEL_BITS, "WEIGHTED", "UNWEIGHTED", "CYCLIC", "ACYCLIC", "TOP_SORTED", "NOT_TOP_SORTED",
                    "COACCESSIBLE", "NOT_COACCESSIBLE", "WEIGHTED_CYCLES", "UNWEIGHTED_CYCLES")
SET_FINAL_MASK = _m(*LABEL_BITS, "CYCLIC", "ACYCLIC", "INITIAL_CYCLIC", "INITIAL_ACYCLIC", "TOP_SORTED",
                    "NOT_TOP_SORTED", "ACCESSIBLE", "NOT_ACCESSIBLE", "WEIGHTED_CYCLES", "UNWEIGHTED_CYCLES")
ADD_STATE_MASK = _m(*LABEL_BITS, "WEIGHTED", "UNWEIGHTED", "CYCLIC", "ACYCLIC", "INITIAL_CYCLIC", "INITIAL_ACYCLIC",
                    "TOP_SORTED", "NOT_TOP_SORTED", "NOT_ACCESSIBLE", "NOT_COACCESSIBLE", "NOT_STRING",
                    "WEIGHTED_CYCLES", "UNWEIGHTED_CYCLES")
ADD_ARC_MASK = _m("NOT_ACCEPTOR", "NOT_I_DETERMINISTIC", "NOT_O_DETERMINISTIC", "EPSILONS", "I_EPSILONS", "O_EPSILONS",
                  "NOT_I_LABEL_SORTED", "NOT_O_LABEL_SORTED", "WEIGHTED", "CYCLIC", "INITIAL_CYCLIC", "NOT_TOP_SORTED",
                  "ACCESSIBLE", "COACCESSIBLE", "WEIGHTED_CYCLES")
ARC_RELEVANT = _m("ACCEPTOR", "NOT_ACCEPTOR", "EPSILONS", "NO_EPSILONS", "I_EPSILONS", "NO_I_EPSILONS", "O_EPSILONS",
                  "NO_O_EPSILONS", "WEIGHTED", "UNWEIGHTED")
WEIGHT_INVARIANT = _m(*LABEL_BITS, "CYCLIC", "ACYCLIC", "INITIAL_CYCLIC", "INITIAL_ACYCLIC", "TOP_SORTED",
                      "NOT_TOP_SORTED", "ACCESSIBLE", "NOT_ACCESSIBLE", "COACCESSIBLE", "NOT_COACCESSIBLE", "STRING",
                      "NOT_STRING")
DFS_BITS = _m("CYCLIC", "ACYCLIC", "INITIAL_CYCLIC", "INITIAL_ACYCLIC", "ACCESSIBLE", "NOT_ACCESSIBLE", "COACCESSIBLE",
              "NOT_COACCESSIBLE")
ALL = 0x0000FFFFFFFF0000
# properties.rs:283-316, 351-381, 383-432, 469-517
DELETE_STATES = _m("ACCEPTOR", "I_DETERMINISTIC", "O_DETERMINISTIC", "NO_EPSILONS", "NO_I_EPSILONS", "NO_O_EPSILONS",
                   "I_LABEL_SORTED", "O_LABEL_SORTED", "UNWEIGHTED", "ACYCLIC", "INITIAL_ACYCLIC", "TOP_SORTED",
                   "UNWEIGHTED_CYCLES")
DELETE_ARCS = DELETE_STATES | NOT_ACCESSIBLE | NOT_COACCESSIBLE
ARCSORT = ALL & ~(I_LABEL_SORTED | NOT_I_LABEL_SORTED | O_LABEL_SORTED | NOT_O_LABEL_SORTED)
_COMMON_INV = _m("WEIGHTED", "UNWEIGHTED", "CYCLIC", "ACYCLIC", "INITIAL_CYCLIC", "INITIAL_ACYCLIC", "TOP_SORTED",
                 "NOT_TOP_SORTED", "ACCESSIBLE", "NOT_ACCESSIBLE", "COACCESSIBLE", "NOT_COACCESSIBLE", "STRING", "NOT_STRING",
                 "WEIGHTED_CYCLES", "UNWEIGHTED_CYCLES")
I_LABEL_INVARIANT = _COMMON_INV | _m("O_DETERMINISTIC", "NOT_O_DETERMINISTIC", "O_EPSILONS", "NO_O_EPSILONS",
                                     "O_LABEL_SORTED", "NOT_O_LABEL_SORTED")
O_LABEL_INVARIANT = _COMMON_INV | _m("I_DETERMINISTIC", "NOT_I_DETERMINISTIC", "I_EPSILONS", "NO_I_EPSILONS",
                                     "I_LABEL_SORTED", "NOT_I_LABEL_SORTED")
ADD_SUPER_FINAL = _m("NOT_ACCEPTOR", "NOT_I_DETERMINISTIC", "NOT_O_DETERMINISTIC", "EPSILONS", "I_EPSILONS", "O_EPSILONS",
                     "NOT_I_LABEL_SORTED", "NOT_O_LABEL_SORTED", "WEIGHTED", "UNWEIGHTED", "CYCLIC", "ACYCLIC",
                     "INITIAL_CYCLIC", "INITIAL_ACYCLIC", "NOT_TOP_SORTED", "NOT_ACCESSIBLE", "COACCESSIBLE",
                     "NOT_COACCESSIBLE", "NOT_STRING", "WEIGHTED_CYCLES", "UNWEIGHTED_CYCLES")
RM_SUPER_FINAL = _m("ACCEPTOR", "NOT_ACCEPTOR", "I_DETERMINISTIC", "O_DETERMINISTIC", "NO_EPSILONS", "NO_I_EPSILONS",
                    "NO_O_EPSILONS", "I_LABEL_SORTED", "O_LABEL_SORTED", "WEIGHTED", "UNWEIGHTED", "CYCLIC", "ACYCLIC",
                    "INITIAL_CYCLIC", "INITIAL_ACYCLIC", "TOP_SORTED", "ACCESSIBLE", "COACCESSIBLE", "NOT_COACCESSIBLE",
                    "STRING", "WEIGHTED_CYCLES", "UNWEIGHTED_CYCLES")
NULL_PROPS = _m("ACCEPTOR", "I_DETERMINISTIC", "O_DETERMINISTIC", "NO_EPSILONS", "NO_I_EPSILONS", "NO_O_EPSILONS",
                "I_LABEL_SORTED", "O_LABEL_SORTED", "UNWEIGHTED", "ACYCLIC", "INITIAL_ACYCLIC", "TOP_SORTED", "ACCESSIBLE",
                "COACCESSIBLE", "STRING", "UNWEIGHTED_CYCLES")
POS, NEG = 0x5555555555555555 & ALL, 0xAAAAAAAAAAAAAAAA & ALL
LABEL_INVARIANT = I_LABEL_INVARIANT & O_LABEL_INVARIANT
# what both operands hand on (mutate_properties.rs:207-220, 717-729)
NEGATIVE = NOT_ACCEPTOR | NOT_I_DETERMINISTIC | NOT_O_DETERMINISTIC | EPSILONS | I_EPSILONS | O_EPSILONS | NOT_I_LABEL_SORTED | \
    NOT_O_LABEL_SORTED | WEIGHTED | WEIGHTED_CYCLES | CYCLIC | NOT_ACCESSIBLE


def known(p):  # fst_properties/utils.rs:4-9 (without the binary bits: the words here carry none)
    return (p & ALL) | ((p & POS) << 1) | ((p & NEG) >> 1)


# ---------------------------------------------------------------- mutate_properties.rs / trs_iter_mut.rs
def p_set_final(p, old, new):  # mutate_properties.rs:15-37 (None = no final weight)
    if old is not None and weighted(old):
        p &= ~WEIGHTED
    if new is not None and weighted(new):
        p = (p | WEIGHTED) & ~UNWEIGHTED
    return p & (SET_FINAL_MASK | WEIGHTED | UNWEIGHTED)


def p_set_weight(p, old, new):  # trs_iter_mut.rs:279-305, 342-350
    if weighted(old):
        p &= ~WEIGHTED
    if weighted(new):
        p = (p | WEIGHTED) & ~UNWEIGHTED
    return p & ARC_RELEVANT


def p_add_state(p):  # :39-41
    return p & ADD_STATE_MASK


def p_add_tr(p, state, tr, prev=None):  # mutate_properties.rs:43-100 (prev: the state's previous arc)
    il, ol, w, ns = tr
    if il != ol:
        p = (p | NOT_ACCEPTOR) & ~ACCEPTOR
    if il == 0:
        p = (p | I_EPSILONS) & ~NO_I_EPSILONS
        if ol == 0:
            p = (p | EPSILONS) & ~NO_EPSILONS
    if ol == 0:
        p = (p | O_EPSILONS) & ~NO_O_EPSILONS
    if prev is not None:
        if prev[0] > il:
            p = (p | NOT_I_LABEL_SORTED) & ~I_LABEL_SORTED
        if prev[1] > ol:
            p = (p | NOT_O_LABEL_SORTED) & ~O_LABEL_SORTED
    if weighted(w):
        p = (p | WEIGHTED) & ~UNWEIGHTED
    if ns <= state:
        p = (p | NOT_TOP_SORTED) & ~TOP_SORTED
    p &= ADD_ARC_MASK | ACCEPTOR | NO_EPSILONS | NO_I_EPSILONS | NO_O_EPSILONS | I_LABEL_SORTED | O_LABEL_SORTED | \
        UNWEIGHTED | TOP_SORTED
    if p & TOP_SORTED:
        p |= ACYCLIC | INITIAL_ACYCLIC
    return p


def p_set_start(p):  # :7-13
    out = p & SET_START_MASK
    if p & ACYCLIC:
        out |= INITIAL_ACYCLIC
    return out


def dfs_bits(facts):
    a, c, cy, ic = facts
    return (ACCESSIBLE if a else NOT_ACCESSIBLE) | (COACCESSIBLE if c else NOT_COACCESSIBLE) | \
        (CYCLIC if cy else ACYCLIC) | (INITIAL_CYCLIC if ic else INITIAL_ACYCLIC)


# ---------------------------------------------------------------- the word of an operation's result
def determinize_props(p, distinct):  # mutate_properties.rs:247-279 with has_subsequential_label = false
    out = ACCESSIBLE
    if p & ACCEPTOR or (p & NO_I_EPSILONS and distinct):
        out |= I_DETERMINISTIC
    out |= (ACCEPTOR | ACYCLIC | INITIAL_ACYCLIC | COACCESSIBLE | STRING) & p
    if p & NO_I_EPSILONS and distinct:
        out |= NO_EPSILONS & p
    if p & ACCESSIBLE:
        out |= (I_EPSILONS | O_EPSILONS | CYCLIC) & p
    if p & ACCEPTOR:
        out |= (NO_I_EPSILONS | NO_O_EPSILONS) & p
    return out


def closure_properties(p):  # mutate_properties.rs:114-145, delayed = false
    out = (ACCEPTOR | UNWEIGHTED | ACCESSIBLE) & p
    if p & UNWEIGHTED:
        out |= UNWEIGHTED_CYCLES
    out |= (COACCESSIBLE | NOT_TOP_SORTED | NOT_STRING) & p
    out |= (NOT_ACCEPTOR | NOT_I_DETERMINISTIC | NOT_O_DETERMINISTIC | NOT_I_LABEL_SORTED | NOT_O_LABEL_SORTED | WEIGHTED |
            WEIGHTED_CYCLES | NOT_ACCESSIBLE | NOT_COACCESSIBLE) & p
    if p & WEIGHTED and p & ACCESSIBLE and p & COACCESSIBLE:
        out |= WEIGHTED_CYCLES
    return out


def concat_properties(p1, p2):  # mutate_properties.rs:186-245, delayed = false
    out = (ACCEPTOR | UNWEIGHTED | UNWEIGHTED_CYCLES | ACYCLIC) & p1 & p2
    out |= (NOT_TOP_SORTED | NOT_STRING) & p1
    out |= (NOT_TOP_SORTED | NOT_STRING) & p2
    out |= (INITIAL_ACYCLIC | INITIAL_CYCLIC) & p1
    out |= (NEGATIVE | NOT_COACCESSIBLE) & p1
    if p1 & ACCESSIBLE and p1 & COACCESSIBLE:
        out |= ACCESSIBLE & p2
        out |= COACCESSIBLE & p2
        out |= (NEGATIVE | NOT_COACCESSIBLE) & p2
    return out


def union_properties(p1, p2):  # mutate_properties.rs:692-748, delayed = false
    out = (ACCEPTOR | UNWEIGHTED | UNWEIGHTED_CYCLES | ACYCLIC | ACCESSIBLE) & p1 & p2
    out |= INITIAL_ACYCLIC
    out |= NOT_TOP_SORTED & p1
    out |= NOT_TOP_SORTED & p2
    out |= EPSILONS | I_EPSILONS | O_EPSILONS
    out |= COACCESSIBLE & p1 & p2
    out |= NEGATIVE & p1
    out |= (NEGATIVE | NOT_COACCESSIBLE) & p2
    return out
