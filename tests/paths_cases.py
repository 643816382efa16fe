"""Input machines of the paths tests (tests/test_paths.py on the CPU, tests/test_paths_gpu.py and tests/test_paths_limits.py
on the device): the hand-made edge machines, the seeded random DAGs and the shapes at the walk's and the batch's limits."""
import json
import os

import numpy as np

import helpers
from helpers import _flat, finals_of, fst
from rustfst_amd import synth

INF = float("inf")
ACYCLIC, CYCLIC = 0x0000000800000000, 0x0000000400000000  # properties.rs:60-63
BATCH_MAX_STATES, BATCH_MAX_ARCS = 4096, 16384              # WFST_PATHS_BATCH_MAX_STATES / _ARCS (include/wfst.h)


def golden_cases():
    with open(os.path.join(helpers.GOLDEN_DIR, "k23_paths.json")) as f:
        return json.load(f)["cases"]


def golden_flat(case):
    m = case["input"]
    return _flat(len(m["rows"]), m["start"], [[tuple(a) for a in row] for row in m["rows"]],
                 [INF if w is None else w for w in m["finals"]])


def golden_rows(case):
    return [(tuple(p["ilabels"]), tuple(p["olabels"]), np.float32(p["weight"])) for p in case["paths"]]


def small_machines():
    """name -> acyclic (from the start) flat FST"""
    m = {}
    m["empty"] = helpers.empty_flat()
    m["no_start"] = _flat(2, None, [[(1, 1, 0.5, 1)], []], [INF, 0.0])
    m["lone_final_start"] = fst([[]], [2.5])
    m["lone_nonfinal_start"] = fst([[]], [INF])
    m["linear"] = helpers.wstring([153, 45, 96], [0.25, 0.5, 1.0], 0.125)
    # unequal tape lengths: epsilons on either tape, and an arc with both
    m["unequal_tapes"] = fst([[(1, 0, 0.5, 1), (0, 2, 0.25, 2)], [(0, 0, 1.0, 2), (3, 4, 0.5, 2)], []], [INF, 1.5, 0.75])
    # parallel arcs to one state, identical ones among them
    m["parallel"] = fst([[(1, 1, 1.0, 1), (1, 1, 1.0, 1), (2, 2, 0.5, 1)], [(3, 3, 0.0, 2), (3, 3, 0.0, 2)], []], [INF, INF, 0.0])
    # branches that reach no final state (states 2, 3), one of them the first arc of the start state
    m["non_coaccessible"] = fst([[(9, 9, 0.0, 2), (1, 1, 1.0, 1), (8, 8, 0.0, 3)], [(2, 2, 2.0, 4)], [(7, 7, 0.0, 3)], [], []],
                                [INF, INF, INF, INF, 0.5])
    # equal lengths through different early arcs: the first arc leads to the HIGHER state number, so an order by state
    # number and the lexicographic order of arc positions differ
    m["lex_not_state"] = fst([[(1, 1, 0.0, 3), (2, 2, 0.0, 1), (3, 3, 0.0, 2)],
                              [(4, 4, 0.0, 4), (5, 5, 0.0, 4)], [(6, 6, 0.0, 4)], [(7, 7, 0.0, 4), (8, 8, 0.0, 2)], []],
                             [INF, INF, INF, INF, 0.0])
    # weights: an inf arc on a path, negative weights, and a path whose left-to-right f32 sum differs from any other
    # association: ((0 + 1e8) + 1) - 1e8) + 1 = 1, while 1e8 - 1e8 + (1 + 1) = 2 and a pairwise tree gives 0
    m["inf_arc"] = fst([[(1, 1, INF, 1), (2, 2, 1.0, 1)], [(3, 3, 0.5, 2)], []], [INF, INF, 0.25])
    m["negative"] = fst([[(1, 1, -1.5, 1), (2, 2, 0.0, 2)], [(3, 3, -0.25, 2)], []], [INF, -2.0, 0.5])
    m["order_of_sum"] = fst([[(1, 1, 1e8, 1)], [(2, 2, 1.0, 2)], [(3, 3, -1e8, 3)], [(4, 4, 1.0, 4)], []], [INF, INF, INF, INF, 0.0])
    m["negative_zero"] = fst([[(1, 1, -0.0, 1)], []], [INF, -0.0])
    # a state reached at two depths (state 2: directly and over state 1), final on the way
    m["two_depths"] = fst([[(1, 1, 0.5, 1), (2, 2, 0.25, 2)], [(3, 3, 0.5, 2)], [(4, 4, 1.0, 3)], []], [INF, INF, 0.75, 0.0])
    # a cycle among states the start does not reach (3 <-> 4), the accessible part acyclic
    m["inaccessible_cycle"] = fst([[(1, 1, 1.0, 1), (2, 2, 2.0, 2)], [(3, 3, 0.5, 2)], [], [(5, 5, 0.0, 4)], [(6, 6, 0.0, 3), (7, 7, 0.0, 1)]],
                                  [INF, INF, 0.0, 0.0, INF])
    return m


def cyclic_machines():
    """name -> flat FST with a cycle that the start state reaches"""
    m = {}
    m["self_loop_on_start"] = fst([[(1, 1, 0.0, 0), (2, 2, 0.0, 1)], []], [INF, 0.0])
    # the cycle 1 <-> 2 reaches no final state; the only successful path avoids it
    m["cycle_without_final"] = fst([[(1, 1, 0.0, 3), (2, 2, 0.0, 1)], [(3, 3, 0.0, 2)], [(4, 4, 0.0, 1)], []], [INF, INF, INF, 0.0])
    m["cycle_behind_final"] = fst([[(1, 1, 0.0, 1)], [(2, 2, 0.0, 2)], [(3, 3, 0.0, 1)]], [INF, 0.0, INF])
    return m


def with_word(flat, bits):
    f = dict(flat)
    f["props"] = (flat["props"] & ~(ACYCLIC | CYCLIC)) | bits
    return f


def random_dag(seed):
    """a seeded DAG of 2 .. 9 states: epsilons on either tape, parallel arcs, dead ends, several final states, an inf
    weight now and then; arcs in no label order"""
    rng = np.random.default_rng(23000 + seed)
    n = int(rng.integers(2, 10))
    f = helpers.random_fst_flat(rng, n, 3, 4, p_eps_i=0.25, p_eps_o=0.25, p_final=0.4, sort="none", acyclic=True)
    arcs = f["arcs"]
    if len(arcs) >= 2 and seed % 3 == 0:  # a parallel arc: the next arc of the same state gets the same destination
        off = f["offsets"]
        for s in range(n):
            if off[s + 1] - off[s] >= 2:
                arcs["nextstate"][off[s] + 1] = arcs["nextstate"][off[s]]
                break
    if len(arcs) and seed % 7 == 0:
        arcs["weight"][int(rng.integers(0, len(arcs)))] = np.inf
    if seed % 5 == 0:
        arcs["weight"] -= np.float32(1.0)  # negative weights
    return f


def fan(n_arcs, tail=2):
    """a start state with n_arcs arcs, alternately to a final sink and to a state with `tail` arcs to that sink: paths of one
    and of two arcs interleave along the start state's arcs"""
    rows = [[(k + 1, k + 1, 0.25 * (k % 5), 1 if k % 2 == 0 else 2) for k in range(n_arcs)], [],
            [(100 + j, 0, 0.5 * j, 1) for j in range(tail)]]
    return fst(rows, [INF, 0.125, INF])


def chain(length):
    """`length` arcs in a row, every 1000th state final as well as the last"""
    f = synth.linear_acceptor_flat(np.arange(1, length + 1, dtype=np.uint32) % 7 + 1, 0.5)
    f["arcs"]["weight"] = (np.arange(length) % 3).astype(np.float32) * np.float32(0.25)
    f["finals"][::1000] = 1.0
    f["props"] = 0
    return f


def diamonds(k):
    """k diamonds in a row: 2^k paths (k = 70: more than a u64 holds)"""
    rows = []
    for d in range(k):
        a = 3 * d
        rows += [[(1, 1, 0.0, a + 1), (2, 2, 0.0, a + 2)], [(3, 3, 0.0, a + 3)], [(4, 4, 0.0, a + 3)]]
    rows.append([])
    return fst(rows, finals_of(3 * k + 1, {3 * k: 0.0}))


def sized(n_states, n_arcs):
    """an acyclic machine of exactly n_states states and n_arcs arcs with six paths: a chain of n_states - 2 arcs into the
    final state n_states - 2, five more arcs parallel to its last one, and the rest of the arcs from the start state to the
    dead state n_states - 1, in front of the chain's arc (the walk has to step over them)"""
    chain_arcs = n_states - 2
    dead = n_arcs - chain_arcs - 5
    assert chain_arcs >= 2 and dead >= 0
    rows = [[(1, 1, 0.25 * (s % 3), s + 1)] for s in range(chain_arcs)] + [[], []]
    rows[0] = [(9, 9, 0.0, n_states - 1)] * dead + rows[0]
    rows[chain_arcs - 1] += [(2 + k, 0, 0.5 * k, n_states - 2) for k in range(5)]
    return fst(rows, finals_of(n_states, {n_states - 2: 0.25}))
