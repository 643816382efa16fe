"""Input families of tr_sum, tr_unique and optimize that more than one test module uses."""
import json
import os

import numpy as np

from oracle.model import ACCESSIBLE, ACYCLIC, INF, content_word_of_flat, rows_flat
from helpers import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "k17_optimize.json")


def golden_cases():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def part_a_rows():
    """degrees at every path boundary; duplicate runs across a chunk boundary and over a whole state"""
    rng = np.random.default_rng(5)
    n = 24

    def rnd(k, dup=0.5, sigma=6):
        row = []
        for _ in range(k):
            if row and rng.random() < dup:
                il, ol, _, ns = row[int(rng.integers(0, len(row)))]
            else:
                il, ol, ns = int(rng.integers(0, sigma)), int(rng.integers(0, sigma)), int(rng.integers(0, n))
            row.append((il, ol, float(rng.integers(0, 8)) / 4, ns))
        return row
    rows = [[], rnd(1), rnd(16), rnd(17), rnd(256), rnd(257), rnd(300), rnd(300, dup=0.0, sigma=1000)]
    rows.append([(3, 3, float(8 - i % 8), 2) for i in range(40)])                    # a run that covers a whole state
    rows.append([(2, 2, float(i % 5), 1) for i in range(300)])                       # ... of a big state
    rows.append([(1, 1, 1.0, 0)] * 10 + [(5, 5, float(20 - i), 3) for i in range(12)] + [(9, 9, 0.0, 1)] * 3)  # run over 16
    rows.append([(i + 1, i + 1, float(i), i % n) for i in range(16)])               # no duplicates
    rows.append([(i + 1, 7, 0.5, 4) for i in range(40)])                            # no duplicates, chunked
    rows.append([(7, 7, 0.25 * (i % 3), 5) for i in range(15)] + [(7, 7, 3.0, 5), (7, 7, 0.0, 5), (8, 8, 1.0, 5)])  # run 15..17
    while len(rows) < n:
        rows.append(rnd(int(rng.integers(0, 20))))
    return rows_flat(rows, [INF] * n)


def part_b_rows():
    """keys that differ in one field only, labels >= 2^31, ilabel 0, signed zeros, +inf, empty states, a run in the last state"""
    big = 0x80000000
    rows = [
        [(5, 2, 1.0, 1), (5, 1, 2.0, 1), (5, 2, 0.5, 1), (5, 1, 3.0, 1)],                      # differ in olabel only
        [],
        [(5, 5, 1.0, 3), (5, 5, 2.0, 2), (5, 5, 0.5, 3), (5, 5, 3.0, 2)],                      # differ in nextstate only
        [(big + 1, 1, 1.0, 0), (1, big, 2.0, 0), (big, big + 7, 0.0, 0), (0xFFFFFFFE, 0, 1.0, 0), (7, 7, 1.0, 0),
         (big + 1, 1, 0.5, 0), (1, big, 2.5, 0)],                                              # unsigned compare
        [],
        [],
        [(0, 0, 1.0, 1), (0, 3, 1.0, 1), (0, 0, 0.5, 1), (3, 0, 2.0, 1), (0, 3, 4.0, 1)],      # ilabel 0
        [(1, 1, 0.0, 0), (1, 1, -0.0, 0), (2, 2, -0.0, 0), (2, 2, 0.0, 0)],                    # ties keep the earlier bits
        [(1, 1, INF, 0), (1, 1, INF, 0), (2, 2, INF, 0), (2, 2, 1.0, 0), (3, 3, 1.0, 0), (3, 3, INF, 0)],
        [(4, 4, 0.0, 2), (4, 4, 0.0009, 2), (4, 4, 0.0018, 2), (4, 4, 0.0027, 2)],             # the KDELTA chain
        [],
        [(6, 6, 2.0, 9), (6, 6, 1.0, 9), (6, 6, 1.0, 9), (6, 6, 3.0, 9)],                      # a run in the LAST state
    ]
    return rows_flat(rows, [INF, 0.0] + [INF] * 9 + [1.5])


def random_arc_lists(seed, n):
    rng = np.random.default_rng(seed)
    rows = []
    for s in range(n):
        row = []
        for _ in range(int(rng.integers(0, 12))):
            if row and rng.random() < 0.5:
                il, ol, _, ns = row[int(rng.integers(0, len(row)))]
            else:
                il, ol, ns = int(rng.integers(0, 4)), int(rng.integers(0, 4)), int(rng.integers(0, n))
            row.append((il, ol, float(rng.integers(0, 64)) / 1024.0 if rng.random() < 0.5 else float(rng.integers(0, 4)), ns))
        rows.append(row)
    return rows_flat(rows, [0.0 if rng.random() < 0.2 else INF for _ in range(n)], props=int(ACYCLIC | ACCESSIBLE))


def optimize_input(rng, n, transducer, deterministic=False, eps=True):
    """an acyclic FST by construction (arcs to higher ids only), integer weights (a grid far coarser than KDELTA), eps:eps
    arcs and parallel arcs; the word is the one computed from its content"""
    rows, finals = [], []
    for s in range(n):
        row = []
        labs = rng.permutation(np.arange(1, 4))
        for k in range(int(rng.integers(1, 4))):  # at least one arc forward: every path ends in the last state, a final one
            if s + 1 >= n:
                break
            il = int(labs[k]) if deterministic else int(rng.integers(1, 4 if transducer else 10))  # nine labels or pairs
            ol = il if not transducer else int(rng.integers(0, 3)) + 4 * il
            t = int(rng.integers(s + 1, min(n, s + 5)))
            row.append((il, ol, float(rng.integers(0, 3)), t))
            if not deterministic and rng.random() < 0.3:  # a parallel arc: tr_sum has work
                row.append((il, ol, float(rng.integers(0, 3)), t))
        if eps and not deterministic and s + 1 < n and rng.random() < 0.2:
            row.append((0, 0, float(rng.integers(0, 2)), int(rng.integers(s + 1, min(n, s + 4)))))
        rows.append(row)
        finals.append(float(rng.integers(0, 2)) if rng.random() < 0.3 or s == n - 1 else INF)
    flat = rows_flat(rows, finals)
    flat["props"] = content_word_of_flat(flat)
    return flat
