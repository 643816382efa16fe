"""Inputs and expectations of the fused batch with a sigma matcher (tests/test_sigma_batch.py on the CPU,
tests/test_sigma_batch_gpu.py on the device): K21's three utterances, the seeded batches and the hand-built machines at the
limits of string_sigma_sp_kernel.  FSTs are in the rows form of oracle.model, matcher configs are sigma_ref's
(sigma_label, rewrite_mode, allowed).  What the kernel is expected to do with an item is stated here from the restatement
alone (tests/sigma_ref.py): the widths of the BFS levels of R.compose_sigma and its number of states."""
import functools

import numpy as np

from oracle.model import flat_to_fst, rows_flat

import helpers
import sigma_cases as S
import sigma_ref as R

INF = np.inf
WIDTH = 64    # states of a BFS level the kernel holds: one per lane
SLICE = 512   # composed states a wave's slice of LDS holds for acceptors of at most 224 states (2 * states + 64 <= 512)
SIZES = (1, 17, 65)
RW_ACC = [(rw, acc) for rw in (0, 1, 2) for acc in (False, True)]
THOUSAND = [2 * x for x in range(1, 1001)]


def weighted_string(labels, weights=None, final=0.0):
    """utils::acceptor with weights: a linear, epsilon-free acceptor"""
    n = len(labels)
    w = weights if weights is not None else [0.0] * n
    return S.machine([[(int(l), int(l), float(w[i]), i + 1)] for i, l in enumerate(labels)] + [[]], [INF] * n + [final])


def level_widths(fst):
    """states per BFS level of a composition (R.compose_sigma numbers the states level by level)"""
    if fst["start"] is None:
        return []
    level = {fst["start"]: 0}
    order = [fst["start"]]
    for s in order:
        for t in fst["rows"][s]:
            if t[3] not in level:
                level[t[3]] = level[s] + 1
                order.append(t[3])
    widths = [0] * (max(level.values()) + 1)
    for v in level.values():
        widths[v] += 1
    return widths


def reference(a, t, m2, flt=R.SEQUENCE, m1=None):
    """(composition before connect or the error's message, the restatement's counters, level widths)"""
    info = {}
    try:
        c = R.compose_sigma(a, t, flt, False, m1, m2, info)
    except R.SigmaError as e:
        return e.args[0], None, None
    return c, info, level_widths(c)


def in_kernel(info, widths):
    """the kernel answers the item: no level wider than a wave, no more composed states than the slice"""
    return max(widths) <= WIDTH and info["states"] <= SLICE


def expected_path(oracle, c):
    """shortest_path of a composition, by the oracle (the canonical predecessor is the reference's on these lattices)"""
    from oracle.model import fst_to_flat
    return helpers.to_oracle(oracle, fst_to_flat(c)).shortest_path_canonical().to_flat()


# ---------------------------------------------------------------- K21
def k21_batch():
    """(utterances, grammar, m2): bowie, radiohead and queen under the allowed set {radiohead, queen}"""
    k = S.k21()
    by_name = {c["name"]: c for c in k["cases"]}
    names = ("bowie_refused", "radiohead_allowed", "queen_allowed")
    return [S.from_spec(by_name[n]["query"]) for n in names], S.from_spec(k["grammar_sigma"]), (1, k["rewrite_mode"], [6, 4])


# ---------------------------------------------------------------- seeded batches
def seeded_grammar(seed, acceptor, sigma_low):
    """T: 6-20 states, ilabel-sorted, no input epsilons, labels 2..6 with sigma = 1 below them (sigma_low) or 1..5 with
    sigma = 9 above; most states get a sigma arc next to their exact arcs, some get two"""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(6, 21))
    t = flat_to_fst(helpers.random_fst_flat(rng, n, 3, 5, p_eps_i=0.0, p_eps_o=0.15, p_final=0.4, sort="none", min_fanout=1))
    shift, sigma = (1, 1) if sigma_low else (0, 9)
    for r in t["rows"]:
        for a in r:
            a[0] += shift
            a[1] += shift if a[1] else 0
    for r in t["rows"]:
        u = rng.random()
        for _ in range(2 if u < 0.25 else (1 if u < 0.8 else 0)):
            ol = [sigma, int(rng.integers(1, 7)), 0][int(rng.integers(0, 3))]
            r.append([sigma, ol, float(rng.integers(0, 2560)) / 512, int(rng.integers(0, n))])
    if acceptor:
        t["rows"] = [[[a[0], a[0], a[2], a[3]] for a in r] for r in t["rows"]]
    t = S._sorted_rows(t, 0)
    assert any(any(a[0] == sigma for a in r) and any(a[0] != sigma for a in r) for r in t["rows"])
    assert any(sum(a[0] == sigma for a in r) == 2 for r in t["rows"])
    assert all(a[0] != 0 for r in t["rows"] for a in r)
    return S.with_sort_word(t, acceptor), sigma


def seeded_strings(seed, n, sigma):
    """n strings of 0-12 labels over 1..8 without sigma: labels 7 and 8 are on no arc of T"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        length = int(rng.integers(0, 13))
        labels = [int(x) for x in rng.integers(1, 9, length)]
        labels = [l if l != sigma else 7 for l in labels]
        out.append(weighted_string(labels, [float(rng.integers(0, 2560)) / 512 for _ in labels], float(rng.integers(0, 512)) / 512))
    return out


@functools.lru_cache(maxsize=None)
def seeded_cases():
    """[(name, strings, T, m2)]: the three rewrite modes x acceptor / transducer T, each with batches of 1, 17 and 65; sigma
    below / above the labels alternates with the grammar, the allowed set (none, one label, a thousand) with the batch"""
    allowed = (None, [7], THOUSAND)
    out = []
    for g, (rw, acc) in enumerate(RW_ACC):
        t, sigma = seeded_grammar(3100 + g, acc, sigma_low=g % 2 == 0)
        for b, size in enumerate(SIZES):
            m2 = (sigma, rw, allowed[(g + b) % 3])
            out.append(("rw%d-%s-sigma%d-n%d-allowed%d" % (rw, "acc" if acc else "tr", sigma, size, (g + b) % 3),
                        seeded_strings(7000 + 10 * g + b, size, sigma), t, m2))
    return out


@functools.lru_cache(maxsize=None)
def seeded_references():
    """name -> [reference(a_i, T, m2)] of every seeded batch: computed once for the CPU and the GPU tests"""
    return {name: [reference(a, t, m2) for a in strs] for name, strs, t, m2 in seeded_cases()}


# ---------------------------------------------------------------- the limits of the kernel
SG = 50


def fan_grammar(n_sigma, n_dest=None):
    """state 0 with n_sigma sigma arcs into n_dest (default: as many) distinct final states, weights that make one of them best"""
    n_dest = n_sigma if n_dest is None else n_dest
    row = [(SG, SG, 0.25 * ((7 * k) % 11) + 0.5, 1 + k % n_dest) for k in range(n_sigma)]
    return S.machine([row] + [[] for _ in range(n_dest)], [INF] + [0.125 * (k % 5) for k in range(n_dest)])


def slice_grammar(m):
    """state 0 fans out by 63 sigma arcs into states that loop on sigma; m of them leave on label 7 for one shared state:
    nine labels [9] * 8 + [7] compose to 1 + 8 * 63 + (63 - m) + 1 states"""
    rows = [[(SG, SG, 0.25 * (k % 7), 1 + k) for k in range(63)]]
    for k in range(63):
        rows.append(([(7, 7, 0.5, 64)] if k < m else []) + [(SG, SG, 0.125 * (k % 3), 1 + k)])
    rows.append([])
    finals = [INF] + [0.25 * (k % 4) for k in range(63)] + [0.0]
    return S.with_sort_word(flat_to_fst(rows_flat(rows, finals, start=0)), acceptor=True)  # (cyclic: the word of the seeded machines)


SLICE_STRING = [9] * 8 + [7]


def long_block_grammar(n_arcs, sigma_first):
    """(T, sigma): state 0 with n_arcs arcs, three of them sigma arcs at the head of the block (sigma = 50) or at its tail
    (sigma = 5000); the others carry distinct labels except for a run of label 300 at positions 62..66 of the block, across
    the boundary of the first 64-arc chunk (as far as the block reaches); everything lands in five final states"""
    sigma, offset = (50, 3) if sigma_first else (5000, 0)
    row = [[sigma, sigma, 1.0 + 0.25 * k, 1 + k] for k in range(3)] if sigma_first else []
    for j in range(n_arcs - 3):
        pos = j + offset
        label = 300 if 62 <= pos <= 66 else (100 + j if pos < 62 else 400 + j)
        row.append([label, 1000 + j, 0.125 * ((5 * j) % 13), 1 + j % 5])
    if not sigma_first:
        row += [[sigma, sigma, 1.0 + 0.25 * k, 1 + k] for k in range(3)]
    assert len(row) == n_arcs and all(row[k][0] <= row[k + 1][0] for k in range(n_arcs - 1))
    return S.machine([row] + [[] for _ in range(5)], [INF] + [0.5 * k for k in range(5)]), sigma


def tie_grammar():
    """two frontier states whose sigma arcs reach one destination with equal weights: olabels 5 and 6 tell the parents apart"""
    return S.machine([[(2, 2, 1.0, 1), (2, 2, 1.0, 2)], [(SG, 5, 1.0, 3)], [(SG, 6, 1.0, 3)], []], [INF, INF, INF, 0.0])


def nonlinear_acceptor():
    return S.machine([[(2, 2, 0.5, 1), (2, 2, 0.25, 2)], [(3, 3, 0.0, 3)], [(6, 6, 0.0, 3)], [(5, 5, 0.0, 4)], []], [INF, INF, INF, INF, 0.0])
