"""top_sort at the limits of its routes.  Every route of top_sort.hip returns the same FST — the one-workgroup narrow kernels,
the device-wide launch per level and phase, the hand-over between them in `auto`, a lane or a whole wave per state — so only
the counters of wfst_ctx_get_top_sort_stats show which one ran.  Every input below sits ON a limit or one step beyond it; each
runs under WFST_TOP_SORT_PATH = auto, narrow and wide, bit-exact against test_top_sort's restatement of the reference, every
counter against a prediction made on the host from the input alone:

  levels, widths    Kahn levels with the super-root in front: a state's level is 1 + the highest level among its predecessors
                    (1 without any); a cyclic input: the levels peeled before the peel runs dry.
  launches          a level is narrow when its width is at most the cap (auto NARROW_STATES, narrow: always, wide: never);
                    a maximal run of narrow levels is one launch per phase, a wide level one launch per phase; four phases
                    (peel, select, sizes, pre), the peel alone on a cyclic input.
  max_tree_depth    from the literal depth-first search: the depth of the deepest state in its forest, roots at 1.
  lift_rows         the least J >= 1 with 2^J >= levels + 1.
  states_compared   states other than the start whose in-arcs come from at least two different states.
  wave_states       states other than the start with WAVE_INDEG in-arcs or more.

Without a GPU: the constants below are the kernels', the shapes sit where they claim, and the prediction agrees with closed
forms written out by hand."""
import os
import re

import numpy as np
import pytest

from oracle import model
from oracle.model import fst_to_flat, top_sort_ref
import helpers
from helpers import assert_flat_identical, dev, make_fst

ROOT = helpers.ROOT
PATHS = ("auto", "narrow", "wide")
NARROW_STATES, WAVE_INDEG, WAVE_ROW = 256, 32, 64  # top_sort.hip
COUNTERS = ("levels", "narrow_launches", "wide_launches", "narrow_levels", "max_level_width", "max_tree_depth", "lift_rows",
            "states_compared", "wave_states", "cyclic")
PHASES = 4


# ---------------------------------------------------------------- the prediction
def kahn_levels(fst):
    """[states of level 1, states of level 2, ...] and the number of states left over (on or behind a cycle)"""
    rows = fst["rows"]
    n = len(rows)
    indeg = [0] * n
    for row in rows:
        for a in row:
            indeg[a[3]] += 1
    level = [s for s in range(n) if indeg[s] == 0]
    levels, done = [], 0
    while level:
        levels.append(level)
        done += len(level)
        nxt = []
        for u in level:
            for a in rows[u]:
                indeg[a[3]] -= 1
                if indeg[a[3]] == 0:
                    nxt.append(a[3])
        level = nxt
    return levels, n - done


def dfs_depths(fst):
    """depth of every state in the forest of the literal search (oracle.model's dfs_top_order, with the parents kept)"""
    rows, start = fst["rows"], fst["start"]
    n = len(rows)
    depth = [0] * n
    for root in [start] + list(range(n)):
        if depth[root]:
            continue
        depth[root] = 1
        stack = [[root, 0]]
        while stack:
            s, pos = stack[-1]
            if pos >= len(rows[s]):
                stack.pop()
                continue
            stack[-1][1] += 1
            t = rows[s][pos][3]
            if not depth[t]:
                depth[t] = depth[s] + 1
                stack.append([t, 0])
    return depth


def predict(fst, path):
    cap = {"auto": NARROW_STATES, "narrow": 1 << 62, "wide": 0}[path]
    levels, left = kahn_levels(fst)
    widths = [len(l) for l in levels]
    narrow = [w <= cap for w in widths]
    narrow_runs = sum(1 for i, x in enumerate(narrow) if x and (i == 0 or not narrow[i - 1]))
    phases = 1 if left else PHASES
    p = dict.fromkeys(COUNTERS, 0)
    p.update(levels=len(levels), narrow_launches=phases * narrow_runs, wide_launches=phases * narrow.count(False),
             narrow_levels=narrow.count(True), max_level_width=max(widths, default=0), cyclic=1 if left else 0)
    if left:
        return p
    sources = [set() for _ in fst["rows"]]
    indeg = [0] * len(fst["rows"])
    for s, row in enumerate(fst["rows"]):
        for a in row:
            sources[a[3]].add(s)
            indeg[a[3]] += 1
    others = [s for s in range(len(fst["rows"])) if s != fst["start"]]
    lift = 1
    while (1 << lift) < len(levels) + 1:
        lift += 1
    p.update(max_tree_depth=max(dfs_depths(fst)), lift_rows=lift, states_compared=sum(1 for s in others if len(sources[s]) >= 2),
             wave_states=sum(1 for s in others if indeg[s] >= WAVE_INDEG))
    return p


# ---------------------------------------------------------------- shapes
class Builder:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.rows = []

    def state(self):
        self.rows.append([])
        return len(self.rows) - 1

    def states(self, k):
        return [self.state() for _ in range(k)]

    def arc(self, s, t, front=False):
        il = int(self.rng.integers(0, 5))
        a = [il, il if self.rng.random() < 0.5 else int(self.rng.integers(0, 5)), float(self.rng.integers(0, 16)) / 8, t]
        self.rows[s].insert(0, a) if front else self.rows[s].append(a)

    def chain(self, head, length):
        """head -> c1 -> .. -> c_length; returns [c1, ..]"""
        out, cur = [], head
        for _ in range(length):
            nxt = self.state()
            self.arc(cur, nxt)
            out.append(nxt)
            cur = nxt
        return out

    def fst(self, start, rename=True):
        """the machine with its states renamed by a random permutation (so that ids say nothing about levels)"""
        n = len(self.rows)
        name = self.rng.permutation(n).tolist() if rename else list(range(n))
        rows = [None] * n
        for s, row in enumerate(self.rows):
            rows[name[s]] = [[il, ol, w, name[t]] for il, ol, w, t in row]
        finals = [float(self.rng.integers(0, 8)) / 4 if self.rng.random() < 0.3 else None for _ in range(n)]
        start = n - 1 if start == "last" else name[start]
        return make_fst(rows, finals, start)


def layers(widths, seed, start=0, fan_in=3):
    """layer k has widths[k] states; every state of layer k > 0 has fan_in in-arcs from layer k - 1 (so its level is k + 1)
    and now and then one from further back"""
    b = Builder(seed)
    ls = [b.states(w) for w in widths]
    for k in range(1, len(ls)):
        for t in ls[k]:
            for _ in range(fan_in):
                b.arc(ls[k - 1][int(b.rng.integers(0, len(ls[k - 1])))], t)
            if k > 1 and b.rng.random() < 0.3:
                far = ls[int(b.rng.integers(0, k - 1))]
                b.arc(far[int(b.rng.integers(0, len(far)))], t)
    for row in b.rows:
        b.rng.shuffle(row)
    return b.fst(start)


def fan(k, seed):
    """one state with k arcs, one to each of k states: the widest single row"""
    b = Builder(seed)
    root = b.state()
    for t in b.states(k):
        b.arc(root, t)
    return b.fst(root)


def no_arcs(n, seed, start=0):
    b = Builder(seed)
    b.states(n)
    return b.fst(start)


def late_join(depth, seed, roots, short=None):
    """two chains of `depth` states (the second `short` states if given) and one state both ends lead into.  roots = 1: the
    chains hang on one state, roots = 2: each chain begins at a root of its own, so the candidates meet at the super-root"""
    b = Builder(seed)
    if roots == 1:
        r = b.state()
        a = b.chain(r, depth)
        c = b.chain(r, depth if short is None else short)
        start = r
    else:
        ra, rc = b.state(), b.state()
        a = [ra] + b.chain(ra, depth - 1)
        c = [rc] + b.chain(rc, (depth if short is None else short) - 1)
        start = rc
    j = b.state()
    b.arc(c[-1], j)
    b.arc(a[-1], j)
    b.chain(j, 2)
    return b.fst(start)


def ancestor_join(depth, k, seed, front):
    """a chain r = c0 -> c1 -> .. -> c_depth and a state with in-arcs from c_depth and from its ancestor c_k, whose arc into
    the join comes before (front) or after the chain's arc in c_k's row"""
    b = Builder(seed)
    r = b.state()
    c = [r] + b.chain(r, depth)
    j = b.state()
    b.arc(c[-1], j)
    b.arc(c[k], j, front=front)
    b.chain(j, 1)
    return b.fst(r)


def in_degree(d, seed, distinct):
    """a state with d in-arcs: from d different states (distinct) or all from two states; the sources hang on chains of
    different lengths below one root, so the comparisons lift"""
    b = Builder(seed)
    r = b.state()
    j = b.state()
    if distinct:
        for i in range(d):
            b.arc((b.chain(r, 1 + i % 3))[-1], j)
    else:
        u, v = b.chain(r, 2)[-1], b.chain(r, 1)[-1]
        for i in range(d):
            b.arc(u if i % 3 else v, j)
    b.chain(j, 1)
    for row in b.rows:
        b.rng.shuffle(row)
    return b.fst(r)


def row_length(k, seed):
    """a state with a row of k arcs into k // 2 + 1 states (doubled arcs), a third of which an earlier root's chain has taken
    before; every target has a subtree of its own, so the preorder numbers along the row are uneven"""
    b = Builder(seed)
    early, r = b.state(), b.state()
    targets = b.states(k // 2 + 1)
    for i in range(k):
        b.arc(r, targets[i % len(targets)])
    b.rng.shuffle(b.rows[r])
    for i, t in enumerate(targets):
        if i % 3 == 0:
            b.arc(early, t)
        b.chain(t, i % 4)
    return b.fst(r, rename=False)


def cyclic(kind, seed):
    b = Builder(seed)
    r = b.state()
    if kind == "self_loop_at_the_start":
        b.arc(r, r)
        return b.fst(r)
    if kind == "first_level":  # no state is without an in-arc: the peel has no level 1
        x = b.chain(r, 3)
        b.arc(x[-1], r)
        return b.fst(r)
    if kind == "last_level":
        x = b.chain(r, 6)
        y = b.chain(x[-1], 2)
        b.arc(y[-1], y[0])
        return b.fst(r)
    if kind == "unreachable":
        b.chain(r, 4)
        u = b.state()
        y = b.chain(u, 2)
        b.arc(y[-1], u)
        return b.fst(r)
    assert kind == "behind_a_wide_level"
    for t in b.states(NARROW_STATES + 1):
        b.arc(r, t)
    y = b.chain(len(b.rows) - 1, 2)
    b.arc(y[-1], y[0])
    return b.fst(r)


POW2 = [d for k in range(2, 6) for d in (2 ** k - 1, 2 ** k, 2 ** k + 1)]
DEPTHS = sorted(set([1, 2, 3, 4, 5, 8, 9] + POW2))
SHAPES = {}
SHAPES.update({f"width_{w}": (lambda w=w: layers([3, w, 2], 11 + w)) for w in (NARROW_STATES, NARROW_STATES + 1)})
SHAPES["narrow_wide_narrow"] = lambda: layers([1, 2, 2, NARROW_STATES + 1, 2, 2, 3], 21)
SHAPES["wide_narrow_wide"] = lambda: layers([NARROW_STATES + 5, 2, 7, NARROW_STATES + 1, NARROW_STATES + 9], 22, start="last")
SHAPES.update({f"fan_{k}": (lambda k=k: fan(k, 30 + k)) for k in (NARROW_STATES, NARROW_STATES + 1)})
SHAPES.update({f"no_arcs_{n}": (lambda n=n: no_arcs(n, 40 + n)) for n in (1, 2, NARROW_STATES, NARROW_STATES + 1)})
SHAPES["no_arcs_start_last"] = lambda: no_arcs(NARROW_STATES + 1, 45, start="last")
SHAPES["layers_start_last"] = lambda: layers([4, 6, 5, 3], 46, start="last")
for d in DEPTHS:
    SHAPES[f"join_below_one_root_depth_{d}"] = lambda d=d: late_join(d, 100 + d, 1)
    SHAPES[f"join_below_two_roots_depth_{d}"] = lambda d=d: late_join(d, 200 + d, 2)
    if d > 1:
        SHAPES[f"join_uneven_depth_{d}"] = lambda d=d: late_join(d, 300 + d, 1, short=(d + 1) // 2)
        SHAPES[f"join_uneven_two_roots_depth_{d}"] = lambda d=d: late_join(d, 350 + d, 2, short=(d + 1) // 2)
        SHAPES[f"ancestor_is_the_root_depth_{d}_front"] = lambda d=d: ancestor_join(d, 0, 400 + d, True)
        SHAPES[f"ancestor_is_the_root_depth_{d}_back"] = lambda d=d: ancestor_join(d, 0, 450 + d, False)
        SHAPES[f"ancestor_halfway_depth_{d}_front"] = lambda d=d: ancestor_join(d, d // 2, 500 + d, True)
        SHAPES[f"ancestor_halfway_depth_{d}_back"] = lambda d=d: ancestor_join(d, d // 2, 550 + d, False)
for d in (WAVE_INDEG - 1, WAVE_INDEG, WAVE_INDEG + 1, 2 * WAVE_INDEG + 1, 3 * 64 + 5):
    SHAPES[f"in_degree_{d}_distinct"] = lambda d=d: in_degree(d, 600 + d, True)
    SHAPES[f"in_degree_{d}_two_sources"] = lambda d=d: in_degree(d, 700 + d, False)
for k in (WAVE_ROW - 1, WAVE_ROW, WAVE_ROW + 1, 2 * WAVE_ROW + 1):
    SHAPES[f"row_length_{k}"] = lambda k=k: row_length(k, 800 + k)
CYCLIC = ("self_loop_at_the_start", "first_level", "last_level", "unreachable", "behind_a_wide_level")
SHAPES.update({f"cyclic_{kind}": (lambda kind=kind: cyclic(kind, 900)) for kind in CYCLIC})


# ================================================================ no GPU
def test_getter_declared_exported_and_bound(wfst_lib):
    import rustfst_amd
    helpers.check_counter_getter(wfst_lib, "wfst_ctx_get_top_sort_stats", COUNTERS, rustfst_amd.Context.top_sort_stats)


def test_constants_are_the_kernels():
    with open(os.path.join(ROOT, "rustfst_amd", "csrc", "top_sort.hip")) as f:
        src = f.read()
    for name, value in (("TOP_SORT_NARROW_STATES", NARROW_STATES), ("TOP_SORT_WAVE_INDEG", WAVE_INDEG), ("TOP_SORT_WAVE_ROW", WAVE_ROW)):
        m = re.search(r"constexpr uint32_t " + name + r" = (\d+);", src)
        assert m and int(m.group(1)) == value, name


def test_shapes_sit_on_their_limits():
    def p(name, path="auto"):
        return predict(SHAPES[name](), path)
    a, b = p(f"width_{NARROW_STATES}"), p(f"width_{NARROW_STATES + 1}")
    assert (a["levels"], a["narrow_launches"], a["wide_launches"], a["narrow_levels"]) == (3, 4, 0, 3)
    assert (b["levels"], b["narrow_launches"], b["wide_launches"], b["narrow_levels"]) == (3, 8, 4, 2)
    assert p(f"width_{NARROW_STATES + 1}", "narrow")["narrow_launches"] == 4 and p(f"width_{NARROW_STATES}", "wide")["wide_launches"] == 12
    c = p("narrow_wide_narrow")
    assert (c["levels"], c["narrow_launches"], c["wide_launches"], c["narrow_levels"], c["lift_rows"]) == (7, 8, 4, 6, 3)
    d = p("wide_narrow_wide")
    assert (d["levels"], d["narrow_launches"], d["wide_launches"], d["narrow_levels"]) == (5, 4, 12, 2)
    assert p(f"fan_{NARROW_STATES + 1}")["max_level_width"] == NARROW_STATES + 1 and p(f"fan_{NARROW_STATES}")["wide_launches"] == 0
    e = p(f"no_arcs_{NARROW_STATES + 1}")
    assert (e["levels"], e["wide_launches"], e["max_tree_depth"], e["lift_rows"], e["states_compared"]) == (1, 4, 1, 1, 0)
    assert p("no_arcs_1") == dict(dict.fromkeys(COUNTERS, 0), levels=1, narrow_launches=4, narrow_levels=1, max_level_width=1,
                                  max_tree_depth=1, lift_rows=1)
    for d in DEPTHS:  # levels = depth + 4: the root, the chains, the join, two states behind it; the join compares
        q = p(f"join_below_one_root_depth_{d}")
        lift = next(j for j in range(1, 10) if 2 ** j >= d + 5)
        assert (q["levels"], q["lift_rows"], q["states_compared"], q["max_tree_depth"]) == (d + 4, lift, 1, d + 4), d
        q = p(f"join_below_two_roots_depth_{d}")
        assert (q["levels"], q["states_compared"], q["max_tree_depth"]) == (d + 3, 1, d + 3), d
    assert len({p(f"join_below_one_root_depth_{d}")["lift_rows"] for d in DEPTHS}) == 4  # 3, 4, 5 and 6 rows
    for d, w in ((WAVE_INDEG - 1, 0), (WAVE_INDEG, 1), (WAVE_INDEG + 1, 1), (2 * WAVE_INDEG + 1, 1)):
        assert p(f"in_degree_{d}_distinct")["wave_states"] == w and p(f"in_degree_{d}_two_sources")["wave_states"] == w
        assert p(f"in_degree_{d}_distinct")["states_compared"] == 1
    for k in (WAVE_ROW - 1, WAVE_ROW, WAVE_ROW + 1, 2 * WAVE_ROW + 1):
        assert max(len(r) for r in SHAPES[f"row_length_{k}"]()["rows"]) == k
    want = dict(self_loop_at_the_start=(0, 0, 0), first_level=(0, 0, 0), last_level=(7, 1, 0), unreachable=(5, 1, 0),
                behind_a_wide_level=(2, 1, 1))
    for kind, (levels, nl, wl) in want.items():
        q = p(f"cyclic_{kind}")
        assert q == dict(dict.fromkeys(COUNTERS, 0), levels=levels, narrow_launches=nl, wide_launches=wl,
                         narrow_levels=levels - wl, max_level_width=q["max_level_width"], cyclic=1), kind


def test_restatement_on_every_shape():
    """the restated result of every acyclic shape is topologically sorted; the cyclic ones come back as they are"""
    for name, make in SHAPES.items():
        m = make()
        got = top_sort_ref(m)
        if name.startswith("cyclic_"):
            assert got["rows"] == m["rows"] and got["props"] == model.CYCLIC | model.NOT_TOP_SORTED, name
        else:
            assert all(ns > s for s, row in enumerate(got["rows"]) for _, _, _, ns in row), name


# ================================================================ on the device
@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
def test_every_shape_on_every_route(gpu_ctx, monkeypatch, path):
    monkeypatch.setenv("WFST_TOP_SORT_PATH", path)
    for name, make in SHAPES.items():
        m = make()
        exp = fst_to_flat(top_sort_ref(m))
        got = dev(m, gpu_ctx).top_sort().to_flat()
        assert_flat_identical(got, exp, f"{name} under {path}", check_props=True)
        assert gpu_ctx.top_sort_stats() == predict(m, path), f"{name} under {path}"


@pytest.mark.gpu
def test_routes_were_taken(gpu_ctx, monkeypatch):
    """the counters tell the routes apart on one input: auto hands over both ways, narrow never launches device-wide, wide
    never launches the one-workgroup kernels"""
    m = SHAPES["narrow_wide_narrow"]()
    seen = {}
    for path in PATHS:
        monkeypatch.setenv("WFST_TOP_SORT_PATH", path)
        dev(m, gpu_ctx).top_sort()
        seen[path] = gpu_ctx.top_sort_stats()
    assert seen["auto"]["narrow_launches"] == 8 and seen["auto"]["wide_launches"] == 4
    assert seen["narrow"]["narrow_launches"] == 4 and seen["narrow"]["wide_launches"] == 0
    assert seen["wide"]["narrow_launches"] == 0 and seen["wide"]["wide_launches"] == 28
