"""minimize at the limits of its routes.  Every route of minimize.hip's level loop returns the same FST — the one-workgroup
narrow kernel, the device-wide launches per level, the hand-over between them in `auto`, a lane or a wave per state — so
only the counters of wfst_ctx_get_minimize_stats show which one ran.  Without a GPU: the symbol, the restatement of the
routing (level_profile, predict) against closed forms written out by hand, and every input below on the limit it is built
for (level sizes, degrees, class sizes: all taken from oracle.model's restatement of minimize).  On the device: every input ON a limit and
its twin one step beyond it, bit-exact against minimize_ref, the source handle unchanged, every counter against the
prediction, under WFST_MINIMIZE_PATH = auto, narrow and wide, as an unweighted and as a weighted acceptor.

The inputs are layered DAGs built from TYPES: every level is a list of (count, arc templates, final); an arc template is
(label, level, type) and every state of the type gets that label into SOME state of the target type, taken round-robin, so
that all states of a type are equivalent and, a label 10 + t being its own, two types of one level are not.  Ids are a
random permutation, rows are shuffled.  The weighted variant puts label % 3 on every arc and type % 2 on every final
state: integer weights, equal within a type, so pushing keeps the types together.

unequal_compares is not predicted for the default run: a full compare that finds a difference needs two signatures that
share the upper 32 bits of a 64-bit hash AND meet on one probe chain; which chains meet depends on the insertion order of
concurrent lanes.  test_default_run_records_unequal_compares therefore asserts only that the result is unchanged and
prints the figure.  With WFST_MINIMIZE_HASH_BITS=0 there is a bound that does not depend on the order (test_hash_bits)."""
import collections
import functools
import re

import numpy as np
import pytest
from oracle import model
import helpers
from helpers import assert_flat_identical, to_device
import minimize_cases as mc
from oracle.model import minimize_ref

INF, ACCEPTOR = model.INF, model.ACCEPTOR
PATHS = ("auto", "narrow", "wide")
NARROW_MAX, LANE_MAX_DEG, NARROW_WAVES = 4096, 64, 16  # minimize.hip (a 1024-thread workgroup: 16 waves)
PASS = ("levels", "wide_levels", "narrow_launches", "exit_wide", "exit_done")
COUNTERS = tuple("check_" + k for k in PASS) + PASS + ("branch", "wave_states", "unequal_compares")
PREDICTED = COUNTERS[:-1]
MSG_CYCLIC = "minimize: cyclic inputs are not supported; use rustfst's minimize"
KMAX = 7  # types of a generic level


# ---------------------------------------------------------------- restatement of the routing
def heights(m):
    """(sizes of the levels peeled, sinks first; height of every state, -1 = never peeled) of an fst dict (rows) or a flat
    FST (offsets): run_core's peeling.  A state that lies on or before a cycle is never peeled."""
    if "rows" in m:
        n = len(m["rows"])
        src = np.repeat(np.arange(n, dtype=np.int64), [len(r) for r in m["rows"]])
        dst = np.array([tr[3] for r in m["rows"] for tr in r], dtype=np.int64)
    else:
        n = m["n_states"]
        src = np.repeat(np.arange(n, dtype=np.int64), np.diff(m["offsets"].astype(np.int64)))
        dst = m["arcs"]["nextstate"].astype(np.int64)
    outdeg = np.bincount(src, minlength=n)
    rsrc = src[np.argsort(dst, kind="stable")]
    roff = np.zeros(n + 1, dtype=np.int64)
    roff[1:] = np.cumsum(np.bincount(dst, minlength=n))
    height = np.full(n, -1, dtype=np.int64)
    sizes = []
    frontier = np.nonzero(outdeg == 0)[0]
    while frontier.size:
        height[frontier] = len(sizes)
        sizes.append(int(frontier.size))
        preds = rsrc[np.concatenate([np.arange(roff[s], roff[s + 1]) for s in frontier])]
        np.subtract.at(outdeg, preds, 1)
        cand = np.unique(preds)
        frontier = cand[outdeg[cand] == 0]
    return sizes, height


def level_profile(m):
    return heights(m)[0]


def route(profile, path):
    """the five counters of one pass of run_core over levels of these sizes"""
    s = dict.fromkeys(PASS, 0)
    s["levels"] = len(profile)
    if not profile:
        return s  # (the first read-back finds an empty level: no launch)
    if path == "narrow":
        s.update(narrow_launches=1, exit_done=1)
    elif path == "wide":
        s["wide_levels"] = len(profile)
    else:
        wide = [size > NARROW_MAX for size in profile]
        s["wide_levels"] = sum(wide)
        for i, w in enumerate(wide):
            s["narrow_launches"] += not w and (i == 0 or wide[i - 1])
            s["exit_wide"] += w and i > 0 and not wide[i - 1]
        s["exit_done"] = int(not wide[-1])
    return s


def predict(profile_check, profile_refine, degrees, path, branch=1):
    """every counter but unequal_compares.  profile_check: the levels of the untrimmed input (None: the stored word knows
    ACYCLIC, no check pass); profile_refine, degrees: the levels and the arc counts of the connected machine T (None / ():
    the call never got there)."""
    s = dict.fromkeys(PREDICTED, 0)
    s.update({"check_" + k: v for k, v in route(profile_check or [], path).items()})
    s.update(route(profile_refine or [], path))
    s["branch"] = branch
    s["wave_states"] = sum(d > LANE_MAX_DEG for d in degrees)
    return s


def hand_over_levels(profile):
    """the levels of `auto` that run in another regime than the level before them"""
    wide = [size > NARROW_MAX for size in profile]
    return [i for i in range(1, len(wide)) if wide[i] != wide[i - 1]]


# ---------------------------------------------------------------- generators
def split(count, k):
    return [count // k + (t < count % k) for t in range(k)]


def generic_level(levels, size, covers=None):
    """the types of a level of `size` states above `levels`: min(KMAX, size // 2) types of (nearly) equal size; type t has
    label 1 into type t of the level below (modulo its types), label 10 + t into the next type, and labels 100.. into the
    types c = t (mod this level's types) of every level of `covers` (default: the level below), as often as it takes for
    the states of this type to reach every state of type c."""
    h = len(levels)
    k = max(1, min(KMAX, size // 2))
    counts = split(size, k)
    types = []
    for t in range(k):
        arcs = []
        if h:
            kb = len(levels[h - 1])
            arcs += [(1, h - 1, t % kb), (10 + t, h - 1, (t + 1) % kb)]
            for g in ([h - 1] if covers is None else covers):
                for c in range(t, len(levels[g]), k):
                    for _ in range(-(-levels[g][c][0] // counts[t])):
                        arcs.append((100 + len(arcs), g, c))
        types.append((counts[t], arcs, h == 0))
    return types


def layers(profile, covers=None):
    levels = []
    for h, size in enumerate(profile):
        levels.append(generic_level(levels, size, (covers or {}).get(h)))
    return levels


def instantiate(levels, weighted, seed, props=ACCEPTOR, unreachable_copy_of=None, dead_end=False, in_label_order=None):
    """the flat FST of the typed levels; the one state of the last level is the start.  unreachable_copy_of = (level, type):
    one more state (the highest id) with the row of a state of that type and no arc into it; dead_end: one more state
    without arcs that is not final, under label 5 of the start; in_label_order: a level whose rows are not shuffled."""
    rng = np.random.default_rng(seed)
    n = sum(c for lv in levels for c, _, _ in lv)
    ids = rng.permutation(n)
    members, k = [], 0  # members[level][type]: the ids
    for lv in levels:
        members.append([])
        for count, _, _ in lv:
            members[-1].append([int(x) for x in ids[k:k + count]])
            k += count
    rows, finals = [None] * n, [INF] * n
    used = collections.Counter()
    for h, lv in enumerate(levels):
        for t, (_, arcs, final) in enumerate(lv):
            for s in members[h][t]:
                row = []
                for lab, g, c in arcs:
                    mem = members[g][c]
                    row.append((lab, lab, float(lab % 3) if weighted else 0.0, mem[used[g, c] % len(mem)]))
                    used[g, c] += 1
                rows[s] = row if h == in_label_order else [row[i] for i in rng.permutation(len(row))]
                if final:
                    finals[s] = float(t % 2) if weighted else 0.0
    assert len(members[-1]) == 1 and len(members[-1][0]) == 1
    start = members[-1][0][0]
    if unreachable_copy_of is not None:
        h, t = unreachable_copy_of
        rows.append(list(rows[members[h][t][0]]))
        finals.append(finals[members[h][t][0]])
    if dead_end:
        rows[start] = rows[start] + [(5, 5, 1.0 if weighted else 0.0, len(rows))]
        rows.append([])
        finals.append(INF)
    return dict(model.make_flat(len(rows), start, rows, finals, props), members=members)


TAPER = (300, 9, 1)  # the top of every large profile: 1 start state reaches 9, those 300, those a level of 4097
ALTERNATING = (4097, 5, 4097, 4096, 4097, 4097) + TAPER
ALTERNATING_COVERS = {1: [], 2: [1, 0]}  # (the 5 states cannot reach 4097 sinks with lane degrees: the level above does)
SMALL_ALTERNATING = (41, 5, 41, 40, 41, 41, 9, 1)  # the same shape at a level bound of 40
M1 = 6  # types of the level below the hubs
HUB_DIFF = [(deg, pos, kind) for deg in (65, 128, 129, 200) for pos in sorted({0, 63, 64, deg - 1}) for kind in ("target", "label")]


def hub_arcs(deg, group, pos=None, kind=None):
    """deg arcs, labels 10000 * group + 10 * j into type j % M1 of level 1; (pos, kind): the arc at sorted position pos goes
    into type c + 3 ("target") or carries the label + 3 ("label": still between its neighbours).  Both leave the weighted
    variant's weights as they are: label % 3 is the same, and types c and c + 3 of level 1 lie equally far from a final
    state ((1 + c) % 3), so the twin's pushed weights equal the pair's."""
    arcs = [(10000 * group + 10 * j, 1, j % M1) for j in range(deg)]
    if pos is not None:
        lab, g, c = arcs[pos]
        arcs[pos] = (lab, g, (c + 3) % M1) if kind == "target" else (lab + 3, g, c)
    return arcs


def hub_level(padding):
    """the level of test 6: (types, names).  `padding` lane states more, in 7 types."""
    types, names = [], []

    def add(name, count, arcs, final=False):
        types.append((count, arcs, final))
        names.append(name)
    g = 1
    for deg in (63, 64, 65):  # pairs that merge, not final and final
        add(f"merge_{deg}", 2, hub_arcs(deg, g))
        add(f"merge_{deg}_final", 2, hub_arcs(deg, g + 1), True)
        g += 2
    for deg, pos, kind in HUB_DIFF:  # two that merge, one that differs in exactly one arc
        add(f"diff_{deg}_{pos}_{kind}_a", 2, hub_arcs(deg, g))
        add(f"diff_{deg}_{pos}_{kind}_b", 1, hub_arcs(deg, g, pos, kind))
        g += 1
    for deg in (64, 65):  # differ only in the final weight
        add(f"final_only_{deg}_a", 2, hub_arcs(deg, g))
        add(f"final_only_{deg}_b", 2, hub_arcs(deg, g), True)
        g += 1
    add("prefix_64", 2, hub_arcs(64, g))  # the shorter list is a prefix of the longer one
    add("prefix_65", 2, hub_arcs(65, g))
    g += 1
    for t in range(5):  # plain lane states
        add(f"lane_{t}", 4, [(1, 1, t % M1), (10 + t, 1, (t + 1) % M1), (30, 1, 0)])
    for t, count in enumerate(split(padding, 7) if padding else []):
        add(f"pad_{t}", count, [(2, 1, t % M1), (40 + t, 1, (t + 1) % M1)])
    return types, names


def degree_levels(wide):
    levels = [[(8, [], True)], [(3, [(1 + i, 0, 0)], False) for i in range(M1)]]
    levels.append(hub_level(4100 if wide else 0)[0])
    for size in ((300, 9, 1) if wide else (40, 1)):
        levels.append(generic_level(levels, size))
    return levels


CASES = {
    "one_4096": lambda w: instantiate(layers((300, 4096) + TAPER), w, 1),
    "one_4097": lambda w: instantiate(layers((300, 4097) + TAPER), w, 2),
    "sinks_4097": lambda w: instantiate(layers((4097,) + TAPER), w, 3),
    "sinks_4096": lambda w: instantiate(layers((4096,) + TAPER), w, 4),
    "alternating": lambda w: instantiate(layers(ALTERNATING, ALTERNATING_COVERS), w, 5),
    "small_alternating": lambda w: instantiate(layers(SMALL_ALTERNATING, ALTERNATING_COVERS), w, 6),
    # level 1 holds 4096 states, and one more that nothing reaches: 4097 for the cycle check, 4096 for the refinement
    "check_differs": lambda w: instantiate(layers((300, 4096) + TAPER), w, 7, unreachable_copy_of=(1, 0), dead_end=True),
    "check_skipped": lambda w: instantiate(layers((300, 4096) + TAPER), w, 7, ACCEPTOR | model.ACYCLIC | model.INITIAL_ACYCLIC,
                                           unreachable_copy_of=(1, 0), dead_end=True),
    # (the hubs' rows in label order: a group's labels are its own, so the encode order of the weighted T, the order of first
    # occurrence, is then the label order within a group)
    "degrees_narrow": lambda w: instantiate(degree_levels(False), w, 8, in_label_order=2),
    "degrees_wide": lambda w: instantiate(degree_levels(True), w, 9, in_label_order=2),
}
BRANCH = {"u": 1, "w": 2}


@functools.lru_cache(maxsize=None)
def case(name, kind):
    return CASES[name](kind == "w")


@functools.lru_cache(maxsize=None)
def analysis(name, kind):
    """the restatement's answer and what it saw: dict(exp, T, part, profile_check, profile, height, degrees)"""
    flat = case(name, kind)
    seen = {}
    exp = minimize_ref(flat, partition_out=seen)
    profile, height = heights(seen["T"])
    check = None if model.known(flat["props"]) & model.ACYCLIC else level_profile(flat)
    return dict(exp=exp, T=seen["T"], part=seen["part"], profile_check=check, profile=profile, height=height,
                degrees=[len(r) for r in seen["T"]["rows"]])


def want(name, kind, path):
    an = analysis(name, kind)
    return predict(an["profile_check"], an["profile"], an["degrees"], path, BRANCH[kind])


def classes_of_level(an, h):
    """the restatement's classes of height h of T: {class: [states]}"""
    groups = collections.defaultdict(list)
    for s in np.nonzero(an["height"] == h)[0]:
        groups[an["part"].cls[s]].append(int(s))
    return groups


def refine_profile(name, kind):
    """what the input is built for: the levels of T (weighted: the superfinal state alone below them)"""
    return ([1] if kind == "w" else []) + list(PROFILES[name])


PROFILES = {"one_4096": (300, 4096) + TAPER, "one_4097": (300, 4097) + TAPER, "sinks_4097": (4097,) + TAPER,
            "sinks_4096": (4096,) + TAPER, "alternating": ALTERNATING, "small_alternating": SMALL_ALTERNATING,
            "check_differs": (300, 4096) + TAPER, "check_skipped": (300, 4096) + TAPER}


# ================================================================ no GPU
def test_new_symbol_declared_exported_and_bound(wfst_lib):
    import rustfst_amd
    header = helpers.check_counter_getter(wfst_lib, "wfst_ctx_get_minimize_stats", COUNTERS, rustfst_amd.Context.minimize_stats)
    assert "WFST_MINIMIZE_HASH_BITS" in header


def test_null_ctx_is_ko(wfst_lib):
    helpers.null_ctx_is_ko(wfst_lib, "wfst_ctx_get_minimize_stats", len(COUNTERS))


def _pass(prefix="", **kw):
    s = dict.fromkeys(PASS, 0)
    s.update(kw)
    return {prefix + k: v for k, v in s.items()}


def test_routing_restatement_against_closed_forms():
    # every level narrow: one launch that ends at the empty level
    small = [7, 3, 1]
    assert route(small, "auto") == route(small, "narrow") == _pass(levels=3, narrow_launches=1, exit_done=1)
    assert route(small, "wide") == _pass(levels=3, wide_levels=3)
    assert route([], "auto") == route([], "narrow") == route([], "wide") == _pass()
    # the limit itself stays in the launch, one more leaves it and the levels after it start a second launch
    assert route([9, 4096, 9, 1], "auto") == _pass(levels=4, narrow_launches=1, exit_done=1)
    assert route([9, 4097, 9, 1], "auto") == _pass(levels=4, wide_levels=1, narrow_launches=2, exit_wide=1, exit_done=1)
    assert route([9, 4097, 9, 1], "narrow") == _pass(levels=4, narrow_launches=1, exit_done=1)
    # a wide first level has no launch before it; a wide last level none after it (the host reads the empty level itself)
    assert route([4097, 9, 1], "auto") == _pass(levels=3, wide_levels=1, narrow_launches=1, exit_done=1)
    assert route([9, 4097], "auto") == _pass(levels=2, wide_levels=1, narrow_launches=1, exit_wide=1)
    assert route([4097, 5000], "auto") == _pass(levels=2, wide_levels=2)
    # W N W N W W N N N: three runs of narrow levels, two of them followed by a wide level
    assert route(list(ALTERNATING), "auto") == _pass(levels=9, wide_levels=4, narrow_launches=3, exit_wide=2, exit_done=1)
    assert hand_over_levels(list(ALTERNATING)) == [1, 2, 3, 4, 6]
    # the whole block: the check pass has its own profile, wave_states counts degrees above 64, None = no check pass
    p = predict([4097, 2], [4096, 2], [3, 64, 65, 200], "auto", 2)
    assert p == dict(_pass("check_", levels=2, wide_levels=1, narrow_launches=1, exit_done=1),
                     **_pass(levels=2, narrow_launches=1, exit_done=1), branch=2, wave_states=2)
    assert predict(None, [3, 1], [1, 1, 1, 0], "wide") == dict(_pass("check_"), **_pass(levels=2, wide_levels=2), branch=1,
                                                               wave_states=0)
    assert set(p) == set(PREDICTED)


def test_level_profile_on_hand_made_graphs():
    # 0 -> 1 -> 3, 0 -> 2 -> 3, 2 -> 4: sinks 3 and 4, then 1 and 2, then 0
    dag = model.make_flat(5, 0, [[(1, 1, 0.0, 1), (2, 2, 0.0, 2)], [(1, 1, 0.0, 3)], [(1, 1, 0.0, 3), (2, 2, 0.0, 4)], [], []],
                       [INF, INF, INF, 0.0, 0.0])
    assert level_profile(dag) == level_profile(model.flat_to_fst(dag)) == [2, 2, 1]
    assert heights(dag)[1].tolist() == [2, 1, 1, 0, 0]
    # the height is the LONGEST way down: 0 -> 1 -> 2 and 0 -> 2
    assert level_profile(model.make_flat(3, 0, [[(1, 1, 0.0, 1), (2, 2, 0.0, 2)], [(1, 1, 0.0, 2)], []], [INF, INF, 0.0])) == [1, 1, 1]
    # two arcs of one state into one state leave together
    assert level_profile(model.make_flat(2, 0, [[(1, 1, 0.0, 1), (2, 2, 0.0, 1)], []], [INF, 0.0])) == [1, 1]
    # a cycle holds itself and what leads to it: 0 -> 1 <-> 2, 1 -> 3
    cyc = model.make_flat(4, 0, [[(1, 1, 0.0, 1)], [(1, 1, 0.0, 2), (2, 2, 0.0, 3)], [(1, 1, 0.0, 1)], []], [INF, INF, INF, 0.0])
    assert level_profile(cyc) == [1] and heights(cyc)[1].tolist() == [-1, -1, -1, 0]
    assert level_profile(model.make_flat(2, 0, [[(1, 1, 0.0, 1)], [(1, 1, 0.0, 0)]], [INF, 0.0])) == []


def _on_profile(name, kind, check=None):
    an = analysis(name, kind)
    flat = case(name, kind)
    assert an["profile"] == refine_profile(name, kind), (name, kind)
    assert an["profile_check"] == (list(PROFILES[name]) if check is None else check), (name, kind)
    assert model.known(flat["props"]) & (model.ACYCLIC | model.I_DETERMINISTIC | model.WEIGHTED) == 0 and flat["n_states"] <= 25000
    assert bool(an["exp"]["props"] & model.UNWEIGHTED) == (kind == "u"), "the branch"
    assert max(an["degrees"]) <= LANE_MAX_DEG
    assert an["exp"]["n_states"] < len(an["T"]["rows"]) // 4, "classes merge"
    return an


@pytest.mark.parametrize("kind", ("u", "w"))
def test_level_size_inputs_sit_on_their_limit(kind):
    for name in ("one_4096", "one_4097", "sinks_4096", "sinks_4097"):
        an = _on_profile(name, kind)
        assert sorted(an["profile"])[-2] < NARROW_MAX and max(an["profile"]) == int(name[-4:])
    a, b = want("one_4096", kind, "auto"), want("one_4097", kind, "auto")
    assert (a["narrow_launches"], a["wide_levels"], a["exit_wide"], a["exit_done"]) == (1, 0, 0, 1)
    assert (b["narrow_launches"], b["wide_levels"], b["exit_wide"], b["exit_done"]) == (2, 1, 1, 1)
    assert a["levels"] == b["levels"] == 5 + (kind == "w")
    # sinks: the first host step of the cycle check goes wide with no launch before it; of the refinement only unweighted
    # (the weighted T has its superfinal state alone at the bottom)
    a, b = want("sinks_4096", kind, "auto"), want("sinks_4097", kind, "auto")
    assert (a["check_wide_levels"], a["check_narrow_launches"], a["check_exit_wide"]) == (0, 1, 0)
    assert (b["check_wide_levels"], b["check_narrow_launches"], b["check_exit_wide"]) == (1, 1, 0)
    assert analysis("sinks_4097", kind)["profile_check"][0] == 4097
    assert (b["wide_levels"], b["narrow_launches"], b["exit_wide"]) == ((1, 1, 0) if kind == "u" else (1, 2, 1))
    assert analysis("sinks_4097", kind)["profile"][:2] == ([4097, 300] if kind == "u" else [1, 4097])


@pytest.mark.parametrize("kind", ("u", "w"))
def test_alternating_input_sits_on_its_limits_and_shows_the_survivor_rule(kind):
    """test 3 and test 4: in the first wide level after a narrow run and the first narrow level after a wide one the class
    that holds the level's highest id has two members or more (it keeps its HIGHEST id, so a stale C_CURMAX shows), and one
    other class has two or more (it keeps its lowest).  The one exception cannot be built: the sinks of the weighted T, the
    first wide level above the superfinal state, are ONE class in any pushed machine (final weight one after the push, a
    single arc into the superfinal state); the first half still holds for it."""
    an = _on_profile("alternating", kind)
    st = want("alternating", kind, "auto")
    shift = int(kind == "w")
    assert (st["levels"], st["wide_levels"], st["narrow_launches"], st["exit_wide"], st["exit_done"]) == \
        (9 + shift, 4, 3 + shift, 2 + shift, 1)
    wide = [size > NARROW_MAX for size in an["profile"]][shift:]
    assert wide == [True, False, True, False, True, True, False, False, False]
    assert an["profile"][shift + 3] == NARROW_MAX  # a level ON the limit directly after a wide one
    levels = hand_over_levels(an["profile"])
    assert levels == ([1] if shift else []) + [h + shift for h in (1, 2, 3, 4, 6)]
    for h in levels:
        groups = classes_of_level(an, h)
        top = max(s for g in groups.values() for s in g)
        holder = next(g for g in groups.values() if top in g)
        assert len(holder) >= 2 and min(holder) != top, (kind, h)
        if not (kind == "w" and h == 1):
            assert sum(len(g) >= 2 for g in groups.values() if top not in g) >= 1, (kind, h)
        else:
            assert len(groups) == 1
    small = _on_profile("small_alternating", kind)
    assert [a > 40 for a in small["profile"][shift:]] == [a > NARROW_MAX for a in ALTERNATING[:6]] + [False, False]


@pytest.mark.parametrize("kind", ("u", "w"))
def test_check_pass_inputs_sit_on_their_limit(kind):
    an = _on_profile("check_differs", kind, check=[301, 4097] + list(TAPER))
    flat = case("check_differs", kind)
    assert len(an["T"]["rows"]) == flat["n_states"] - 2 + (kind == "w")  # connect removes the two
    a = want("check_differs", kind, "auto")
    assert (a["check_wide_levels"], a["check_narrow_launches"], a["check_exit_wide"], a["check_exit_done"]) == (1, 2, 1, 1)
    assert (a["wide_levels"], a["narrow_launches"], a["exit_wide"], a["exit_done"]) == (0, 1, 0, 1)
    skipped = analysis("check_skipped", kind)
    assert skipped["profile_check"] is None and skipped["profile"] == an["profile"]
    assert model.known(case("check_skipped", kind)["props"]) & model.ACYCLIC
    b = want("check_skipped", kind, "auto")
    assert all(b["check_" + k] == 0 for k in PASS) and {k: b[k] for k in PASS} == {k: a[k] for k in PASS}


def _hub_states(name):
    """{type name: [ids]} of the hub level (connect keeps every state, so T has the input's ids; both kinds share them)"""
    names = hub_level(4100 if name == "degrees_wide" else 0)[1]
    return dict(zip(names, case(name, "u")["members"][2]))


@pytest.mark.parametrize("name", ("degrees_narrow", "degrees_wide"))
def test_degree_inputs_sit_on_their_limit(name):
    """test 6: the hub level as the restatement sees it, in both branches: degrees, which pairs merge and which do not, more
    than 16 wave states next to lane states, in a narrow level and in a wide one.  The rows of a pair and its twin are equal
    up to the position named and differ there, in both branches; they differ NOWHERE ELSE in the unweighted T and, for a
    twin with another target, in the weighted T.  The weighted T is sorted on the encode order, the scan position of a
    tuple's first occurrence over the whole input: a twin with another LABEL holds one tuple the pair does not share, first
    seen in a later scan, so it sorts behind the shared ones and the rows differ from that position on.  The pairs that
    differ only in the final weight and the prefix pair are pinned down for the unweighted T (in the weighted one the final
    weight is an arc, and one more arc may move the distance the weights are pushed by)."""
    hubs = _hub_states(name)
    assert case(name, "w")["members"] == case(name, "u")["members"]
    per_kind = {}
    for kind in ("u", "w"):
        an = analysis(name, kind)
        flat = case(name, kind)
        T, cls, deg = an["T"], an["part"].cls, an["degrees"]
        shift = int(kind == "w")
        assert len(T["rows"]) == flat["n_states"] + shift and flat["n_states"] <= 25000
        assert np.array_equal(np.diff(flat["offsets"].astype(np.int64)) + np.isfinite(flat["finals"]) * shift, deg[:flat["n_states"]])
        h = 2 + shift  # the hub level
        level = np.nonzero(an["height"] == h)[0]
        assert set(level.tolist()) == {s for v in hubs.values() for s in v}
        wave = [s for s in level if deg[s] > LANE_MAX_DEG]
        assert len(wave) > NARROW_WAVES and len(level) - len(wave) >= 20, "lane states next to more than 16 wave states"
        assert (len(level) > NARROW_MAX) == (name == "degrees_wide") and max(s for i, s in enumerate(an["profile"]) if i != h) <= NARROW_MAX
        # 63, 64 and 65 arcs: a final state counts one more in the weighted T
        for d in (63, 64, 65):
            assert {deg[s] for s in hubs[f"merge_{d}"]} == {d} and {deg[s] for s in hubs[f"merge_{d}_final"]} == {d + shift}
        same = lambda a, b: cls[a] == cls[b]  # noqa: E731
        for d in (63, 64, 65):
            for nm in (f"merge_{d}", f"merge_{d}_final"):
                assert same(*hubs[nm]), (kind, nm)
            assert not same(hubs[f"merge_{d}"][0], hubs[f"merge_{d}_final"][0])
        sig = lambda s: [(x[0], cls[x[3]]) for x in T["rows"][s]]  # noqa: E731
        for d, pos, what in HUB_DIFF:
            a, b = hubs[f"diff_{d}_{pos}_{what}_a"], hubs[f"diff_{d}_{pos}_{what}_b"]
            assert same(*a) and not same(a[0], b[0]) and deg[a[0]] == deg[b[0]] == d, (kind, d, pos, what)
            # ... the sorted rows are equal up to that position and differ there
            ra, rb = T["rows"][a[0]], T["rows"][b[0]]
            diff = [j for j, (x, y) in enumerate(zip(sig(a[0]), sig(b[0]))) if x != y]
            assert diff[0] == pos, (kind, d, pos, what, diff[:3])
            if kind == "u" or what == "target":  # ... and nowhere else
                assert diff == [pos], (kind, d, pos, what, diff[:3])
                assert (ra[pos][0] == rb[pos][0]) == (what == "target") and (cls[ra[pos][3]] == cls[rb[pos][3]]) == (what == "label")
        for d in (64, 65):
            a, b = hubs[f"final_only_{d}_a"], hubs[f"final_only_{d}_b"]
            assert same(*a) and same(*b) and not same(a[0], b[0])
            if kind == "u":
                assert sig(a[0]) == sig(b[0]) and T["finals"][a[0]] is None and T["finals"][b[0]] is not None
        a, b = hubs["prefix_64"], hubs["prefix_65"]
        assert same(*a) and same(*b) and not same(a[0], b[0]) and (deg[a[0]], deg[b[0]]) == (64, 65)
        if kind == "u":
            assert sig(a[0]) == sig(b[0])[:64]
        per_kind[kind] = want(name, kind, "auto")["wave_states"]
    # final states with exactly 64 label arcs are lane states of the unweighted T and wave states of the weighted one
    moved = len(hubs["merge_64_final"]) + len(hubs["final_only_64_b"])
    assert per_kind["w"] == per_kind["u"] + moved and per_kind["u"] > NARROW_WAVES


def test_cyclic_inputs_stop_where_they_are_built_to():
    for name, (flat, profile) in cyclic_cases().items():
        assert level_profile(flat) == profile, name
        assert sum(profile) < flat["n_states"] and model.is_cyclic(flat), name
        assert model.known(flat["props"]) & model.ACYCLIC == 0
        with pytest.raises(model.Unsupported, match="cyclic"):
            minimize_ref(flat)
    c = {k: route(v[1], "auto") for k, v in cyclic_cases().items()}
    assert c["ring"] == _pass()
    assert c["after_wide"] == _pass(levels=1, wide_levels=1)
    assert c["inside_narrow"] == _pass(levels=3, narrow_launches=1, exit_done=1)
    assert c["removed_by_connect"]["exit_done"] == 1
    # the cycle of the last one lies among states connect removes: the connected machine is acyclic
    flat = cyclic_cases()["removed_by_connect"][0]
    fst = model.flat_to_fst(flat)
    model.connect(fst)
    assert len(fst["rows"]) == flat["n_states"] - 2 and not model.is_cyclic(model.fst_to_flat(fst))


def cyclic_cases():
    """name -> (flat, the levels the cycle check peels); every word leaves ACYCLIC unknown"""
    out = {}
    # (a) a cycle through every state
    out["ring"] = (model.make_flat(6, 0, [[(1, 1, 0.0, (s + 1) % 6)] for s in range(6)], [INF] * 5 + [0.0], ACCEPTOR), [])
    # (b) 4097 sinks under a ring of 70 states with 60 arcs each into them: the one level that leaves is wide
    rows = [[(1, 1, 0.0, (s + 1) % 70)] + [(2 + j, 2 + j, 0.0, 70 + (60 * s + j) % 4097) for j in range(60)] for s in range(70)]
    out["after_wide"] = (model.make_flat(70 + 4097, 0, rows + [[]] * 4097, [INF] * 70 + [0.0] * 4097, ACCEPTOR), [4097])
    # (c) 0 -> 1 <-> 2 above a chain 3 -> 4 -> 5 (from 1): three levels leave inside one narrow launch
    rows = [[(1, 1, 0.0, 1)], [(1, 1, 0.0, 2), (2, 2, 0.0, 3)], [(1, 1, 0.0, 1)], [(1, 1, 0.0, 4)], [(1, 1, 0.0, 5)], []]
    out["inside_narrow"] = (model.make_flat(6, 0, rows, [INF] * 5 + [0.0], 0), [1, 1, 1])
    # (d) a good machine and two states nothing reaches that form a cycle
    good = case("small_alternating", "u")
    rows = [[tuple(a) for a in good["arcs"][good["offsets"][s]:good["offsets"][s + 1]]] for s in range(good["n_states"])]
    n = good["n_states"]
    rows += [[(1, 1, 0.0, n + 1)], [(1, 1, 0.0, n)]]
    out["removed_by_connect"] = (model.make_flat(n + 2, good["start"], rows, list(good["finals"]) + [0.0, INF], ACCEPTOR),
                                 list(SMALL_ALTERNATING))
    return out


# ================================================================ GPU
def _diff(st, exp):
    return ", ".join(f"{k} {st[k]} != {exp[k]}" for k in exp if st[k] != exp[k])


def _check(ctx, monkeypatch, name, kind, paths=PATHS):
    """minimize under every path: the result against the restatement, the counters against the prediction, the source
    handle unchanged; returns {path: counters}"""
    flat, an = case(name, kind), analysis(name, kind)
    dev = to_device(flat, ctx)
    before = dev.to_flat()
    out = {}
    for path in paths:
        monkeypatch.setenv("WFST_MINIMIZE_PATH", path)
        got = dev.minimize().to_flat()
        st = ctx.minimize_stats()
        assert_flat_identical(got, an["exp"], f"{name} {kind} {path}")
        exp = want(name, kind, path)
        print(f"{name} {kind} {path}: {st}")
        assert {k: st[k] for k in PREDICTED} == exp, f"{name} {kind} {path}: " + _diff(st, exp)
        out[path] = st
    assert_flat_identical(dev.to_flat(), before, f"{name} {kind}: source handle")
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("u", "w"))
def test_one_level_of_4096_then_4097(gpu_ctx, monkeypatch, kind):
    a = _check(gpu_ctx, monkeypatch, "one_4096", kind)["auto"]
    b = _check(gpu_ctx, monkeypatch, "one_4097", kind)["auto"]
    assert (a["narrow_launches"], a["wide_levels"], a["exit_wide"]) == (1, 0, 0)
    assert (b["narrow_launches"], b["wide_levels"], b["exit_wide"]) == (2, 1, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("u", "w"))
def test_sinks_level_of_4097(gpu_ctx, monkeypatch, kind):
    a = _check(gpu_ctx, monkeypatch, "sinks_4096", kind)["auto"]
    b = _check(gpu_ctx, monkeypatch, "sinks_4097", kind)["auto"]
    assert a["check_wide_levels"] == 0 and b["check_wide_levels"] == 1 and b["check_exit_wide"] == 0
    if kind == "u":
        assert (b["wide_levels"], b["exit_wide"], b["narrow_launches"]) == (1, 0, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("u", "w"))
def test_alternating_profile_and_survivors_across_the_hand_over(gpu_ctx, monkeypatch, kind):
    st = _check(gpu_ctx, monkeypatch, "alternating", kind)["auto"]
    assert st["wide_levels"] == 4 and st["exit_wide"] >= 2 and st["exit_done"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("u", "w"))
def test_check_pass_sees_a_different_profile(gpu_ctx, monkeypatch, kind):
    a = _check(gpu_ctx, monkeypatch, "check_differs", kind)["auto"]
    assert (a["check_wide_levels"], a["wide_levels"]) == (1, 0)
    b = _check(gpu_ctx, monkeypatch, "check_skipped", kind)["auto"]
    assert all(b["check_" + k] == 0 for k in PASS) and b["levels"] == a["levels"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("degrees_narrow", "degrees_wide"))
def test_degrees_63_64_65_lane_and_wave(gpu_ctx, monkeypatch, name):
    u = _check(gpu_ctx, monkeypatch, name, "u")
    w = _check(gpu_ctx, monkeypatch, name, "w")
    for path in PATHS:
        assert w[path]["wave_states"] == u[path]["wave_states"] + 4 > NARROW_WAVES
    assert (u["auto"]["wide_levels"] == 1) == (name == "degrees_wide")


def _class_pairs(name, kind):
    """sum over the levels of T of C * (C - 1) / 2, C = the restatement's classes of the level"""
    an = analysis(name, kind)
    per_level = collections.defaultdict(set)
    for s, h in enumerate(an["height"]):
        per_level[int(h)].add(an["part"].cls[s])
    return sum(len(c) * (len(c) - 1) // 2 for c in per_level.values())


def _classes(name, kind):
    return len(set(analysis(name, kind)["part"].cls))


@pytest.mark.gpu
@pytest.mark.parametrize("bits", (0, 4))
def test_hash_bits(gpu_ctx, monkeypatch, bits):
    """with few hash bits different signatures share slot and tag, and only the full compare (and the probe that goes on
    after an unequal one) keeps them apart.  With 0 bits every state of a level walks one chain, and a chain of C
    representatives costs at least 0 + 1 + ... + (C - 1) unequal compares whatever the insertion order."""
    monkeypatch.setenv("WFST_MINIMIZE_HASH_BITS", str(bits))
    for name in ("degrees_narrow", "degrees_wide", "small_alternating"):
        for kind in ("u", "w"):
            for path, st in _check(gpu_ctx, monkeypatch, name, kind).items():
                if bits == 0:
                    assert st["unequal_compares"] >= _class_pairs(name, kind), (name, kind, path, st["unequal_compares"])
                else:  # 16 values: the representatives of one value but the first meet an unequal one
                    assert st["unequal_compares"] >= _classes(name, kind) - 16, (name, kind, path, st["unequal_compares"])


@pytest.mark.gpu
def test_hash_bits_knob_values(gpu_ctx, monkeypatch):
    import rustfst_amd
    dev = to_device(case("small_alternating", "u"), gpu_ctx)
    for value in ("65", "-1", "x", "4x", " 4", "100"):
        monkeypatch.setenv("WFST_MINIMIZE_HASH_BITS", value)
        with pytest.raises(rustfst_amd.WfstError, match="WFST_MINIMIZE_HASH_BITS"):
            dev.minimize()
        assert gpu_ctx.minimize_stats() == dict.fromkeys(COUNTERS, 0)
    for value in ("", "64", "0", "07"):
        monkeypatch.setenv("WFST_MINIMIZE_HASH_BITS", value)
        assert_flat_identical(dev.minimize().to_flat(), analysis("small_alternating", "u")["exp"], f"bits '{value}'")


@pytest.mark.gpu
def test_default_run_records_unequal_compares(gpu_ctx, monkeypatch):
    """test 8 without the hash restated in Python (module docstring): the default run of test 7's inputs gives the same
    result, and its unequal_compares is printed, not asserted"""
    monkeypatch.delenv("WFST_MINIMIZE_HASH_BITS", raising=False)
    for name in ("degrees_narrow", "degrees_wide", "small_alternating"):
        for kind in ("u", "w"):
            for path, st in _check(gpu_ctx, monkeypatch, name, kind).items():
                print(f"{name} {kind} {path}: unequal_compares {st['unequal_compares']} with all 64 bits")


@pytest.mark.gpu
def test_cyclic_inputs_are_ko_with_their_counters(gpu_ctx, monkeypatch):
    import rustfst_amd
    good = to_device(case("small_alternating", "u"), gpu_ctx)
    for name, (flat, profile) in cyclic_cases().items():
        dev = to_device(flat, gpu_ctx)
        for path in PATHS:
            monkeypatch.setenv("WFST_MINIMIZE_PATH", path)
            with pytest.raises(rustfst_amd.WfstError, match=re.escape(MSG_CYCLIC)):
                dev.minimize()
            st = gpu_ctx.minimize_stats()
            exp = predict(profile, None, (), path, 0)
            assert {k: st[k] for k in PREDICTED} == exp and st["unequal_compares"] == 0, f"{name} {path}: " + _diff(st, exp)
            if path == "auto":
                assert st["check_exit_done"] == {"ring": 0, "after_wide": 0, "inside_narrow": 1, "removed_by_connect": 1}[name]
                assert name != "ring" or (st["check_narrow_launches"], st["check_levels"]) == (0, 0)
            # the same context minimizes a good input, and the counters are that call's
            assert_flat_identical(good.minimize().to_flat(), analysis("small_alternating", "u")["exp"], f"after {name}")
            st = gpu_ctx.minimize_stats()
            assert {k: st[k] for k in PREDICTED} == want("small_alternating", "u", path), f"after {name} {path}"


@pytest.mark.gpu
def test_counters_reset_and_empty_inputs(gpu_ctx, monkeypatch):
    monkeypatch.setenv("WFST_MINIMIZE_PATH", "auto")
    dev = to_device(case("one_4097", "w"), gpu_ctx)
    dev.minimize()
    first = gpu_ctx.minimize_stats()
    assert {k: first[k] for k in PREDICTED} == want("one_4097", "w", "auto")
    for props in (0, ACCEPTOR, ACCEPTOR | model.I_DETERMINISTIC | model.WEIGHTED):
        empty = model.make_flat(0, None, [], [], props)
        assert to_device(empty, gpu_ctx).minimize().to_flat()["n_states"] == 0
        assert gpu_ctx.minimize_stats() == dict.fromkeys(COUNTERS, 0), hex(props)
        dev.minimize()
        assert gpu_ctx.minimize_stats() == first
    # the branches that end early: nothing left after connect (4), weighted without a start state (3)
    dead = model.make_flat(3, 0, [[(1, 1, 1.0, 1)], [(1, 1, 2.0, 2)], []], [INF, INF, INF], ACCEPTOR)
    to_device(dead, gpu_ctx).minimize()
    st = gpu_ctx.minimize_stats()
    assert st["branch"] == 4 and st["check_levels"] == 3 and st["levels"] == 0
    flat, message = mc.no_start_cases()[0]
    assert message is None
    to_device(flat, gpu_ctx).minimize()
    assert gpu_ctx.minimize_stats()["branch"] == 3
