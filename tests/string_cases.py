"""The string kernel of compose.hip: its limits restated once, the walk that predicts its run counters, and the input
families that more than one test module uses."""
import functools

from helpers import analyse, assert_flat_identical, finals_of, fst, to_device

# ---- the string kernel's own limits (rustfst_amd/csrc/compose.hip), restated once
STR_MAXS = 2048         # :1018
STR_LEVEL = 64          # :1115 idx >= 64u
STR_SLICES = (512, 1024, 2048)  # :1480-1481 the least slice >= 2 * max_states + 64, packed batches of >= 16
STR_PACKED_MIN, STR_SCALAR_MAX_N = 16, 8  # :1477 n >= 16; :1496 n <= 8
RUN_BLOCK = 64  # fc <= 64u


@functools.lru_cache(maxsize=None)
def ladder_t(w):
    """label 1 leads from the start state to w states that loop on it: every level of 1^L has w states.  Label 2 loops too,
    and adds ONE state from g0: a string that ends in 2 has one state more in all, and w + 1 in its last level."""
    g = lambda j: 1 + j
    rows = [[(1, 100 + j, (j % 4) / 4.0, g(j)) for j in range(w)]]
    for j in range(w):
        rows.append([(1, 100 + j, 0.25, g(j)), (2, 200 + j, 0.0, g(j))] + ([(2, 300, 0.25, g(w))] if j == 0 else []))
    rows.append([(1, 400, 0.25, g(w))])
    return fst(rows, finals_of(w + 2, {g(j): ((j * 3) % 5) / 4.0 for j in range(w + 1)}))


def string_slice(n_eligible, max_states, unpacked=False):
    """states per problem of the string kernel's LDS slice: packed batches of >= 16 take the least slice >= 2 * states + 64"""
    if unpacked or n_eligible < STR_PACKED_MIN:
        return STR_MAXS
    return next(m for m in STR_SLICES if 2 * max_states + 64 <= m or m == STR_MAXS)


def walk(labels, t, maxs):
    """(composed states, widest level, run levels, runs) of string o T as the kernel's vector path does it with slice maxs"""
    off, arcs = t["offsets"], t["arcs"]
    il, ns = arcs["ilabel"], arcs["nextstate"]
    L = len(labels)
    frontier, hi, widest, run_levels, runs, in_run = [int(t["start"])], 1, 1, 0, 0, False
    for pos in range(L):
        nxt, matches = [], 0
        for q in frontier:
            for e in range(int(off[q]), int(off[q + 1])):
                if int(il[e]) == int(labels[pos]):
                    matches += 1
                    if int(ns[e]) not in nxt:
                        nxt.append(int(ns[e]))
        q = frontier[0]
        taken = (len(frontier) == 1 and int(off[q + 1]) - int(off[q]) <= RUN_BLOCK and pos + 1 < L and hi + 1 < maxs
                 and matches == 1)
        if taken:
            run_levels += 1
            runs += not in_run
        in_run = taken
        hi += len(nxt)
        widest = max(widest, len(nxt))
        frontier = nxt
        if not frontier:
            break
    return hi, widest, run_levels, runs


def predict(strs, t, scalar, unpacked):
    """(string_run_stats(), problems the string kernel answers) of one call with the run on"""
    eligible = [s for s in strs if s["n_states"] <= STR_MAXS]
    out, answered = dict(run_levels=0, runs=0), 0
    if not eligible:
        return out, answered
    vector = scalar == "0" or (scalar is None and len(eligible) > 8)
    maxs = string_slice(len(eligible), max(s["n_states"] for s in eligible), unpacked)
    for s in eligible:
        n, widest, rl, r = walk(s["arcs"]["ilabel"], t, maxs)
        if widest <= STR_LEVEL and n <= maxs:  # answered by the string kernel: its counters are tallied
            answered += 1
            if vector:  # (scalar rows: the run is not entered)
                out["run_levels"] += rl
                out["runs"] += r
    return out, answered


def four_ways(ctx, oracle, monkeypatch, strs, t, sizes, scalar=None, unpacked=False, min_run_levels=1):
    import rustfst_amd
    dt, handles = to_device(t, ctx), rustfst_amd.DeviceFst.upload_many(strs, ctx)
    ans = [analyse(oracle, s, t) for s in strs]
    for name, val in (("WFST_STRING_SCALAR", scalar), ("WFST_STRING_UNPACKED", "1" if unpacked else None)):
        monkeypatch.delenv(name, raising=False) if val is None else monkeypatch.setenv(name, val)
    seen = 0
    for n in sizes:
        want, answered = predict(strs[:n], t, scalar, unpacked)
        seen += want["run_levels"]
        for mode in ("run", "no_run", "general"):
            monkeypatch.setenv("WFST_STRING_RUN", "0" if mode == "no_run" else "1")
            monkeypatch.setenv("WFST_STRING_KERNEL", "0" if mode == "general" else "1")
            outs, n_arcs = rustfst_amd.compose_shortest_path_batch(handles[:n], dt)
            what = "%s, batch of %d" % (mode, n)
            for k in range(n):
                assert_flat_identical(outs[k].to_flat(), ans[k]["path"], "%s, string %d" % (what, k))
            assert n_arcs == sum(len(a["full"]["arcs"]) for a in ans[:n]), what
            assert int(ctx.stats()["compose_states"]) == sum(a["full"]["n_states"] for a in ans[:n]), what
            got, st = ctx.string_run_stats(), ctx.compose_path_stats()
            assert got == (want if mode == "run" else dict(run_levels=0, runs=0)), (what, got, want)
            assert st["string_answered"] == (answered if mode != "general" else 0), (what, st)
    for name in ("WFST_STRING_RUN", "WFST_STRING_KERNEL", "WFST_STRING_SCALAR", "WFST_STRING_UNPACKED"):
        monkeypatch.delenv(name, raising=False)
    assert seen >= min_run_levels, "the case has no run level at all"


N_MIX = 9


@functools.lru_cache(maxsize=None)
def mix_t():
    """9 states, all final.  Labels 1, 2, 3: one arc each (a level of them is one match).  4: two arcs to ONE state, the
    second the cheaper one.  5: two arcs to two states.  6: no arc.  7: three arcs to three states.  8: one arc to state 0
    (whatever the frontier was, it collapses to one state)."""
    rows = []
    for s in range(N_MIX):
        g = lambda k: (s + k) % N_MIX
        rows.append([(1, 10 + s, ((s * 5) % 9) / 512.0, g(1)), (2, 20 + s, ((s * 7) % 11) / 512.0, g(4)),
                     (3, 30 + s, 0.0, (2 * s + 1) % N_MIX), (4, 40 + s, 3 / 512.0, g(2)), (4, 50 + s, 1 / 512.0, g(2)),
                     (5, 60 + s, 2 / 512.0, g(1)), (5, 70 + s, 1 / 512.0, g(5)), (7, 80 + s, 0.0, g(1)), (7, 90 + s, 5 / 512.0, g(2)),
                     (7, 100 + s, 1 / 512.0, g(3)), (8, 110 + s, (s % 3) / 512.0, 0)])
    return fst(rows, finals_of(N_MIX, {s: s / 512.0 for s in range(N_MIX)}))
