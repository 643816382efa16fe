"""top_sort and state_sort (dfs_visit.rs, top_sort.rs, state_sort.rs), restated."""
import copy

from .props import ACYCLIC, ALL, CYCLIC, INITIAL_ACYCLIC, NOT_STRING, NOT_TOP_SORTED, STRING, TOP_SORTED


STATESORT_MASK = ALL & ~(TOP_SORTED | NOT_TOP_SORTED | STRING | NOT_STRING)  # properties.rs:319-348
WHITE, GREY, BLACK = 0, 1, 2


def dfs_top_order(fst):
    """dfs_visit(fst, TopOrderVisitor, AnyTrFilter, access_only = false) (dfs_visit.rs:97-187, top_sort.rs:12-61):
    (acyclic, order); order is empty when the search found a back arc or the FST has no start state"""
    rows = fst["rows"]
    finish, acyclic = [], True
    start = fst["start"]
    if start is not None:
        n = len(rows)
        color = [WHITE] * n
        stack = []
        dfs, root = True, start
        while dfs and root < n:
            color[root] = GREY
            stack.append([root, 0])
            dfs = True  # init_state
            while stack:
                s, pos = stack[-1]
                if not dfs or pos >= len(rows[s]):
                    color[s] = BLACK
                    stack.pop()
                    finish.append(s)  # finish_state, with or without a parent
                    if stack:
                        stack[-1][1] += 1
                    continue
                t = rows[s][pos][3]
                if color[t] == WHITE:
                    dfs = True  # tree_tr
                    color[t] = GREY
                    stack.append([t, 0])
                    dfs = True  # init_state
                elif color[t] == GREY:
                    acyclic = False  # back_tr
                    dfs = False
                    stack[-1][1] += 1
                else:
                    dfs = True  # forward_or_cross_tr
                    stack[-1][1] += 1
            root = 0 if root == start else root + 1
            while root < n and color[root] != WHITE:
                root += 1
    order = []
    if acyclic:  # finish_visit
        order = [0] * len(finish)
        for s in range(len(finish)):
            order[finish[len(finish) - s - 1]] = s
    return acyclic, order


def state_sort_ref(fst, order):
    """state_sort.rs:16-78, in place; the mutations' own property updates are overwritten by the last statement"""
    n = len(fst["rows"])
    if len(order) != n:
        raise ValueError(f"StateSort : Bad order vector size : {len(order)}. Expected {n}")
    if fst["start"] is None:
        return fst
    props = fst["props"] & STATESORT_MASK
    done = [False] * n
    fst["start"] = order[fst["start"]]
    for s1 in range(n):
        if done[s1]:
            continue
        final1, final2 = fst["finals"][s1], None
        trsa, trsb = [list(t) for t in fst["rows"][s1]], []
        while not done[s1]:
            s2 = order[s1]
            if not done[s2]:
                final2 = fst["finals"][s2]
                trsb = [list(t) for t in fst["rows"][s2]]
            fst["finals"][s2] = final1
            fst["rows"][s2] = [[il, ol, w, order[ns]] for il, ol, w, ns in trsa]
            done[s1] = True
            trsa, trsb = trsb, trsa
            final1 = final2
            s1 = s2
    fst["props"] = props  # set_properties_with_mask(props, all_properties())
    return fst


def top_sort_ref(fst):
    """top_sort.rs:76-94 on a copy; raises ValueError with state_sort's message"""
    fst = copy.deepcopy(fst)
    acyclic, order = dfs_top_order(fst)
    if acyclic:
        state_sort_ref(fst, order)
        p = ACYCLIC | INITIAL_ACYCLIC | TOP_SORTED
    else:
        p = CYCLIC | NOT_TOP_SORTED
    fst["props"] = (fst["props"] & ~p) | (p & p)  # set_properties_with_mask(p, p) (vector_fst/mutable_fst.rs:411-414)
    return fst
