"""CPU model of the bounded head of a single-shortest-path query (sssp_mailbox.h, mbox_narrow<LOG, true>): which part of a
graph the first launch follows before the best final state is settled, and whether it may end the search there.  numpy only;
used by tools/bounded_reach.py and by the tests that place final states at the limits of the head.

The model is level-synchronous like the kernel: a level expands the states the previous one listed, B (the best total seen)
and the threshold min(tau0, B) are taken once per level.  It lists a state once per level, with the least candidate of that
level; the kernel lists every winning candidate, so its lists can be a few entries longer than the model's."""
from __future__ import annotations

import numpy as np

NW_GROW = 384  # a level wider than this hands over to the WIDE levels (sssp_mailbox.h)
NW_CAP = 1024
NW_MAX_LEVELS = 4096


def first_band(t: dict, tau0_mult: float = 1.0) -> float:
    """tau0 of a mailbox solve of t as relax_setup fixes it: 1.5 mean arc weights, scaled by 10 / (arcs per state) outside
    8.5 .. 10 arcs per state, and by the ratio of the states' cheapest arcs to what uniform weights would give where that
    ratio is below 0.7 or above 2 (band_from_mean_weight, band_from_cheapest_arcs)."""
    w = t["arcs"]["weight"].astype(np.float64)
    off = t["offsets"].astype(np.int64)
    n = int(t["n_states"])
    fin = np.isfinite(w)
    mean = float(np.float32(w[fin].mean()))
    deg = w.shape[0] / n
    delta = np.float32(1.5) * np.float32(mean)
    if deg > 10.0 or deg < 8.5:
        delta = np.float32(float(delta) * 10.0 / deg)
    has = off[1:] > off[:-1]
    mins = np.minimum.reduceat(np.where(fin, w, np.inf), off[:-1][has])
    mins = mins[np.isfinite(mins)]
    if mins.size:
        ratio = float(np.float32(mins.mean())) * (deg + 1.0) / (2.0 * mean)
        if ratio < 0.7:
            delta = np.float32(float(delta) * max(ratio, 0.1))
        elif ratio > 2.0:
            delta = delta * np.float32(1.4)
    return float(np.float32(delta) * np.float32(tau0_mult))


def head_reach(t: dict, start: int | None = None, tau0: float | None = None, tau0_mult: float = 1.0) -> dict:
    """Runs the head's loop.  Returns tau0, B (inf: no total seen), `engaged` (the head ends the search), `why` (the exit
    when it does not), the list size of every level, the states expanded, the arcs relaxed, the least candidate not followed,
    and `dist` (float32, inf where the head left no key)."""
    n = int(t["n_states"])
    off = t["offsets"].astype(np.int64)
    nxt = t["arcs"]["nextstate"].astype(np.int64)
    w = t["arcs"]["weight"].astype(np.float32)
    finals = t["finals"].astype(np.float32)
    s0 = int(t["start"] if start is None else start)
    tau = np.float32(first_band(t, tau0_mult) if tau0 is None else tau0)
    d = np.full(n, np.inf, dtype=np.float32)
    d[s0] = 0.0
    B = np.float32(finals[s0]) if np.isfinite(finals[s0]) else np.float32(np.inf)
    cur = np.array([s0], dtype=np.int64)
    sizes, expanded, relaxed = [], 0, 0
    least_left = np.float32(np.inf)
    far_seen = False
    why = None
    prev_n = prev2_n = 0
    for level in range(NW_MAX_LEVELS + 1):
        n_lv = int(cur.shape[0])
        if n_lv == 0:
            break
        sizes.append(n_lv)
        thr = min(tau, B)
        in_band = bool(B <= tau)
        if n_lv > NW_GROW:
            why = f"level {level} holds {n_lv} states, more than NW_GROW = {NW_GROW}"
            break
        if level >= 2 and prev_n < prev2_n and far_seen and not in_band:
            why = f"the near set shrank at level {level} while states waited beyond the first band and B = {float(B):g} > tau0"
            break
        if level >= NW_MAX_LEVELS:
            why = "NW_MAX_LEVELS"
            break
        cnt = off[cur + 1] - off[cur]
        idx = np.repeat(off[cur], cnt) + (np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt))
        c = (np.repeat(d[cur], cnt) + w[idx]).astype(np.float32)
        tg = nxt[idx]
        expanded += n_lv
        relaxed += int(idx.shape[0])
        ok = np.isfinite(c)
        far = ok & (c > thr)
        if far.any():
            far_seen = True
            least_left = min(least_left, np.float32(c[far].min()))
        near = ok & ~far
        best = np.full(n, np.inf, dtype=np.float32)
        np.minimum.at(best, tg[near], c[near])
        won = np.flatnonzero(best < d)
        d[won] = best[won]
        tot = (d[won] + finals[won]).astype(np.float32)
        if tot.size and np.isfinite(tot).any():
            B = min(B, np.float32(tot[np.isfinite(tot)].min()))
        prev2_n, prev_n = prev_n, n_lv
        cur = won
    engaged = why is None and bool(np.isfinite(B)) and bool(B <= tau)
    if why is None and not engaged:
        why = "no final state within the first band" if not np.isfinite(B) else f"B = {float(B):g} > tau0 = {float(tau):g}"
    return dict(tau0=float(tau), B=float(B), engaged=engaged, why=why, levels=len(sizes), sizes=sizes, expanded=expanded,
                relaxed=relaxed, least_not_followed=float(least_left), dist=d)
