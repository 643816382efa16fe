#!/usr/bin/env python
"""Medians per launch of the shortest-path query's chain, from a rocprofv3 --kernel-trace rocpd database.
usage: python tools/chain_medians.py <trace_results.db> [label]
A solve is counted when its relaxation is the predicted three launches, in one of two shapes:
  set-up, head (sssp_mbox_kernel, NARROW), the resident launch, the NARROW tail launch (sssp_mbox_kernel again), sssp_tail_kernel
  head, resident, NARROW tail launch, sssp_tail_kernel          (re-armed scratch: no set-up launch; WFST_SSSP_REARM)
or when the bounded head ended it (WFST_SSSP_BOUNDED), with or without a set-up launch:
  head, sssp_tail_kernel                      (the NARROW-tail column then reads "-")
  head, a spare resident launch that leaves at entry, sssp_tail_kernel
any of them with sssp_mbox_rearm_kernel behind the tail or without.  The label gets the count of each shape.  Kernels of other streams (the string batch of the bench
step) are ignored.  Prints one markdown row: median (min) in us per launch (set-up over the solves that have one), first start ->
tail end, the re-arm launch, and the gap from its end to the next launch of the chain (the next solve's first): the two are on one
stream, so a re-arm launch that does not hide in the host's gap shows as a gap near zero — the share below 1 us is printed."""
import sqlite3
import statistics
import sys

SETUP, MBOX, RES, TAIL, REARM = ("sssp_mbox_setup_kernel", "sssp_mbox_kernel", "sssp_mbox_resident_kernel", "sssp_tail_kernel",
                                 "sssp_mbox_rearm_kernel")
BODY = (MBOX, RES, MBOX, TAIL)
BOUNDED_BODIES = ((MBOX, TAIL), (MBOX, RES, TAIL))  # head [spare launch] tail
NAMES = (SETUP, MBOX, RES, TAIL, REARM)


def solves(path):
    """[(set-up row or None, the four rows of BODY, re-arm row or None, start of the chain's next launch or None)]"""
    c = sqlite3.connect(path)
    rows = c.execute("select name, start, end from kernels order by start").fetchall()
    rows = [(next((k for k in NAMES if k + "<" in n or k + "(" in n), None), s, e) for n, s, e in rows]
    rows = [r for r in rows if r[0]]
    out, cur = [], []
    for i, r in enumerate(rows):
        if r[0] == REARM:
            continue  # (attached to the solve in front of it below)
        if r[0] == SETUP:
            cur = []
        cur.append(r)
        if r[0] == TAIL:
            names = tuple(k for k, _, _ in cur)
            body = names[1:] if names and names[0] == SETUP else names
            if body == BODY or body in BOUNDED_BODIES:
                rearm = rows[i + 1] if i + 1 < len(rows) and rows[i + 1][0] == REARM else None
                nxt = rows[i + 2][1] if rearm and i + 2 < len(rows) else None
                b = cur[len(cur) - len(body):]
                # four columns: head, resident (or the spare launch), NARROW tail launch, tail — None where the shape has none
                four = b if body == BODY else [b[0], b[1] if len(b) == 3 else None, None, b[-1]]
                out.append((cur[0] if names[0] == SETUP else None, four, rearm, nxt))
            cur = []
    return out


def cell(v):
    return f"{statistics.median(v):.2f} ({min(v):.2f})" if v else "-"


def main():
    sv = solves(sys.argv[1])
    label = sys.argv[2] if len(sys.argv) > 2 else sys.argv[1]
    if len(sv) < 3:
        print(f"| {label} | only {len(sv)} solves of the predicted shape |")
        return
    sv = sv[len(sv) // 8:]  # (the first solves run while the clocks ramp)
    us = lambda r: (r[2] - r[1]) / 1e3
    setup = [us(s) for s, _, _, _ in sv if s]
    cols = [[us(b[i]) for _, b, _, _ in sv if b[i]] for i in range(4)]
    n_bounded = sum(b[2] is None for _, b, _, _ in sv)
    label = f"{label} ({n_bounded} bounded, {len(sv) - n_bounded} full)"
    whole = [(b[-1][2] - (s or b[0])[1]) / 1e3 for s, b, _, _ in sv]
    rearm = [us(r) for _, _, r, _ in sv if r]
    gap = [(nx - r[2]) / 1e3 for _, _, r, nx in sv if r and nx is not None]
    tight = f", {100.0 * sum(g < 1.0 for g in gap) / len(gap):.0f} % below 1 us" if gap else ""
    print(f"| {label} | {len(sv)} | {len(setup)} with set-up: {cell(setup)} | " + " | ".join(cell(c) for c in cols) +
          f" | {cell(whole)} | {len(rearm)} re-armed: {cell(rearm)} | {cell(gap)}{tight} |")


if __name__ == "__main__":
    main()
