#!/usr/bin/env python
"""Medians per launch of the shortest-path query's chain, from a rocprofv3 --kernel-trace rocpd database.
usage: python tools/chain_medians.py <trace_results.db> [label]
A solve is counted when its relaxation is the predicted three launches: set-up, head (sssp_mbox_kernel, NARROW), the resident
launch, the NARROW tail launch (sssp_mbox_kernel again), sssp_tail_kernel.  Kernels of other streams (the string batch of the
bench step) are ignored.  Prints one markdown row: median (min) in us per launch, and first start -> tail end."""
import sqlite3
import statistics
import sys

ORDER = ("sssp_mbox_setup_kernel", "sssp_mbox_kernel", "sssp_mbox_resident_kernel", "sssp_mbox_kernel", "sssp_tail_kernel")


def solves(path):
    c = sqlite3.connect(path)
    rows = c.execute("select name, start, end from kernels order by start").fetchall()
    rows = [(next((k for k in set(ORDER) if k + "<" in n or k + "(" in n), None), s, e) for n, s, e in rows]
    rows = [r for r in rows if r[0]]
    out, cur = [], []
    for r in rows:
        if r[0] == ORDER[0]:
            cur = []
        cur.append(r)
        if r[0] == ORDER[-1]:
            if tuple(k for k, _, _ in cur) == ORDER:
                out.append(cur)
            cur = []
    return out


def main():
    sv = solves(sys.argv[1])
    label = sys.argv[2] if len(sys.argv) > 2 else sys.argv[1]
    if len(sv) < 3:
        print(f"| {label} | only {len(sv)} solves of the predicted shape |")
        return
    sv = sv[len(sv) // 8:]  # (the first solves run while the clocks ramp)
    cols = [[(e - s) / 1e3 for s, e in ((x[i][1], x[i][2]) for x in sv)] for i in range(len(ORDER))]
    cols.append([(x[-1][2] - x[0][1]) / 1e3 for x in sv])
    print(f"| {label} | {len(sv)} | " + " | ".join(f"{statistics.median(c):.2f} ({min(c):.2f})" for c in cols) + " |")


if __name__ == "__main__":
    main()
