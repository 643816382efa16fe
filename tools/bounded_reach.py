"""What the bounded head of a shortest_path query follows on a given T and source, simulated on the CPU (rustfst_amd/reach.py:
numpy only, no native library): tau0, B, the levels and their list sizes, states expanded, arcs relaxed, the least candidate
not followed, and whether the head ends the search (engaged) or why not.
usage: bounded_reach.py [states] [fanout] [sigma] [seed] [--source S]... [--walks K] [--sweep-walks K2] [--tau0-mult M]
  --walks K         the end states of K random walks become final with weight 0.5, as bench.py's T has them for its batch
                    (default 64; 0: none)
  --sweep-walks K2  ... and those of the K2 walks of its batch_sweep extra, drawn with or without --full (default 4096;
                    0: the T of bench.py --no-extras)
Defaults are bench.py's T: 1 000 000 states, fan-out 10, 256 labels, seed 3, source 0."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rustfst_amd import reach, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("states", nargs="?", type=int, default=1_000_000)
    ap.add_argument("fanout", nargs="?", type=int, default=10)
    ap.add_argument("sigma", nargs="?", type=int, default=256)
    ap.add_argument("seed", nargs="?", type=int, default=3)
    ap.add_argument("--source", type=int, action="append")
    ap.add_argument("--walks", type=int, default=64)
    ap.add_argument("--sweep-walks", type=int, default=4096)
    ap.add_argument("--tau0-mult", type=float, default=1.0)
    a = ap.parse_args()
    t = synth.make_transducer(a.states, a.fanout, a.sigma, 0.0, seed=a.seed)
    if a.walks:
        synth.make_acceptors(t, a.walks, 200, seed0=1000)
    if a.sweep_walks:
        synth.make_acceptors(t, a.sweep_walks, 200, seed0=50_000)
    import numpy as np
    print(f"{int(np.isfinite(t['finals']).sum())} final states")
    print("| source | tau0 | B | engaged | levels | list sizes per level | states expanded | arcs relaxed | least candidate not followed |")
    print("|---|---:|---:|---|---:|---|---:|---:|---:|")
    for s in a.source or [int(t["start"])]:
        r = reach.head_reach(t, start=s, tau0_mult=a.tau0_mult)
        print(f"| {s} | {r['tau0']:.4f} | {r['B']:.7g} | {'yes' if r['engaged'] else 'no: ' + r['why']} | {r['levels']} | "
              f"{', '.join(map(str, r['sizes']))} | {r['expanded']} | {r['relaxed']} | {r['least_not_followed']:.7g} |")


if __name__ == "__main__":
    main()
