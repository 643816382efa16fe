"""N un-profiled shortest_path(T) solves on the C3 graph (for rocprofv3 --kernel-trace timelines and PMC passes).
usage: sp_repeat.py [states] [reps] [warm-up solves] [--full] [--walk-finals] [--far-final]
  --full         every solve relaxes all arcs (WFST_SSSP_BOUNDED=0): what a roofline or PMC figure of the relaxation needs
  --walk-finals  the end states of the benchmark's random walks (64 of its batch, 4096 of its batch_sweep extra) are final with
                 weight 0.5 as in bench.py's T: the bounded head then ends the query in launch 0 (without them the best total
                 of this T, 8.20, lies beyond the first band, 7.50, and every solve is the full one)
  --far-final    the only final state is the state of greatest distance: the bounded head runs and cannot stop"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
opts = {a for a in sys.argv[1:] if a.startswith("--")}
sys.argv = [a for a in sys.argv if not a.startswith("--")]
if "--full" in opts:
    os.environ["WFST_SSSP_BOUNDED"] = "0"
import rustfst_amd
from rustfst_amd import synth

states = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
warm = int(sys.argv[3]) if len(sys.argv) > 3 else 0  # solves before anything is timed (the GPU's clocks ramp over the first few hundred)
t = synth.make_transducer(states, 10, 256, 0.0, seed=3)
if "--walk-finals" in opts:
    synth.make_acceptors(t, 64, 200, seed0=1000)
    synth.make_acceptors(t, 4096, 200, seed0=50_000)
ctx = rustfst_amd.Context(0)
if "--far-final" in opts:
    import numpy as np
    d0 = rustfst_amd.DeviceFst.from_arrays(t["n_states"], t["start"], t["offsets"], t["arcs"], t["finals"], t["props"], ctx)
    far = int(np.argmax(np.where(np.isfinite(d0.shortest_distance()), d0.shortest_distance(), -1.0)))
    t["finals"][:] = np.inf
    t["finals"][far] = 0.5
    del d0
d = rustfst_amd.DeviceFst.from_arrays(t["n_states"], t["start"], t["offsets"], t["arcs"], t["finals"], t["props"], ctx)
import hashlib
dist, hops = d.shortest_distance(want_hops=True)  # (a digest of the labels: library variants run in separate processes)
print("labels sha1", hashlib.sha1(dist.tobytes() + hops.tobytes()).hexdigest()[:16], "kernel", ctx.stats()["relax_kernel"])
for _ in range(warm):
    d.shortest_path()
best = 1e9
for _ in range(reps):
    t0 = time.perf_counter(); d.shortest_path(); best = min(best, time.perf_counter() - t0)
print(f"best of {reps}: {best*1e3:.3f} ms, sweeps {ctx.stats()['sweeps']} (after {warm} warm-up solves)")
# (profiling mode 2 always runs the full solve: the chain below is the relaxation of every arc, bounded head or not)
# the same solves with the relaxation chain bracketed by HIP events (profiling mode 2): under `rocprofv3 --kernel-trace` this
# process then holds BOTH clocks for the same launches — the events' chain time and the trace's per-kernel durations
import statistics
print("rearm_stats", ctx.rearm_stats(), "bounded_stats", ctx.bounded_stats())
ctx.set_profiling(2)
chain = []
for _ in range(max(5, reps // 2)):
    d.shortest_path()
    st = ctx.stats()
    if st["relax_launches"]:
        chain.append(st["relax_ms"] * 1e3)
ctx.set_profiling(0)
if chain:
    print(f"relaxation chain by HIP events (this process): median {statistics.median(chain):.1f} us, min {min(chain):.1f} us "
          f"over {len(chain)} solves, {int(ctx.stats()['relax_launches'])} launches, kernel {int(ctx.stats()['relax_kernel'])}")
