"""shortest_distance(reverse), reweight and push_weights on T (1M states / 10M arcs by default): the first call and a
repeated call on one handle, wall clock around each call (synchronous API).  python tools/push_timing.py [states]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import rustfst_amd
from rustfst_amd import synth

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
t = synth.make_transducer(N)
ctx = rustfst_amd.default_context()
R = rustfst_amd.ReweightType


def upload():
    return rustfst_amd.DeviceFst.from_arrays(t["n_states"], t["start"], t["offsets"], t["arcs"], t["finals"], t["props"], ctx)


def timed(fn, reps=5):
    t0 = time.perf_counter(); out = fn(); ctx.synchronize(); first = (time.perf_counter() - t0) * 1e3
    rep = []
    for _ in range(reps):
        t0 = time.perf_counter(); out = fn(); ctx.synchronize(); rep.append((time.perf_counter() - t0) * 1e3)
    return first, float(np.median(rep)), out


d = upload()
first, rep, dist = timed(lambda: d.shortest_distance(reverse=True))
print(f"reverse distance      first {first:8.2f} ms   repeated {rep:8.2f} ms   (T {N} states / {len(t['arcs'])} arcs)")
d2 = upload()
first, rep, _ = timed(lambda: d2.reweight(dist, R.REWEIGHT_TO_INITIAL))
print(f"reweight (host pot.)  first {first:8.2f} ms   repeated {rep:8.2f} ms   (start branch + structural pass included)")
d2.set_start(0)
d3 = upload()
first, rep, _ = timed(lambda: d3.push_weights(R.REWEIGHT_TO_INITIAL))
print(f"push_weights ToInitial first {first:8.2f} ms   repeated {rep:8.2f} ms")
d4 = upload()
first, rep, _ = timed(lambda: d4.push_weights(R.REWEIGHT_TO_FINAL, rustfst_amd.PushWeightsConfig(remove_total_weight=True)))
print(f"push_weights ToFinal+remove first {first:8.2f} ms   repeated {rep:8.2f} ms")
