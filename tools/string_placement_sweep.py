"""Where the waves of a fused string batch should sit: B linear acceptors (200 labels) against the bench's T, B in
{16, 64, 128, 256, 512, 1024, 4096} x WFST_STRING_WPB in {1, 2, 4, 8, unset}.  Per cell: the host clock of the fused call
(packed records: no handles to build), best of 5 after one warm-up call, and Context.string_placement() of the last call.
The process solves nothing, so "unset" is the rule without a resident grid (rustfst_amd/csrc/string_placement.h).
A library from before the rule (WFST_LIB_PATH) ignores the knob: its five columns are five runs of one placement.

    python tools/string_placement_sweep.py [B ...]          one markdown table; profiles/string_placement_ab.md has one"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rustfst_amd
from rustfst_amd import synth

KNOB = "WFST_STRING_WPB"
sizes = [int(a) for a in sys.argv[1:]] or [16, 64, 128, 256, 512, 1024, 4096]
t = synth.make_transducer(1_000_000, 10, 256, 0.0, seed=3)
accs = synth.make_acceptors(t, max(sizes), 200, seed0=50_000)
ctx = rustfst_amd.Context(0)
dt = rustfst_amd.DeviceFst.from_arrays(t["n_states"], t["start"], t["offsets"], t["arcs"], t["finals"], t["props"], ctx)
arms = ["1", "2", "4", "8", None]
print("| B | " + " | ".join("WPB=%s" % a if a else "unset" for a in arms) + " | placement when unset |")
print("|---:|" + "---:|" * len(arms) + "---|")
for b in sizes:
    db = rustfst_amd.HandleArray(rustfst_amd.DeviceFst.upload_many(accs[:b], ctx))
    cells, place = [], None
    for arm in arms:
        if arm is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = arm
        tab, _ = rustfst_amd.compose_shortest_path_batch_packed(db, dt, 208)
        best = 1e9
        for _ in range(5):
            ctx.synchronize()
            t0 = time.perf_counter()
            tab, _ = rustfst_amd.compose_shortest_path_batch_packed(db, dt, 208, out=tab)
            best = min(best, time.perf_counter() - t0)
        place = ctx.string_placement()
        cells.append("%.1f (w %d)" % (best * 1e6, place["waves_per_workgroup"]))
    os.environ.pop(KNOB, None)
    print("| %d | " % b + " | ".join(cells) + " | %d waves x %d workgroups, slice %d, packed_for_resident %d |" % (
        place["waves_per_workgroup"], place["workgroups"], place["slice_states"], place["packed_for_resident"]), flush=True)
print("(us per fused call, host clock, best of 5; w = waves per workgroup the launch took)")
