"""The CPU model of the bounded head (rustfst_amd/reach.py) against the oracle, without a GPU: where the model says the head
ends the search, every state at or below B carries its final distance, nothing not followed is at or below B, and B is the
oracle's best total — the three facts the stop rests on."""
import numpy as np
import pytest

from rustfst_amd import reach, synth
from helpers import to_oracle

N = 70_000


@pytest.fixture(scope="module")
def t():
    return synth.make_transducer(N, 8, 64, 0.0, seed=9)


def test_first_band_of_the_fixture(t):
    assert abs(reach.first_band(t) - 9.362) < 1e-3
    assert abs(reach.first_band(t, 2.0) - 2 * reach.first_band(t)) < 1e-5


@pytest.mark.parametrize("start", [0, 11, 4097, N - 1])
def test_engaged_head_settles_everything_at_or_below_b(t, oracle, start):
    f = dict(t, start=start)
    r = reach.head_reach(f)
    can = to_oracle(oracle, f).shortest_path_canonical()
    dist = np.asarray(can.distance, dtype=np.float32)
    best = np.float32((dist + t["finals"]).min())
    if not r["engaged"]:
        assert best > np.float32(r["tau0"]) or max(r["sizes"]) > reach.NW_GROW, (start, r["why"], best)
        return
    b = np.float32(r["B"])
    assert b == best
    settled = dist <= b
    np.testing.assert_array_equal(r["dist"][settled].view(np.uint32), dist[settled].view(np.uint32))
    assert (r["dist"][~settled] >= dist[~settled]).all()  # (what the head left above B is a real path's length, or nothing)
    assert r["least_not_followed"] > b


def test_the_two_sources_of_the_gpu_tests(t):
    r = reach.head_reach(t)
    assert r["engaged"] and r["levels"] == 8 and max(r["sizes"]) == 13 and r["expanded"] == 67 and abs(r["B"] - 6.1387) < 1e-3
    r = reach.head_reach(t, start=N // 3)
    assert not r["engaged"] and abs(r["B"] - 12.85) < 1e-2 and r["B"] > r["tau0"]
