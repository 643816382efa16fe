"""The input handle of top_sort / state_sort is left as it is: what it answered before the call — a shortest_path query, with
the derived data that query caches on the handle — it answers bit for bit afterwards, and the new handle answers for the
renamed machine (in the manner of test_handle_state.py: fill a cache, call, observe)."""
import numpy as np
import pytest

from oracle.model import ACYCLIC, INITIAL_ACYCLIC, fst_to_flat, state_sort_ref, top_sort_ref
from helpers import assert_flat_identical, dev
from inputs import chain


def _weights(flat):
    from helpers import enumerate_paths
    return sorted(w for w, _, _ in enumerate_paths(flat))


@pytest.mark.gpu
@pytest.mark.parametrize("n", (40, 3000))
def test_input_still_answers_shortest_path(gpu_ctx, n):
    rng = np.random.default_rng(1950 + n)
    m = chain(n, rng, fan=3)
    order = rng.permutation(n).tolist()
    m = state_sort_ref(m, order)  # ids that say nothing about the topological order
    m["props"] = ACYCLIC | INITIAL_ACYCLIC
    fresh = dev(m, gpu_ctx).shortest_path().to_flat()
    h = dev(m, gpu_ctx)
    first = h.shortest_path().to_flat()  # (the second query of a handle builds its cached transpose)
    before = h.to_flat()
    sorted_h = h.top_sort()
    for _ in range(2):
        assert_flat_identical(h.shortest_path().to_flat(), fresh, "shortest_path after top_sort")
    renamed = h.state_sort(order)
    assert_flat_identical(h.shortest_path().to_flat(), fresh, "shortest_path after state_sort")
    assert_flat_identical(first, fresh, "shortest_path")
    assert_flat_identical(h.to_flat(), before, "the input handle", check_props=True)
    # the new handles are machines of their own: the same best path weight, found on the renamed states
    exp = top_sort_ref(m)
    assert_flat_identical(sorted_h.to_flat(), fst_to_flat(exp), "top_sort", check_props=True)
    assert _weights(sorted_h.shortest_path().to_flat()) == _weights(fresh)
    assert _weights(renamed.shortest_path().to_flat()) == _weights(fresh)
