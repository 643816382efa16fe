"""invert in place on the device (wfst_fst_invert): the K22 vector, the involution, and — the checks tests/test_handle_state.py
makes for project — that after the edit the handle answers every call exactly as a fresh upload of the host-inverted FST
does: arrays and property word, compose on the newly sorted tape, shortest_path, reverse, isomorphic, the string shape."""
import numpy as np
import pytest

import rustfst_amd
from rustfst_amd import ComposeConfig, WfstError, synth

from oracle.model import ALL, flat_to_fst, fst_to_flat

import helpers
from helpers import assert_flat_identical, one_sided_eps_transducer, random_fst_flat, to_device
import isomorphic_cases as K
import isomorphic_ref as R

pytestmark = pytest.mark.gpu


def host_inverted(flat):
    """the flat FST with its two label columns exchanged and the word invert_properties gives"""
    arcs = flat["arcs"].copy()
    arcs["ilabel"], arcs["olabel"] = flat["arcs"]["olabel"].copy(), flat["arcs"]["ilabel"].copy()
    return dict(flat, arcs=arcs, props=R.invert_properties(flat["props"] & ALL))


def inputs_for_invert():
    rng = np.random.default_rng(2230)
    out = [("ilabel-sorted", random_fst_flat(rng, 40, 4, 6, p_eps_i=0.1, p_eps_o=0.2, sort="ilabel")),
           ("olabel-sorted", random_fst_flat(rng, 300, 3, 5, p_eps_i=0.2, p_eps_o=0.0, sort="olabel", acyclic=True)),
           ("unsorted", random_fst_flat(rng, 17, 5, 4, sort="none")),
           ("input-epsilons-only", one_sided_eps_transducer(rng, 30, 4, 5, "ilabel", sort="ilabel")),
           ("output-epsilons-only", one_sided_eps_transducer(rng, 30, 4, 5, "olabel", sort="olabel")),
           ("no-arcs", helpers.fst([[], []], [np.inf, 0.5])),
           ("T", synth.make_transducer(2000, 6, 32, 0.05, seed=9))]
    return out


@pytest.mark.parametrize("name,flat", inputs_for_invert(), ids=[n for n, _ in inputs_for_invert()])
def test_inverted_handle_equals_fresh_upload(gpu_ctx, name, flat):
    h = to_device(flat, gpu_ctx)
    h.shortest_path()  # (fills what a query caches on the handle before the edit)
    assert h.invert() is h
    exp = host_inverted(flat)
    fresh = to_device(exp, gpu_ctx)
    assert_flat_identical(h.to_flat(), exp, name)
    assert h.properties == fresh.properties == exp["props"]
    assert_flat_identical(h.shortest_path().to_flat(), fresh.shortest_path().to_flat(), name + " shortest_path")
    assert_flat_identical(h.reverse().to_flat(), fresh.reverse().to_flat(), name + " reverse")
    assert h.isomorphic(fresh) is True and fresh.isomorphic(h) is True
    try:  # the original against the inverted handle: whatever the restatement says of the two
        got = 1 if to_device(flat, gpu_ctx).isomorphic(h) else 0
    except WfstError as e:
        got = str(e).split(": ", 1)[1]
    assert got == R.verdict(flat_to_fst(flat), flat_to_fst(exp)), name
    # compose on the tape the word now calls sorted: the same FST or the same refusal as the fresh upload
    rng = np.random.default_rng(7)
    partner = to_device(random_fst_flat(rng, 12, 3, 6, p_eps_i=0.1, p_eps_o=0.1, sort="ilabel"), gpu_ctx)
    partner_o = to_device(random_fst_flat(rng, 12, 3, 6, p_eps_i=0.1, p_eps_o=0.1, sort="olabel"), gpu_ctx)
    for connect in (True, False):
        for as_fst2 in (True, False):
            def run(x):
                try:
                    cfg = ComposeConfig(connect=connect)
                    return (partner_o.compose(x, cfg) if as_fst2 else x.compose(partner, cfg)).to_flat()
                except WfstError as e:
                    return str(e)
            got, want = run(h), run(fresh)
            if isinstance(want, str):
                assert got == want, name
            else:
                assert_flat_identical(got, want, "%s compose connect=%s" % (name, connect))
    # twice: arrays and word bit for bit
    h.invert()
    back = h.to_flat()
    assert_flat_identical(back, dict(flat, props=flat["props"] & ALL), name + " twice")


def test_k22_vector(gpu_ctx):
    inv = K.k22()["invert"]
    h = helpers.dev(K.from_spec(inv["input"]), gpu_ctx).invert()
    exp = fst_to_flat(K.from_spec(inv["expected"]))
    got = h.to_flat()
    assert np.array_equal(got["offsets"], exp["offsets"]) and np.array_equal(got["arcs"], exp["arcs"])
    assert np.array_equal(got["finals"], exp["finals"]) and got["start"] == exp["start"]
    v = rustfst_amd.VectorFst()
    s = [v.add_state() for _ in range(3)]
    v.set_start(s[0])
    v.set_final(s[2], 1.0)
    for src, il, ol, w, dst in ((0, 1, 2, 1.0, 1), (0, 3, 4, 2.0, 1), (1, 5, 6, 1.5, 1), (1, 3, 5, 1.0, 2)):
        v.add_tr(s[src], rustfst_amd.Tr(il, ol, w, s[dst]))
    assert rustfst_amd.invert(v) is v
    assert np.array_equal(v.to_device(gpu_ctx).to_flat()["arcs"], exp["arcs"])


def test_sorted_tape_follows_the_labels(gpu_ctx):
    """tr_sort on the output tape, invert: the handle is known to be sorted on the input tape, and composes as fst2"""
    rng = np.random.default_rng(2231)
    flat = random_fst_flat(rng, 25, 4, 5, sort="none")
    h = to_device(flat, gpu_ctx)
    h.tr_sort(ilabel_cmp=False)
    word = h.properties
    assert word & R.O_LABEL_SORTED
    h.invert()
    assert h.properties == R.invert_properties(word) and h.properties & R.I_LABEL_SORTED
    left = to_device(random_fst_flat(rng, 10, 3, 5, sort="none"), gpu_ctx)  # sorted on neither tape: fst2 must carry the match
    fresh = to_device(h.to_flat(), gpu_ctx)
    assert_flat_identical(left.compose(h).to_flat(), left.compose(fresh).to_flat(), "compose")


def test_string_shape_is_asked_again(gpu_ctx):
    """a string (ilabel == olabel on every arc) stays one; the fused batch takes it down the string route as a fresh upload"""
    t = synth.make_transducer(500, 6, 16, 0.0, seed=5)
    accs = synth.make_acceptors(t, 3, 12, seed0=50)
    dt = to_device(t, gpu_ctx)
    edited = [to_device(a, gpu_ctx).invert() for a in accs]
    fresh = rustfst_amd.DeviceFst.upload_many(accs, gpu_ctx)
    for a, e in zip(accs, edited):
        assert_flat_identical(e.to_flat(), host_inverted(a), "string")
    got, _ = rustfst_amd.compose_shortest_path_batch(edited, dt)
    n_edited = gpu_ctx.stats()["string_problems"]  # (of the last call)
    want, _ = rustfst_amd.compose_shortest_path_batch(fresh, dt)
    assert n_edited == gpu_ctx.stats()["string_problems"] == len(accs)  # the string kernel took both batches alike
    for g, w in zip(got, want):
        assert_flat_identical(g.to_flat(), w.to_flat(), "string batch")


def test_errors(gpu_ctx):
    other = rustfst_amd.Context(0)
    f = to_device(helpers.fst([[(1, 2, 0.5, 1)], []], [np.inf, 0.0]), other)
    from rustfst_amd import _lib
    assert helpers.ko_message(_lib.lib().wfst_fst_invert(gpu_ctx._h, f._h)) == "invert: the FST belongs to another context"
    assert helpers.ko_message(_lib.lib().wfst_fst_invert(gpu_ctx._h, None)) == "null pointer"
    assert np.array_equal(f.to_flat()["arcs"]["ilabel"], [1])  # untouched
    assert f.invert().to_flat()["arcs"]["ilabel"][0] == 2
