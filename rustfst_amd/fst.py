"""Host-side mirror of the reference's Python surface for the compose -> shortest_path path.

Names, argument meaning and error behaviour follow rustfst-python
(rustfst-python/rustfst/fst/vector_fst.py, rustfst/tr.py, rustfst/algorithms/{compose,shortest_path}.py)
so that the parity tests read like the reference's own tests.  Everything that computes goes
through the C-ABI of libwfst_amd.so (include/wfst.h) onto the GPU; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import threading
from enum import Enum
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib
from ._lib import TR_DTYPE, WfstError, check

KSHORTESTDELTA = 1e-6  # rustfst/src/lib.rs:271
KDELTA = 1.0 / 1024.0  # rustfst/src/lib.rs:266


class Tr:
    """An arc (rustfst-python/rustfst/tr.py:17-136): ilabel, olabel, weight, next_state."""

    __slots__ = ("ilabel", "olabel", "weight", "next_state")

    def __init__(self, ilabel: int = 0, olabel: int = 0, weight: Optional[float] = None, nextstate: int = 0):
        self.ilabel = int(ilabel)
        self.olabel = int(olabel)
        self.weight = 0.0 if weight is None else float(weight)  # weight_one
        self.next_state = int(nextstate)

    def __eq__(self, other):
        return (self.ilabel, self.olabel, self.next_state) == (other.ilabel, other.olabel, other.next_state) and \
            abs(np.float32(self.weight) - np.float32(other.weight)) <= 1.0 / 1024.0

    def __repr__(self):
        return f"<Tr ilabel={self.ilabel}, olabel={self.olabel}, weight={self.weight}, next_state={self.next_state}>"


# ------------------------------------------------------------------ context
def _counters(family: str, ctx: "Context") -> dict:
    """One family of route counters of ctx (_lib.COUNTERS) as a dict of ints, in the order of the getter's parameters."""
    symbol, names = _lib.COUNTERS[family]
    vals = [C.c_uint64() for _ in names]
    check(getattr(_lib.lib(), symbol)(ctx._h, *[C.byref(v) for v in vals]), symbol)
    return {k: int(v.value) for k, v in zip(names, vals)}


class Context:
    """One engine context per (host thread, GPU): a HIP stream + device memory pools."""

    def __init__(self, device: int = 0, stream: Optional[int] = None, cu_mask: Optional[Sequence[int]] = None):
        """stream: an existing HIP stream handle to run on; cu_mask: list of 32-bit words, bit i of word i//32 =
        compute unit i — the context then owns a stream restricted to those CUs."""
        L = _lib.lib()
        h = C.c_void_p()
        if cu_mask is not None:
            words = np.asarray(list(cu_mask), dtype=np.uint32)
            check(L.wfst_ctx_create_with_cu_mask(device, words.ctypes.data, len(words), C.byref(h)),
                  "wfst_ctx_create_with_cu_mask")
        elif stream is None:
            check(L.wfst_ctx_create(device, C.byref(h)), "wfst_ctx_create")
        else:
            check(L.wfst_ctx_create_on_stream(device, C.c_void_p(stream), C.byref(h)), "wfst_ctx_create_on_stream")
        self._h = h
        self.device = device

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                _lib.lib().wfst_ctx_destroy(h)
            except Exception:
                pass
            self._h = None

    def synchronize(self):
        check(_lib.lib().wfst_ctx_synchronize(self._h), "wfst_ctx_synchronize")

    def set_resident_share(self, share: int):
        """0 (default): a resident relaxation launch may fill the device (fastest alone); 1: at most half of it, so that it runs
        beside a large fused batch instead of behind it (wfst_ctx_set_resident_share)."""
        check(_lib.lib().wfst_ctx_set_resident_share(self._h, int(share)), "wfst_ctx_set_resident_share")

    def rearm_stats(self) -> dict:
        """Re-armed relaxation scratch of this context (wfst_ctx_get_rearm_stats): solves that parked their cleaned scratch
        (armed), that started from parked scratch without a set-up launch (adopted), parked scratch given back unused (dropped)."""
        if not hasattr(_lib.lib(), "wfst_ctx_get_rearm_stats"):  # (WFST_LIB_PATH: a build from before the counters)
            return dict(armed=0, adopted=0, dropped=0)
        return _counters("rearm", self)

    def bounded_stats(self) -> dict:
        """The bounded head of the single-shortest-path relaxation on this context (wfst_ctx_get_bounded_stats): queries whose
        first launch ended the search once the best final state was settled (stops), queries of the large-FST route that ran
        the full solve (full_solves) and why the last of those did (last_reason)."""
        if not hasattr(_lib.lib(), "wfst_ctx_get_bounded_stats"):  # (WFST_LIB_PATH: a build from before the counters)
            return dict(stops=0, full_solves=0, last_reason="")
        stops, full, why = C.c_uint64(), C.c_uint64(), C.c_char_p()
        check(_lib.lib().wfst_ctx_get_bounded_stats(self._h, C.byref(stops), C.byref(full), C.byref(why)), "wfst_ctx_get_bounded_stats")
        return dict(stops=int(stops.value), full_solves=int(full.value), last_reason=(why.value or b"").decode())

    def solo_query(self) -> dict:
        """The solo query of this context (wfst_ctx_get_solo_query): launches of the one-workgroup kernel that answers a repeated
        bounded shortest-path query on the parked scratch (attempts), those that answered, those that gave the query up to the
        ordinary route (aborted), why the last of those did (last_abort: "", "BAND", "GREW", "LOG" or "OTHER") and the keys
        the last launch put back (cleaned).  All 0 / "" with a library from before the route."""
        if not hasattr(_lib.lib(), "wfst_ctx_get_solo_query"):  # (WFST_LIB_PATH: a build from before the route)
            return dict(dict.fromkeys(_lib.SOLO_QUERY, 0), last_abort="")
        vals = [C.c_uint64() for _ in _lib.SOLO_QUERY]
        check(_lib.lib().wfst_ctx_get_solo_query(self._h, *[C.byref(v) for v in vals]), "wfst_ctx_get_solo_query")
        out = {k: int(v.value) for k, v in zip(_lib.SOLO_QUERY, vals)}
        out["last_abort"] = _lib.SOLO_ABORTS[out["last_abort"]]
        return out

    def parked_key_check(self) -> int:
        """Tests: how many words of this context's parked relaxation keys are not +inf (wfst_ctx_parked_key_check): an armed
        scratch has none.  Raises when nothing is parked."""
        not_inf = C.c_uint64()
        check(_lib.lib().wfst_ctx_parked_key_check(self._h, C.byref(not_inf)), "wfst_ctx_parked_key_check")
        return int(not_inf.value)

    def small_path_stats(self) -> dict:
        """Which path answered the small shortest-path queries of this context (wfst_ctx_get_small_path_stats): the last
        launch of the nshortest = 1 wave kernel (n1_in_kernel, n1_staged, n1_handed_back) and the last n-best batch
        (nbest_in_kernel, nbest_tree_full, nbest_out_full, nbest_tree_capacity)."""
        return _counters("small_path", self)

    def compose_path_stats(self) -> dict:
        """Which route answered the problems of this context's last compose / compose_shortest_path_batch call
        (wfst_ctx_get_compose_path_stats): the string kernel (string_answered) or its hand-backs (string_handed_back), the
        wave kernel's first launch (wave_first), relaunches with a 4x arena by overflow status (relaunch_states / _arcs /
        _hash / _path), the wide driver (switched_wide), the two-step route (two_step), and the capacities of the last
        wave launch (caps_states, caps_arcs, caps_hash)."""
        return _counters("compose_path", self)

    def string_run_stats(self) -> dict:
        """The chase runs of the string kernel in this context's last compose_shortest_path_batch call
        (wfst_ctx_get_string_run_stats): levels taken inside runs (run_levels) and the number of runs (runs), summed over
        the problems the kernel answered.  Both are 0 with WFST_STRING_RUN=0 and on the scalar-row path."""
        return _counters("string_run", self)

    def string_pair_counts(self) -> dict:
        """The pair levels of the string kernel in this context's last compose_shortest_path_batch call
        (wfst_ctx_get_string_pair_counts): levels its run loop carried that are not run levels — a frontier of two states,
        or one state that matches two arcs, one or two matches in all with distinct destinations — (pair_levels) and those
        of them with two matches (pair_splits), summed over the problems the kernel answered.  Both are 0 with
        WFST_STRING_PAIR=0, with WFST_STRING_RUN=0 and on the scalar-row path."""
        vals = [C.c_uint64() for _ in _lib.STRING_PAIR_COUNTS]
        check(_lib.lib().wfst_ctx_get_string_pair_counts(self._h, *[C.byref(v) for v in vals]),
              "wfst_ctx_get_string_pair_counts")
        return {k: int(v.value) for k, v in zip(_lib.STRING_PAIR_COUNTS, vals)}

    def string_placement(self) -> dict:
        """Where the waves of this context's last string launch sat (wfst_ctx_get_string_placement): waves per workgroup
        (waves_per_workgroup), composed states a wave's LDS slice holds (slice_states), workgroups of the launch
        (workgroups), whether a resident relaxation launch on the device made the launch pack its waves
        (packed_for_resident) and whether WFST_STRING_WPB or WFST_STRING_UNPACKED decided (forced).  All 0 when the last
        compose_shortest_path_batch call launched no string kernel, and with a library from before the counters."""
        if not hasattr(_lib.lib(), "wfst_ctx_get_string_placement"):  # (WFST_LIB_PATH: a build from before the counters)
            return dict.fromkeys(_lib.STRING_PLACEMENT, 0)
        vals = [C.c_uint64() for _ in _lib.STRING_PLACEMENT]
        check(_lib.lib().wfst_ctx_get_string_placement(self._h, *[C.byref(v) for v in vals]), "wfst_ctx_get_string_placement")
        return {k: int(v.value) for k, v in zip(_lib.STRING_PLACEMENT, vals)}

    def determinize_stats(self) -> dict:
        """Which route the levels of this context's last determinize / determinize_with_distance call took
        (wfst_ctx_get_determinize_stats): levels completed (levels) and those the device-wide launches ran (wide_levels),
        launches of the one-workgroup kernel (narrow_launches) by how they ended (exit_wide_states, exit_wide_cands,
        exit_budget, exit_need, exit_done), device-wide checks that asked for room (wide_need), arrays enlarged (grow_states,
        grow_elts, grow_arcs, grow_cands, rehashes), their final sizes (cap_states, cap_elts, cap_arcs, cap_cands) and the most
        resolve rounds of a device-wide level (rounds_max).  Unspecified after a batch call."""
        return _counters("determinize", self)

    def minimize_stats(self) -> dict:
        """Which route this context's last minimize call took (wfst_ctx_get_minimize_stats).  For the cycle check on the
        untrimmed input (check_*) and for the refinement of the connected machine (no prefix): non-empty levels peeled
        (levels), those the device-wide launches ran (wide_levels), launches of the one-workgroup kernel (narrow_launches)
        by how they ended (exit_wide, exit_done).  For the call: the branch taken (branch: 0 none, 1 unweighted, 2 weighted,
        3 weighted without a start state, 4 nothing left after connect), states a wave refined (wave_states) and full
        signature compares that found a difference (unequal_compares).  Unspecified after minimize_batch and optimize."""
        return _counters("minimize", self)

    def push_stats(self) -> dict:
        """Which route this context's last shortest_distance(reverse=..) with a length, reweight or push_weights call took
        (wfst_ctx_get_push_stats): frontier searches (searches), their bfs_round_kernel launches (rounds), host reads of a
        frontier size (reads), the most rounds of one search (rounds_max), the grids of the last bfs_round_kernel,
        reweight_arcs_kernel and total_weight_kernel launch (bfs_blocks, arcs_blocks, total_blocks; 0: did not run), whether
        the structural facts were searched (structural), the start branch (start_branch: 0 not taken, 1 in place, 2 new
        start state) and remove_total_weight (removed: 0 not requested, 1 skipped, 2 applied).  Unspecified after any other
        call."""
        return _counters("push", self)

    def top_sort_stats(self) -> dict:
        """Which route this context's last top_sort call took (wfst_ctx_get_top_sort_stats): Kahn levels peeled (levels),
        launches of the one-workgroup and of the device-wide level kernels over the four level phases (narrow_launches,
        wide_launches), levels peeled inside one-workgroup launches (narrow_levels), the widest level (max_level_width), the
        deepest state of the search forest (max_tree_depth), rows of the ancestor table (lift_rows), states with in-arcs from
        at least two states (states_compared), states a whole wave took (wave_states) and the CYCLIC exit (cyclic)."""
        return _counters("top_sort", self)

    def isomorphic_stats(self) -> dict:
        """Which route this context's last isomorphic call took (wfst_ctx_get_isomorphic_counters): levels of the search that
        ran, launches of the one-workgroup and of the device-wide phase kernels (narrow_launches, wide_launches: four per
        wide level), levels inside one-workgroup launches (narrow_levels), the widest level in pairs (max_level_width),
        pairs and arc slots of the levels that ran (pairs, events), pairs a whole wave walked (wave_pairs), states of both
        operands sorted by the radix route (big_states_sorted) and non-determinism marks made (nondet_marks)."""
        vals = [C.c_uint64() for _ in _lib.ISOMORPHIC_COUNTERS]
        check(_lib.lib().wfst_ctx_get_isomorphic_counters(self._h, *[C.byref(v) for v in vals]),
              "wfst_ctx_get_isomorphic_counters")
        return {k: int(v.value) for k, v in zip(_lib.ISOMORPHIC_COUNTERS, vals)}

    def paths_counters(self) -> dict:
        """The route of this context's last count_paths / paths / paths_batch call (wfst_ctx_get_paths_counters): kernel
        launches and library calls (launches), items counted by the one-workgroup kernel and by the device-wide route
        (items_in_kernel, items_single), the deepest peel (levels), the paths counted (paths), the arcs of the longest path
        (max_path_arcs) and items whose count saturated (saturated)."""
        vals = [C.c_uint64() for _ in _lib.PATHS_COUNTERS]
        check(_lib.lib().wfst_ctx_get_paths_counters(self._h, *[C.byref(v) for v in vals]), "wfst_ctx_get_paths_counters")
        return {k: int(v.value) for k, v in zip(_lib.PATHS_COUNTERS, vals)}

    def lookahead_stats(self) -> dict:
        """Which route answered the compositions of this context's last LookAhead.compose / compose_batch call
        (wfst_ctx_get_lookahead_stats): items and those without a start state, compositions the single-wave kernel finished
        (wave_answered), gave up on for their states or for a level's width (handed_over_states, handed_over_width) or for a
        full arena (overflow_arcs, overflow_states), compositions the wide driver ran (wide_items), lone relaunches under
        WFST_LOOKAHEAD_PATH=wave (wave_regrows), growths of the wide arena (wide_grows), wide arenas raised by the handle's
        hint (wide_hinted) and hinted allocations that were refused (hint_fallbacks), and whether the limits of a call with
        one composition applied (one_limits)."""
        return _counters("lookahead", self)

    def replace_stats(self) -> dict:
        """This context's last replace call (wfst_ctx_get_replace_stats): levels of the search, states and arcs of the result,
        distinct non-empty call stacks interned (prefixes) and the deepest of them (max_depth), call arcs emitted, call arcs
        dropped for a callee without a start state, return arcs emitted, times the search's arena grew (arena_grows) and
        times the expansion ran again with a larger call-stack table (prefix_reruns), and the level kernels queued
        (level_launches: three per level, idle ones behind the last level included)."""
        return _counters("replace", self)

    def compose_sigma_stats(self) -> dict:
        """This context's last composition with a MatcherConfig (wfst_ctx_get_compose_sigma_counters): levels of the search,
        states and arcs before connect, composed states whose fst1 / fst2 state carries a sigma arc (require1_states,
        require2_states), items of a sigma side answered by its sorted matcher (exact_items) and by its sigma arcs
        (sigma_items), the arcs those emitted (sigma_arcs), items the allowed set refused (refused_items), times the
        search's arena grew (arena_grows) and the level kernels queued (level_launches)."""
        vals = [C.c_uint64() for _ in _lib.COMPOSE_SIGMA_COUNTERS]
        check(_lib.lib().wfst_ctx_get_compose_sigma_counters(self._h, *[C.byref(v) for v in vals]),
              "wfst_ctx_get_compose_sigma_counters")
        return {k: int(v.value) for k, v in zip(_lib.COMPOSE_SIGMA_COUNTERS, vals)}

    def sigma_batch_stats(self) -> dict:
        """This context's last compose_shortest_path_batch with a MatcherConfig (wfst_ctx_get_sigma_batch_counters): launches
        of the wave-per-utterance kernel, items it answered (items_in_kernel), items it handed back (a level wider than 64
        states or more composed states than its slice of LDS holds), items never sent to it (items_loop), then, summed over
        the items the kernel answered, the item counters of compose_sigma_stats (exact_items, sigma_items, sigma_arcs,
        refused_items) and the widest level among them (max_level_width)."""
        vals = [C.c_uint64() for _ in _lib.SIGMA_BATCH_COUNTERS]
        check(_lib.lib().wfst_ctx_get_sigma_batch_counters(self._h, *[C.byref(v) for v in vals]),
              "wfst_ctx_get_sigma_batch_counters")
        return {k: int(v.value) for k, v in zip(_lib.SIGMA_BATCH_COUNTERS, vals)}

    def trim_pool(self):
        """Frees every device block the context's pool holds without an owner: cached blocks and parked scratch
        (wfst_ctx_trim_pool).  Synchronises the device."""
        check(_lib.lib().wfst_ctx_trim_pool(self._h), "wfst_ctx_trim_pool")

    def set_tie_order(self, reference_order: bool):
        """shortest_path(nshortest = 1): False = the canonical tie rule (default); True = the reference's own choice among
        tied optima on ACYCLIC inputs (wfst_ctx_set_tie_order)."""
        check(_lib.lib().wfst_ctx_set_tie_order(self._h, 1 if reference_order else 0), "wfst_ctx_set_tie_order")

    @property
    def stream(self) -> int:
        s = C.c_void_p()
        check(_lib.lib().wfst_ctx_stream(self._h, C.byref(s)))
        return s.value or 0

    def set_profiling(self, on):
        """False / 0: off; True / 1: events around every relaxation launch (synchronises after each); 2: the sweeps of a
        repeated shortest_path query timed as one chain between two events (stats: relax_ms, relax_launches)."""
        check(_lib.lib().wfst_ctx_set_profiling(self._h, int(on)))

    def reset_stats(self):
        check(_lib.lib().wfst_ctx_reset_stats(self._h))

    def sweep_trace(self):
        """(ms, arcs, states) arrays, one entry per relaxation launch of the last profiled solve."""
        n = C.c_size_t()
        check(_lib.lib().wfst_ctx_get_sweep_trace(self._h, None, None, None, 0, C.byref(n)))
        ms = np.zeros(n.value, dtype=np.float64)
        arcs = np.zeros(n.value, dtype=np.uint64)
        states = np.zeros(n.value, dtype=np.uint64)
        check(_lib.lib().wfst_ctx_get_sweep_trace(self._h, ms.ctypes.data, arcs.ctypes.data, states.ctypes.data,
                                                  n.value, C.byref(n)))
        return ms, arcs, states

    def sweep_modes(self):
        """What ran each launch of the last profiled solve: 0 atomic sweep, 7 binned level, or the mailbox mode."""
        n = C.c_size_t()
        check(_lib.lib().wfst_ctx_get_sweep_modes(self._h, None, 0, C.byref(n)))
        modes = np.zeros(n.value, dtype=np.uint32)
        check(_lib.lib().wfst_ctx_get_sweep_modes(self._h, modes.ctypes.data, n.value, C.byref(n)))
        return modes

    def stats(self) -> dict:
        st = _lib.Stats()
        check(_lib.lib().wfst_ctx_get_stats(self._h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in st._fields_}


_default_ctx = threading.local()


def default_context() -> Context:
    ctx = getattr(_default_ctx, "ctx", None)
    if ctx is None:
        ctx = Context(0)
        _default_ctx.ctx = ctx
    return ctx


def set_default_context(ctx: Context):
    _default_ctx.ctx = ctx


# ------------------------------------------------------------------ device FST handle
class DeviceFst:
    """Owning wrapper of a wfst_fst handle: an FST resident in HBM as CSR."""

    def __init__(self, handle, ctx: Context, owner=None):
        self._h = handle
        self.ctx = ctx
        self._owner = owner  # a PathList that owns the handle (this object is then a view)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and getattr(self, "_owner", None) is None:
            try:
                _lib.lib().wfst_fst_destroy(h)
            except Exception:
                pass
        self._h = None

    @classmethod
    def from_arrays(cls, n_states: int, start: Optional[int], offsets, arcs, finals, props: int,
                    ctx: Optional[Context] = None) -> "DeviceFst":
        ctx = ctx or default_context()
        offsets = np.ascontiguousarray(offsets, dtype=np.uint32)
        arcs = np.ascontiguousarray(arcs, dtype=TR_DTYPE)
        finals = np.ascontiguousarray(finals, dtype=np.float32)
        if offsets.shape[0] != n_states + 1 or finals.shape[0] != n_states:
            raise ValueError("offsets must have n_states+1 entries and finals n_states")
        if n_states and arcs.shape[0] != int(offsets[-1]):
            raise ValueError("arcs must have offsets[-1] entries")
        h = C.c_void_p()
        check(_lib.lib().wfst_fst_upload(ctx._h, n_states, -1 if start is None else int(start), offsets.ctypes.data,
                                         arcs.ctypes.data, finals.ctypes.data, int(props), C.byref(h)),
              "wfst_fst_upload")
        return cls(h, ctx)

    @classmethod
    def from_device_arrays(cls, n_states: int, start: Optional[int], d_offsets: int, d_arcs: int, d_finals: int,
                           props: int, ctx: Optional[Context] = None) -> "DeviceFst":
        """Arrays already in HBM (raw device pointers, e.g. torch tensor .data_ptr())."""
        ctx = ctx or default_context()
        h = C.c_void_p()
        check(_lib.lib().wfst_fst_upload_device(ctx._h, n_states, -1 if start is None else int(start),
                                                C.c_void_p(d_offsets), C.c_void_p(d_arcs), C.c_void_p(d_finals),
                                                int(props), C.byref(h)), "wfst_fst_upload_device")
        return cls(h, ctx)

    @classmethod
    def upload_many(cls, flats: Sequence[dict], ctx: Optional[Context] = None) -> List["DeviceFst"]:
        """flats: dicts with n_states,start,offsets,arcs,finals,props. One arena, one copy."""
        ctx = ctx or default_context()
        n = len(flats)
        if n == 0:
            return []
        n_states = np.array([f["n_states"] for f in flats], dtype=np.uint32)
        starts = np.array([-1 if f["start"] is None else f["start"] for f in flats], dtype=np.int64)
        props = np.array([f["props"] for f in flats], dtype=np.uint64)
        offsets_cat = np.concatenate([np.asarray(f["offsets"], dtype=np.uint32) for f in flats])
        arcs_cat = np.concatenate([np.asarray(f["arcs"], dtype=TR_DTYPE) for f in flats])
        finals_cat = np.concatenate([np.asarray(f["finals"], dtype=np.float32) for f in flats])
        outs = (C.c_void_p * n)()
        check(_lib.lib().wfst_fst_upload_many(ctx._h, n, n_states.ctypes.data, starts.ctypes.data,
                                              offsets_cat.ctypes.data, arcs_cat.ctypes.data, finals_cat.ctypes.data,
                                              props.ctypes.data, outs), "wfst_fst_upload_many")
        return [cls(C.c_void_p(outs[i]), ctx) for i in range(n)]

    @classmethod
    def from_bytes(cls, data: bytes, ctx: Optional[Context] = None) -> "DeviceFst":
        ctx = ctx or default_context()
        h = C.c_void_p()
        check(_lib.lib().wfst_fst_from_openfst_bytes(ctx._h, data, len(data), C.byref(h)),
              "wfst_fst_from_openfst_bytes")
        return cls(h, ctx)

    def to_bytes(self, fst_type: str = "vector") -> bytes:
        """OpenFST binary: "vector" (VectorFst::store) or "const" (ConstFst::store, version 2)."""
        if fst_type not in ("vector", "const"):
            raise ValueError("fst_type must be 'vector' or 'const'")
        p = C.c_void_p()
        n = C.c_size_t()
        fn = _lib.lib().wfst_fst_to_openfst_bytes if fst_type == "vector" else _lib.lib().wfst_fst_to_openfst_const_bytes
        check(fn(self._h, C.byref(p), C.byref(n)), "wfst_fst_to_openfst_bytes")
        try:
            return C.string_at(p.value, n.value)
        finally:
            _lib.lib().wfst_bytes_destroy(p)

    def info(self):
        n, a, s, p = C.c_uint32(), C.c_uint64(), C.c_int64(), C.c_uint64()
        check(_lib.lib().wfst_fst_info(self._h, C.byref(n), C.byref(a), C.byref(s), C.byref(p)))
        return n.value, a.value, (None if s.value < 0 else s.value), p.value

    @property
    def num_states(self):
        return self.info()[0]

    @property
    def num_arcs(self):
        return self.info()[1]

    @property
    def start(self):
        return self.info()[2]

    @property
    def properties(self):
        return self.info()[3]

    def to_flat(self) -> dict:
        n, a, start, props = self.info()
        offsets = np.zeros(n + 1, dtype=np.uint32)
        arcs = np.zeros(a, dtype=TR_DTYPE)
        finals = np.zeros(n, dtype=np.float32)
        check(_lib.lib().wfst_fst_download(self._h, offsets.ctypes.data, arcs.ctypes.data, finals.ctypes.data),
              "wfst_fst_download")
        return dict(n_states=n, start=start, offsets=offsets, arcs=arcs, finals=finals, props=props)

    def to_vector_fst(self) -> "VectorFst":
        v = C.c_void_p()
        check(_lib.lib().wfst_vec_fst_from_device(self._h, C.byref(v)), "wfst_vec_fst_from_device")
        return VectorFst(ptr=v, ctx=self.ctx)

    # algorithms on device handles (no host round trip of the operands)
    def compose(self, other: "DeviceFst", config: Optional["ComposeConfig"] = None) -> "DeviceFst":
        out = C.c_void_p()
        cfg = config._c(matchers=True) if config is not None else None
        if config is not None and (config.matcher1_config is not None or config.matcher2_config is not None):
            m1, m2 = config.matcher1_config, config.matcher2_config  # (kept alive over the call: they own the allowed arrays)
            check(_lib.lib().wfst_compose_with_matchers(self.ctx._h, self._h, other._h, cfg, m1._c() if m1 else None,
                                                        m2._c() if m2 else None, C.byref(out)), "Error during composition")
            return DeviceFst(out, self.ctx)
        check(_lib.lib().wfst_compose(self.ctx._h, self._h, other._h, cfg, C.byref(out)), "Error during composition")
        return DeviceFst(out, self.ctx)

    def shortest_path(self, config: Optional["ShortestPathConfig"] = None) -> "DeviceFst":
        out = C.c_void_p()
        cfg = config._c() if config is not None else None
        check(_lib.lib().wfst_shortest_path(self.ctx._h, self._h, cfg, C.byref(out)), "Error computing shortest path")
        return DeviceFst(out, self.ctx)

    def shortest_path_begin(self, config: Optional["ShortestPathConfig"] = None, ctx: Optional["Context"] = None) -> "ShortestPathJob":
        """Queue shortest_path (nshortest = 1) on this FST's context (or on `ctx`: a handle may be queried from several
        contexts of its device) and return at once (wfst_shortest_path_begin); job.finish() returns what shortest_path() returns."""
        job = C.c_void_p()
        cfg = config._c() if config is not None else None
        check(_lib.lib().wfst_shortest_path_begin((ctx or self.ctx)._h, self._h, cfg, C.byref(job)), "Error computing shortest path")
        return ShortestPathJob(job, self)

    def reverse(self) -> "DeviceFst":
        """algorithms::reverse (reverse.rs:33-87): new FST with a super-initial state 0."""
        out = C.c_void_p()
        check(_lib.lib().wfst_reverse(self.ctx._h, self._h, C.byref(out)), "Error during reverse")
        return DeviceFst(out, self.ctx)

    def rm_epsilon(self) -> "DeviceFst":
        """algorithms::rm_epsilon, default config (rm_epsilon_static.rs:50-163): a NEW FST without epsilon:epsilon arcs."""
        out = C.c_void_p()
        check(_lib.lib().wfst_rm_epsilon(self.ctx._h, self._h, C.byref(out)), "Error during rm_epsilon")
        return DeviceFst(out, self.ctx)

    def top_sort(self) -> "DeviceFst":
        """algorithms::top_sort (top_sort.rs:76-94): a NEW FST.  Acyclic content: the states in the reference's depth-first
        order and ACYCLIC | INITIAL_ACYCLIC | TOP_SORTED in the word; a cycle anywhere: a copy with CYCLIC | NOT_TOP_SORTED."""
        out = C.c_void_p()
        check(_lib.lib().wfst_top_sort(self.ctx._h, self._h, C.byref(out)), "Error during top_sort")
        return DeviceFst(out, self.ctx)

    def state_sort(self, order) -> "DeviceFst":
        """algorithms::state_sort (state_sort.rs:16-78): a NEW FST in which state order[s] is this FST's state s."""
        arr = np.ascontiguousarray(np.asarray(order, dtype=np.uint32))
        out = C.c_void_p()
        check(_lib.lib().wfst_state_sort(self.ctx._h, self._h, arr.ctypes.data, arr.size, C.byref(out)), "Error during state_sort")
        return DeviceFst(out, self.ctx)

    def connect(self) -> "DeviceFst":
        """algorithms::connect (connect.rs:51-66): a NEW FST with the accessible and coaccessible states only."""
        out = C.c_void_p()
        check(_lib.lib().wfst_connect(self.ctx._h, self._h, C.byref(out)), "Error during connect")
        return DeviceFst(out, self.ctx)

    def project(self, proj_type: Optional["ProjectType"] = None) -> "DeviceFst":
        """In-place projection on the device (algorithms/projection.rs:65-95): PROJECT_INPUT copies the input labels
        over the output labels, PROJECT_OUTPUT the other way round."""
        out = proj_type is not None and ProjectType(proj_type) == ProjectType.PROJECT_OUTPUT
        check(_lib.lib().wfst_fst_project(self.ctx._h, self._h, 1 if out else 0), "Error during projection")
        return self

    def invert(self) -> "DeviceFst":
        """In-place inversion on the device (algorithms/inversion.rs:32-48): every arc's input and output label change
        places, the property word follows invert_properties.  Returns this FST."""
        check(_lib.lib().wfst_fst_invert(self.ctx._h, self._h), "Error during invert")
        return self

    def isomorphic(self, other: "DeviceFst", delta: Optional[float] = None) -> bool:
        """algorithms::isomorphic_with_config (isomorphic.rs:134-158, 200-212) of this FST and `other` on the device; delta
        None: IsomorphicConfig::default() (KDELTA).  The reference's verdict, not symmetric in the operands; raises WfstError
        with the reference's message where it reports non-determinism.  Both FSTs are left as they are."""
        cfg = None if delta is None else C.byref(_lib.IsomorphicConfig(float(delta)))
        res = C.c_int()
        check(_lib.lib().wfst_isomorphic(self.ctx._h, self._h, other._h, cfg, C.byref(res)), "Error checking isomorphic FSTs")
        return bool(res.value)

    def paths(self, max_paths: int = 1 << 20) -> "PathTable":
        """Fst::paths_iter (fst_traits/paths_iterator.rs:24-62) on the device (wfst_fst_paths): every successful path in the
        reference's order — (number of arcs, arc positions) — as a PathTable, weights bit for bit.  Raises WfstError when a
        cycle is accessible from the start state (the reference would never return) and when the FST has more than
        max_paths paths, which is decided before any per-path memory is taken."""
        out = C.c_void_p()
        check(_lib.lib().wfst_fst_paths(self.ctx._h, self._h, int(max_paths), C.byref(out)), "Error enumerating paths")
        return PathTable._take(out, self.ctx)

    def count_paths(self) -> int:
        """The number of successful paths (wfst_fst_count_paths), saturated at 2^64 - 1; raises WfstError when a cycle is
        accessible from the start state."""
        res = C.c_uint64()
        check(_lib.lib().wfst_fst_count_paths(self.ctx._h, self._h, C.byref(res)), "Error counting paths")
        return int(res.value)

    def tr_sort(self, ilabel_cmp: bool = True) -> "DeviceFst":
        """In-place stable per-state arc sort on the device by ilabel (ILabelCompare) or olabel
        (OLabelCompare) + the reference's property update: algorithms/tr_sort.rs:13-62,
        rustfst-python fst.tr_sort (rustfst/algorithms/tr_sort.py)."""
        check(_lib.lib().wfst_fst_tr_sort(self.ctx._h, self._h, 1 if ilabel_cmp else 0), "Error during tr_sort")
        return self

    def set_start(self, state: int) -> "DeviceFst":
        """MutableFst::set_start (fst_impls/vector_fst/mutable_fst.rs:35-44) on the device-resident handle: the arcs stay in
        HBM, the derived data that does not depend on the start state stays cached.  KO for a state beyond the FST."""
        check(_lib.lib().wfst_fst_set_start(self.ctx._h, self._h, int(state)), "Error setting start state")
        return self

    def shortest_distance(self, want_hops: bool = False, reverse: bool = False, delta: Optional[float] = None):
        """Distances from the start state (wfst_shortest_distance), or with reverse=True the distances TO the final states
        (shortest_distance(fst, true), shortest_distance.rs:322-334; wfst_shortest_distance_with_config): n_states
        entries, +inf where the reference's Vec ends.  `delta` is checked (finite, >= 0); the device returns the exact
        fixed point.  hops exist for the forward search only."""
        if reverse or delta is not None:
            if want_hops:
                raise ValueError("want_hops is not available with reverse=True or a delta")
            return self.shortest_distance_with_len(reverse=reverse, delta=delta)[0]
        n = self.num_states
        dist = np.zeros(n, dtype=np.float32)
        hops = np.zeros(n, dtype=np.uint32) if want_hops else None
        check(_lib.lib().wfst_shortest_distance(self.ctx._h, self._h, dist.ctypes.data,
                                                hops.ctypes.data if want_hops else None), "wfst_shortest_distance")
        return (dist, hops) if want_hops else dist

    def shortest_distance_with_len(self, reverse: bool = False, delta: Optional[float] = None):
        """(distance[n_states], len): len is the length of the reference's Vec (wfst_shortest_distance_with_config);
        distance[:len] is what shortest_distance_with_config returns."""
        n = self.num_states
        dist = np.zeros(n, dtype=np.float32)
        ln = C.c_uint32()
        cfg = _lib.ShortestDistanceConfig(1 if reverse else 0, KSHORTESTDELTA if delta is None else float(delta))
        check(_lib.lib().wfst_shortest_distance_with_config(self.ctx._h, self._h, C.byref(cfg), dist.ctypes.data,
                                                            C.byref(ln)), "wfst_shortest_distance_with_config")
        return dist, ln.value

    def reweight(self, potentials, reweight_type: "ReweightType") -> "DeviceFst":
        """algorithms::reweight (reweight.rs:29-154) with the given potentials (+inf = zero; states past the end have
        potential zero): a NEW FST."""
        pot = np.ascontiguousarray(potentials, dtype=np.float32)
        out = C.c_void_p()
        check(_lib.lib().wfst_reweight(self.ctx._h, self._h, pot.ctypes.data if pot.size else None, int(pot.size),
                                       ReweightType(reweight_type).value, C.byref(out)), "Error during reweight")
        return DeviceFst(out, self.ctx)

    def push_weights(self, reweight_type: "ReweightType", config: Optional["PushWeightsConfig"] = None) -> "DeviceFst":
        """algorithms::push_weights_with_config (push.rs:89-118): a NEW FST."""
        out = C.c_void_p()
        cfg = config._c() if config is not None else None
        check(_lib.lib().wfst_push_weights(self.ctx._h, self._h, ReweightType(reweight_type).value, cfg, C.byref(out)),
              "Error during push_weights")
        return DeviceFst(out, self.ctx)

    def determinize(self, config: Optional["DeterminizeConfig"] = None) -> "DeviceFst":
        """algorithms::determinize_with_config (determinize_static.rs:149-190) of an acceptor (wfst_determinize): a NEW
        FST.  A word without ACCEPTOR (a transducer) raises WfstError: that path stays on rustfst."""
        out = C.c_void_p()
        cfg = config._c() if config is not None else None
        check(_lib.lib().wfst_determinize(self.ctx._h, self._h, cfg, C.byref(out)), "Error during determinization")
        return DeviceFst(out, self.ctx)

    def minimize(self, config: Optional["MinimizeConfig"] = None) -> "DeviceFst":
        """algorithms::minimize_with_config (minimize.rs:92-176) of an input-deterministic acyclic acceptor
        (wfst_minimize): a NEW FST, this one is left as it is.  Transducers, non-deterministic and cyclic inputs raise
        WfstError: those paths stay on rustfst."""
        out = C.c_void_p()
        cfg = config._c() if config is not None else None
        check(_lib.lib().wfst_minimize(self.ctx._h, self._h, cfg, C.byref(out)), "Error during minimization")
        return DeviceFst(out, self.ctx)

    def tr_sum(self) -> "DeviceFst":
        """algorithms::tr_sum (tr_sum.rs:7-22, wfst_tr_sum): a NEW FST in which arcs of one state with equal
        (ilabel, olabel, nextstate) are merged, their weights summed (tropical: the smallest); arcs come out sorted on
        that key."""
        out = C.c_void_p()
        check(_lib.lib().wfst_tr_sum(self.ctx._h, self._h, C.byref(out)), "Error during tr_sum")
        return DeviceFst(out, self.ctx)

    def tr_unique(self) -> "DeviceFst":
        """algorithms::tr_unique (tr_unique.rs:38-51, wfst_tr_unique): a NEW FST with a single instance of arcs of one
        state that agree in labels, nextstate and (within KDELTA) weight; arcs come out sorted on the key."""
        out = C.c_void_p()
        check(_lib.lib().wfst_tr_unique(self.ctx._h, self._h, C.byref(out)), "Error during tr_unique")
        return DeviceFst(out, self.ctx)

    def optimize(self) -> "DeviceFst":
        """algorithms::optimize (optimize.rs:11-128, wfst_optimize): rm_epsilon, tr_sum, then determinize + minimize (through
        a label encoding for transducers) of an ACYCLIC FST: a NEW FST.  Inputs whose property word does not hold ACYCLIC
        (unless it holds I_DETERMINISTIC) raise WfstError: those stay on rustfst."""
        out = C.c_void_p()
        check(_lib.lib().wfst_optimize(self.ctx._h, self._h, C.byref(out)), "Error during optimize")
        return DeviceFst(out, self.ctx)

    def union(self, other: "DeviceFst") -> "DeviceFst":
        """algorithms::union (union/union_static.rs:55-118, wfst_union): a NEW FST equal to what the reference leaves in
        its first operand; this FST and `other` are left as they are.  The result is in general not label-sorted."""
        out = C.c_void_p()
        check(_lib.lib().wfst_union(self.ctx._h, self._h, other._h, C.byref(out)), "Error during union")
        return DeviceFst(out, self.ctx)

    def concat(self, other: "DeviceFst") -> "DeviceFst":
        """algorithms::concat (concat/concat_static.rs:53-109, wfst_concat): a NEW FST, the operands are left as they are."""
        out = C.c_void_p()
        check(_lib.lib().wfst_concat(self.ctx._h, self._h, other._h, C.byref(out)), "Error during concat")
        return DeviceFst(out, self.ctx)

    def closure(self, closure_type: "ClosureType") -> "DeviceFst":
        """algorithms::closure (closure/closure_static.rs:25-73, wfst_closure): a NEW FST, this one is left as it is."""
        out = C.c_void_p()
        check(_lib.lib().wfst_closure(self.ctx._h, self._h, ClosureType(closure_type).value, C.byref(out)),
              "Error during closure")
        return DeviceFst(out, self.ctx)


class HandleArray:
    """A batch of DeviceFst handles marshalled once for the C-ABI (`const wfst_fst* const*`): callers that submit the
    same acceptors repeatedly build it once instead of paying the ctypes marshalling on every call."""

    def __init__(self, fsts: Sequence["DeviceFst"]):
        self._keep = list(fsts)
        n = len(self._keep)
        self._arr = (C.c_void_p * n)(*[a._h.value if isinstance(a._h, C.c_void_p) else a._h for a in self._keep])

    def __len__(self):
        return len(self._keep)


class PathList(Sequence):
    """The outs[] of a fused batch: owns the n result handles (released with ONE wfst_fst_destroy_many call) and
    hands out DeviceFst views on demand — a step that only forwards the results pays no per-path Python work."""

    def __init__(self, handles, n: int, ctx: Context):
        self._arr, self._n, self.ctx = handles, n, ctx

    def __len__(self):
        return self._n

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(self._n))]
        if i < 0:
            i += self._n
        if not 0 <= i < self._n:
            raise IndexError(i)
        return DeviceFst(C.c_void_p(self._arr[i]), self.ctx, owner=self)

    def __del__(self):
        arr = getattr(self, "_arr", None)
        if arr is not None:
            try:
                _lib.lib().wfst_fst_destroy_many(arr, self._n)
            except Exception:
                pass
            self._arr = None


class FstPath:
    """A successful path (rustfst/src/fst_path.rs:13-20): the input labels and the output labels with label 0 dropped per
    tape, and the weight.  == compares the labels exactly and the weight bit for bit."""

    __slots__ = ("ilabels", "olabels", "weight")

    def __init__(self, ilabels=(), olabels=(), weight: float = 0.0):
        self.ilabels = [int(l) for l in ilabels]
        self.olabels = [int(l) for l in olabels]
        self.weight = np.float32(weight)

    def __eq__(self, other):
        if not isinstance(other, FstPath):
            return NotImplemented
        return (self.ilabels, self.olabels) == (other.ilabels, other.olabels) and \
            self.weight.view(np.uint32) == other.weight.view(np.uint32)

    def __hash__(self):  # (fst_path.rs:76-82: labels and weight; consistent with ==)
        return hash((tuple(self.ilabels), tuple(self.olabels), int(self.weight.view(np.uint32))))

    def __repr__(self):
        return f"<FstPath ilabels={self.ilabels}, olabels={self.olabels}, weight={self.weight}>"


class PathTable(Sequence):
    """The downloaded table of wfst_fst_paths / wfst_fst_paths_batch: a sequence of FstPath in the reference's order over
    six numpy arrays, which a decoder may take as they are — `item_off` (rows of item i: item_off[i] .. item_off[i + 1]),
    `weights`, `ilabel_off` with `ilabels`, `olabel_off` with `olabels` (row k's labels: labels[off[k]:off[k + 1]])."""

    def __init__(self, item_off, weights, ilabel_off, ilabels, olabel_off, olabels):
        self.item_off, self.weights = item_off, weights
        self.ilabel_off, self.ilabels, self.olabel_off, self.olabels = ilabel_off, ilabels, olabel_off, olabels

    @classmethod
    def _take(cls, handle, ctx: "Context") -> "PathTable":
        """downloads the table behind `handle` and destroys it"""
        L = _lib.lib()
        try:
            counts = [C.c_uint64() for _ in range(4)]
            check(L.wfst_paths_info(handle, *[C.byref(c) for c in counts]), "wfst_paths_info")
            n_items, n_paths, n_il, n_ol = (int(c.value) for c in counts)
            item_off, weights = np.zeros(n_items + 1, np.uint64), np.zeros(n_paths, np.float32)
            iloff, il = np.zeros(n_paths + 1, np.uint64), np.zeros(n_il, np.uint32)
            oloff, ol = np.zeros(n_paths + 1, np.uint64), np.zeros(n_ol, np.uint32)
            check(L.wfst_paths_download(ctx._h, handle, item_off.ctypes.data, weights.ctypes.data, iloff.ctypes.data,
                                        il.ctypes.data, oloff.ctypes.data, ol.ctypes.data), "wfst_paths_download")
        finally:
            L.wfst_paths_destroy(handle)
        return cls(item_off, weights, iloff, il, oloff, ol)

    @property
    def num_items(self) -> int:
        return len(self.item_off) - 1

    def __len__(self):
        return len(self.weights)

    def __getitem__(self, k):
        if isinstance(k, slice):
            return [self[j] for j in range(*k.indices(len(self)))]
        if k < 0:
            k += len(self)
        if not 0 <= k < len(self):
            raise IndexError(k)
        return FstPath(self.ilabels[int(self.ilabel_off[k]):int(self.ilabel_off[k + 1])],
                       self.olabels[int(self.olabel_off[k]):int(self.olabel_off[k + 1])], self.weights[k])

    def item(self, i: int) -> "PathTable":
        """the rows of item i as a table of one item (views of this table's arrays, offsets rebased)"""
        if not 0 <= i < self.num_items:
            raise IndexError(i)
        b, e = int(self.item_off[i]), int(self.item_off[i + 1])
        iloff, oloff = self.ilabel_off[b:e + 1], self.olabel_off[b:e + 1]
        return PathTable(np.array([0, e - b], np.uint64), self.weights[b:e], iloff - iloff[0],
                         self.ilabels[int(iloff[0]):int(iloff[-1])], oloff - oloff[0], self.olabels[int(oloff[0]):int(oloff[-1])])


DEFAULT_MAX_PATHS = 1 << 20


def paths_batch(fsts: Sequence["DeviceFst"], max_paths: int = DEFAULT_MAX_PATHS, ctx: Optional[Context] = None,
                return_in_kernel: bool = False):
    """[f.paths(max_paths) for f in fsts] as ONE call and ONE table (wfst_fst_paths_batch): the items of at most 4096
    states and 16384 arcs — the n-best results of a decoding batch — are counted by one launch, one workgroup each, and
    the paths of all items are unranked, ordered and written together.  max_paths applies per item.
    return_in_kernel: also the uint8 array that says which items the batch kernel counted."""
    n = len(fsts)
    if ctx is None:
        ctx = _first_ctx(fsts) if n else default_context()
    out = C.c_void_p()
    flags = np.zeros(n, np.uint8)
    check(_lib.lib().wfst_fst_paths_batch(ctx._h, _handles(fsts), n, int(max_paths), C.byref(out), flags.ctypes.data),
          "wfst_fst_paths_batch")
    table = PathTable._take(out, ctx)
    return (table, flags) if return_in_kernel else table


class LookAhead:
    """Look-ahead composition set up on a first operand (wfst_lookahead_*): what the reference builds with
    MatcherFst::new_with_relabeling + LabelLookAheadMatcher + PushLabels(PushWeights(LookAhead(AltSequence)))
    (rustfst-cli/src/cmds/compose.rs:77-181).

        la = LookAhead(fst1_on_device)           # reachability data + relabelled fst1 (MatcherFst::new)
        fst2r = la.relabel(fst2_on_device)        # LabelLookAheadRelabeler::relabel + tr_sort(ILabelCompare)
        out = la.compose(fst2r)                   # ComposeFst(..).compute(), not connected
    """

    def __init__(self, fst1: Optional["DeviceFst"] = None, _handle=None, _ctx=None):
        if _handle is not None:
            self._h, self.ctx = _handle, _ctx
            return
        h = C.c_void_p()
        check(_lib.lib().wfst_lookahead_create(fst1.ctx._h, fst1._h, C.byref(h)), "wfst_lookahead_create")
        self._h, self.ctx = h, fst1.ctx

    @classmethod
    def reachable_from_arrays(cls, n_states: int, offsets, arcs, finals, reach_input: bool = False) -> "LookAhead":
        """Host-only handle: LabelReachable::compute_data on flat CSR arrays (no GPU); serves data() only."""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint32)
        arcs = np.ascontiguousarray(arcs, dtype=TR_DTYPE)
        finals = np.ascontiguousarray(finals, dtype=np.float32)
        h = C.c_void_p()
        check(_lib.lib().wfst_label_reachable_compute(n_states, offsets.ctypes.data, arcs.ctypes.data if len(arcs) else None,
                                                      finals.ctypes.data if n_states else None, 1 if reach_input else 0,
                                                      C.byref(h)), "wfst_label_reachable_compute")
        return cls(_handle=h, _ctx=None)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                _lib.lib().wfst_lookahead_destroy(h)
            except Exception:
                pass
        self._h = None

    @property
    def fst1(self) -> "DeviceFst":
        """The relabelled, olabel-sorted first operand (a view: the handle stays owned by this object)."""
        h = C.c_void_p()
        check(_lib.lib().wfst_lookahead_fst1(self._h, C.byref(h)), "wfst_lookahead_fst1")
        return DeviceFst(h, self.ctx, owner=self)

    def relabel(self, fst2: "DeviceFst") -> "DeviceFst":
        out = C.c_void_p()
        check(_lib.lib().wfst_lookahead_relabel(self._h, fst2._h, C.byref(out)), "wfst_lookahead_relabel")
        return DeviceFst(out, fst2.ctx)

    def compose(self, relabeled_fst2: "DeviceFst", ctx: Optional[Context] = None) -> "DeviceFst":
        ctx = ctx or self.ctx
        out = C.c_void_p()
        check(_lib.lib().wfst_compose_lookahead(ctx._h, self._h, relabeled_fst2._h, C.byref(out)), "Error during look-ahead composition")
        return DeviceFst(out, ctx)

    def compose_batch(self, relabeled_fst2s: Sequence["DeviceFst"], ctx: Optional[Context] = None) -> List["DeviceFst"]:
        """n look-ahead compositions against this first operand in one launch (wfst_compose_lookahead_batch)."""
        ctx = ctx or self.ctx
        n = len(relabeled_fst2s)
        arr = (C.c_void_p * n)(*[f._h for f in relabeled_fst2s])
        outs = (C.c_void_p * n)()
        check(_lib.lib().wfst_compose_lookahead_batch(ctx._h, self._h, arr, n, outs), "Error during look-ahead composition")
        return [DeviceFst(C.c_void_p(outs[i]), ctx) for i in range(n)]

    def data(self) -> dict:
        """LabelReachableData: dict(final_label, label2index {label: index}, intervals [per state list of (begin, end)])."""
        n, ni, nl, fl = C.c_uint32(), C.c_uint64(), C.c_uint32(), C.c_uint32()
        check(_lib.lib().wfst_lookahead_info(self._h, C.byref(n), C.byref(ni), C.byref(nl), C.byref(fl)), "wfst_lookahead_info")
        off = np.zeros(n.value + 1, dtype=np.uint32)
        iv = np.zeros(2 * ni.value, dtype=np.uint32)
        labels = np.zeros(nl.value, dtype=np.uint32)
        idx = np.zeros(nl.value, dtype=np.uint32)
        check(_lib.lib().wfst_lookahead_download(self._h, off.ctypes.data, iv.ctypes.data if len(iv) else None,
                                                 labels.ctypes.data if nl.value else None,
                                                 idx.ctypes.data if nl.value else None), "wfst_lookahead_download")
        ivs = [[(int(iv[2 * k]), int(iv[2 * k + 1])) for k in range(off[s], off[s + 1])] for s in range(n.value)]
        return {"final_label": int(fl.value), "label2index": {int(l): int(i) for l, i in zip(labels, idx)}, "intervals": ivs}


class ShortestPathJob:
    """A single-shortest-path solve in flight (wfst_shortest_path_begin); finish() = wfst_shortest_path_end."""

    def __init__(self, job, fst):
        self._job, self._fst = job, fst  # the input FST must outlive the job

    def finish(self) -> "DeviceFst":
        if self._job is None:
            raise WfstError("shortest_path job already finished")
        out = C.c_void_p()
        job, self._job = self._job, None
        check(_lib.lib().wfst_shortest_path_end(job, C.byref(out)), "Error computing shortest path")
        fst, self._fst = self._fst, None
        return DeviceFst(out, fst.ctx)

    def __del__(self):
        if getattr(self, "_job", None) is not None:  # abandoned: wait for the kernels and free the job
            _lib.lib().wfst_shortest_path_end(self._job, None)
            self._job = None


class BatchJob:
    """A fused batch in flight (wfst_compose_shortest_path_batch_begin); finish() = ..._end."""

    def __init__(self, job, n, ctx, keep_alive):
        self._job, self._n, self._ctx, self._keep = job, n, ctx, keep_alive

    def finish(self):
        if self._job is None:
            raise WfstError("batch job already finished")
        outs = (C.c_void_p * self._n)()
        na = C.c_uint64()
        job, self._job = self._job, None
        check(_lib.lib().wfst_compose_shortest_path_batch_end(job, outs, C.byref(na)),
              "wfst_compose_shortest_path_batch_end")
        self._keep = None
        return PathList(outs, self._n, self._ctx), na.value

    def __del__(self):
        if getattr(self, "_job", None) is not None:  # abandoned: wait for the kernel and free the job
            _lib.lib().wfst_compose_shortest_path_batch_end(self._job, None, None)
            self._job = None


def compose_shortest_path_batch_begin(acceptors: Sequence[DeviceFst], t: DeviceFst,
                                      compose_config: Optional["ComposeConfig"] = None,
                                      shortest_path_config: Optional["ShortestPathConfig"] = None,
                                      ctx: Optional[Context] = None) -> BatchJob:
    """Enqueue the fused batch on `ctx`'s stream (default: t's context) and return at once; work issued
    afterwards on ANOTHER context (e.g. shortest_path of a large FST) overlaps with it on the GPU."""
    n = len(acceptors)
    ctx = ctx or t.ctx
    arr = acceptors._arr if isinstance(acceptors, HandleArray) else HandleArray(acceptors)._arr
    job = C.c_void_p()
    check(_lib.lib().wfst_compose_shortest_path_batch_begin(
        ctx._h, arr, n, t._h, compose_config._c() if compose_config else None,
        shortest_path_config._c() if shortest_path_config else None, C.byref(job)),
        "wfst_compose_shortest_path_batch_begin")
    return BatchJob(job, n, ctx, (acceptors, t, arr))


def compose_shortest_path_batch(acceptors: Sequence[DeviceFst], t: DeviceFst,
                                compose_config: Optional["ComposeConfig"] = None,
                                shortest_path_config: Optional["ShortestPathConfig"] = None,
                                ctx: Optional[Context] = None):
    """for a in acceptors: shortest_path(compose(a, t)) as one device-resident pipeline.
    Returns (list of DeviceFst paths, total composed arcs before trimming).  A `compose_config` that carries a MatcherConfig
    goes through wfst_compose_shortest_path_batch_with_matchers: strings against a sigma matcher on `t` run one wavefront
    each in one launch, everything else as compose + shortest_path per item (Context.sigma_batch_stats says which)."""
    n = len(acceptors)
    ctx = ctx or t.ctx
    arr = acceptors._arr if isinstance(acceptors, HandleArray) else HandleArray(acceptors)._arr
    outs = (C.c_void_p * n)()
    na = C.c_uint64()
    if compose_config is not None and (compose_config.matcher1_config is not None or compose_config.matcher2_config is not None):
        m1, m2 = compose_config.matcher1_config, compose_config.matcher2_config  # (kept alive over the call)
        check(_lib.lib().wfst_compose_shortest_path_batch_with_matchers(
            ctx._h, arr, n, t._h, compose_config._c(matchers=True), m1._c() if m1 else None, m2._c() if m2 else None,
            shortest_path_config._c() if shortest_path_config else None, outs, C.byref(na)),
            "wfst_compose_shortest_path_batch_with_matchers")
        return PathList(outs, n, ctx), na.value
    check(_lib.lib().wfst_compose_shortest_path_batch(
        ctx._h, arr, n, t._h, compose_config._c() if compose_config else None,
        shortest_path_config._c() if shortest_path_config else None, outs, C.byref(na)),
        "wfst_compose_shortest_path_batch")
    return PathList(outs, n, ctx), na.value


def compose_shortest_path_batch_packed(acceptors: Sequence[DeviceFst], t: DeviceFst, max_arcs: int,
                                       compose_config: Optional["ComposeConfig"] = None,
                                       shortest_path_config: Optional["ShortestPathConfig"] = None,
                                       ctx: Optional[Context] = None, out: Optional[np.ndarray] = None):
    """compose_shortest_path_batch with the results as one table instead of handles
    (wfst_compose_shortest_path_batch_packed): returns (uint32 array [n, 4 + 4 * max_arcs] in the record layout of
    dist.pack_paths / dist.unpack_paths, total composed arcs).  No per-path host object is built: the form for large batches.
    `out`: a C-contiguous uint32 array of that shape to fill (a caller that decodes batch after batch reuses one)."""
    n = len(acceptors)
    ctx = ctx or t.ctx
    arr = acceptors._arr if isinstance(acceptors, HandleArray) else HandleArray(acceptors)._arr
    shape = (n, 4 + 4 * int(max_arcs))
    if out is None:
        out = np.empty(shape, dtype=np.uint32)
    elif out.shape != shape or out.dtype != np.uint32 or not out.flags["C_CONTIGUOUS"]:
        raise ValueError(f"out must be a C-contiguous uint32 array of shape {shape}")
    na = C.c_uint64()
    check(_lib.lib().wfst_compose_shortest_path_batch_packed(
        ctx._h, arr, n, t._h, compose_config._c() if compose_config else None,
        shortest_path_config._c() if shortest_path_config else None, int(max_arcs), out.ctypes.data, C.byref(na)),
        "wfst_compose_shortest_path_batch_packed")
    return out, na.value


def shortest_path_batch(fsts: Sequence[DeviceFst], config: Optional["ShortestPathConfig"] = None,
                        ctx: Optional[Context] = None) -> List[DeviceFst]:
    """[f.shortest_path(config) for f in fsts] as ONE call (wfst_shortest_path_batch): with nshortest > 1 the small
    inputs — the composed lattices of a decoding batch — are searched by one launch, one wavefront each."""
    n = len(fsts)
    if n == 0:
        return []
    ctx = ctx or fsts[0].ctx
    arr = fsts._arr if isinstance(fsts, HandleArray) else (C.c_void_p * n)(*[f._h.value if isinstance(f._h, C.c_void_p) else f._h for f in fsts])
    outs = (C.c_void_p * n)()
    check(_lib.lib().wfst_shortest_path_batch(ctx._h, arr, n, config._c() if config is not None else None, outs),
          "wfst_shortest_path_batch")
    return [DeviceFst(C.c_void_p(outs[i]), ctx) for i in range(n)]


def _handles(fsts):
    n = len(fsts)
    return fsts._arr if isinstance(fsts, HandleArray) else (C.c_void_p * n)(*[f._h.value if isinstance(f._h, C.c_void_p) else f._h for f in fsts])


def _first_ctx(fsts):
    return (fsts._keep[0] if isinstance(fsts, HandleArray) else fsts[0]).ctx


def _batch_call(fn_name, fsts, ctx, want_flags, *config):
    """fn_name(ctx, fsts, n, *config, outs, in_kernel) of the one-workgroup-per-item batch calls: the results, and with
    want_flags the uint8 array in_kernel too"""
    n = len(fsts)
    if n == 0:
        return ([], np.zeros(0, np.uint8)) if want_flags else []
    ctx = ctx or _first_ctx(fsts)
    outs = (C.c_void_p * n)()
    flags = np.zeros(n, np.uint8)
    check(getattr(_lib.lib(), fn_name)(ctx._h, _handles(fsts), n, *config, outs, flags.ctypes.data), fn_name)
    res = [DeviceFst(C.c_void_p(outs[i]), ctx) for i in range(n)]
    return (res, flags) if want_flags else res


def determinize_batch(fsts: Sequence[DeviceFst], config: Optional["DeterminizeConfig"] = None,
                      ctx: Optional[Context] = None, want_flags: bool = False):
    """[f.determinize(config) for f in fsts] as ONE call (wfst_determinize_batch): one workgroup per acceptor, one launch
    for the batch — the form for the many small lattices of a decoding batch.  want_flags: also the uint8 array that
    says which items the batch kernel constructed (0: a level of more than 256 states or 8192 raw candidates sent the
    item through the single-FST path)."""
    return _batch_call("wfst_determinize_batch", fsts, ctx, want_flags, config._c() if config is not None else None)


def _list_call(fn_name, fsts, ctx, what):
    n = len(fsts)
    ctx = ctx or _first_ctx(fsts)
    out = C.c_void_p()
    check(getattr(_lib.lib(), fn_name)(ctx._h, _handles(fsts), n, C.byref(out)), what)
    return DeviceFst(out, ctx)


def _device_union_list(fsts: Sequence[DeviceFst], ctx: Optional[Context] = None) -> DeviceFst:
    """the left fold of union over device FSTs as ONE call (wfst_union_list): a NEW FST"""
    return _list_call("wfst_union_list", fsts, ctx, "Error during union")


def _device_concat_list(fsts: Sequence[DeviceFst], ctx: Optional[Context] = None) -> DeviceFst:
    """the left fold of concat over device FSTs as ONE call (wfst_concat_list): a NEW FST"""
    return _list_call("wfst_concat_list", fsts, ctx, "Error during concat")


def _device_replace(root_idx: int, fst_list, epsilon_on_replace: bool, ctx: Optional[Context] = None) -> DeviceFst:
    """replace over (label, DeviceFst) pairs as ONE call (wfst_replace): a NEW FST"""
    n = len(fst_list)
    ctx = ctx or (fst_list[0][1].ctx if n else default_context())
    pairs = (_lib.LabelFstPair * max(n, 1))()
    for i, (label, f) in enumerate(fst_list):
        pairs[i].label = int(label)
        pairs[i].fst = f._h.value if isinstance(f._h, C.c_void_p) else f._h
    out = C.c_void_p()
    check(_lib.lib().wfst_replace(ctx._h, int(root_idx), pairs, n, 1 if epsilon_on_replace else 0, C.byref(out)),
          "Error performing replace")
    return DeviceFst(out, ctx)


def determinize_batch_stats(ctx: Optional[Context] = None) -> dict:
    """The last determinize_batch / determinize_with_distance_batch call of ctx (wfst_ctx_get_determinize_batch_stats)."""
    return _counters("determinize_batch", ctx or default_context())


def rm_epsilon_stats(ctx: Optional[Context] = None) -> dict:
    """The last rm_epsilon call of ctx (wfst_ctx_get_rm_epsilon_stats)."""
    return _counters("rm_epsilon", ctx or default_context())


def minimize_batch(fsts: Sequence[DeviceFst], config: Optional["MinimizeConfig"] = None, ctx: Optional[Context] = None,
                   return_in_kernel: bool = False):
    """[f.minimize(config) for f in fsts] as ONE call (wfst_minimize_batch): one workgroup per acceptor and one launch
    of the batch kernel for the whole list, whatever its length and the items' depths — the step after determinize_batch for the many small
    lattices of a decoding batch.  return_in_kernel: also the uint8 array that says which items the batch kernel
    minimized (0: more than 4096 states or 16384 arcs sent the item through the single-FST path).  Any item that
    f.minimize would refuse raises WfstError with "item <i>: " in front of that call's message."""
    return _batch_call("wfst_minimize_batch", fsts, ctx, return_in_kernel, config._c() if config is not None else None)


def minimize_batch_stats(ctx: Optional[Context] = None) -> dict:
    """The last minimize_batch call of ctx (wfst_ctx_get_minimize_batch_stats)."""
    return _counters("minimize_batch", ctx or default_context())


def rm_epsilon_batch(fsts: Sequence[DeviceFst], ctx: Optional[Context] = None, return_in_kernel: bool = False):
    """[f.rm_epsilon() for f in fsts] as ONE call (wfst_rm_epsilon_batch): one workgroup per FST, and a number of launches
    that depends neither on the length of the list nor on any item's epsilon depth — the step in front of
    determinize_batch and minimize_batch for the many small lattices of a decoding batch.  return_in_kernel: also the uint8
    array that says which items the batch kernel finished (0: more than 4096 states or 16384 arcs, an epsilon cycle, or a
    rewritten state beyond a closure of 64 states, 128 stack entries or 128 arcs sent the item through the single-FST
    path).  Any item that f.rm_epsilon would refuse raises WfstError with "item <i>: " in front of that call's message."""
    return _batch_call("wfst_rm_epsilon_batch", fsts, ctx, return_in_kernel)


def rm_epsilon_batch_stats(ctx: Optional[Context] = None) -> dict:
    """The last rm_epsilon_batch call of ctx (wfst_ctx_get_rm_epsilon_batch_stats)."""
    return _counters("rm_epsilon_batch", ctx or default_context())


def tr_sum_batch(fsts: Sequence[DeviceFst], ctx: Optional[Context] = None, return_in_kernel: bool = False):
    """[f.tr_sum() for f in fsts] as ONE call (wfst_tr_sum_batch): one workgroup per FST and one launch for the whole
    list — the step between rm_epsilon_batch and determinize_batch.  return_in_kernel: also the uint8 array that says
    which items the batch kernel finished (0: more than 4096 states or 16384 arcs, or a state with more than 256 arcs,
    sent the item through the single-FST path)."""
    return _batch_call("wfst_tr_sum_batch", fsts, ctx, return_in_kernel)


def tr_unique_batch(fsts: Sequence[DeviceFst], ctx: Optional[Context] = None, return_in_kernel: bool = False):
    """[f.tr_unique() for f in fsts] as ONE call (wfst_tr_unique_batch); see tr_sum_batch."""
    return _batch_call("wfst_tr_unique_batch", fsts, ctx, return_in_kernel)


def tr_sum_batch_stats(ctx: Optional[Context] = None) -> dict:
    """The last tr_sum_batch / tr_unique_batch call of ctx (wfst_ctx_get_tr_sum_batch_stats)."""
    return _counters("tr_sum_batch", ctx or default_context())


def top_sort_batch(fsts: Sequence[DeviceFst], ctx: Optional[Context] = None, return_in_kernel: bool = False):
    """[f.top_sort() for f in fsts] as ONE call (wfst_top_sort_batch): one workgroup per FST and one launch for the whole
    list, whatever its length and the items' depths — the step between a list of compositions or unions and
    optimize_batch, which wants ACYCLIC in the word.  A cyclic item comes back as a copy with CYCLIC | NOT_TOP_SORTED, as
    from top_sort.  return_in_kernel: also the uint8 array that says which items the batch kernel finished (0: more than
    4096 states or 16384 arcs sent the item through the single-FST path).  An item with states but no start state raises
    WfstError with "item <i>: " in front of top_sort's message."""
    return _batch_call("wfst_top_sort_batch", fsts, ctx, return_in_kernel)


def top_sort_batch_stats(ctx: Optional[Context] = None) -> dict:
    """The last top_sort_batch call of ctx (wfst_ctx_get_top_sort_batch_counters): launches, items_in_kernel, items_single."""
    ctx = ctx or default_context()
    vals = [C.c_uint64() for _ in _lib.TOP_SORT_BATCH_COUNTERS]
    check(_lib.lib().wfst_ctx_get_top_sort_batch_counters(ctx._h, *[C.byref(v) for v in vals]),
          "wfst_ctx_get_top_sort_batch_counters")
    return {k: int(v.value) for k, v in zip(_lib.TOP_SORT_BATCH_COUNTERS, vals)}


def compose_batch(fst1s, fst2s, config: Optional["ComposeConfig"] = None, ctx: Optional[Context] = None,
                  return_in_kernel: bool = False):
    """[a.compose(b, config) for a, b in zip(fst1s, fst2s)] as ONE call (wfst_compose_batch): one wavefront per pair, each
    with its own second operand and its own arena, results bit for bit the single call's.  Either side may be a single
    DeviceFst (or a list of one), which then serves every item: one grammar against n lattices, one lattice against n
    grammars.  return_in_kernel: also the uint8 array that says which items the batch kernel finished (0: the only item
    with start states, which is the single call, or an item whose estimate passed 16384 composed states and went to the
    wide driver).  A config with matcher configs is refused; an item's own error raises WfstError with "item <i>: " in
    front."""
    if isinstance(fst1s, DeviceFst):
        fst1s = [fst1s]
    if isinstance(fst2s, DeviceFst):
        fst2s = [fst2s]
    cfg = config._c() if config is not None else None
    n1, n2 = len(fst1s), len(fst2s)
    n = max(n1, n2)
    if ctx is None:
        ctx = _first_ctx(fst1s) if n1 else (_first_ctx(fst2s) if n2 else default_context())
    outs = (C.c_void_p * max(n, 1))()
    flags = np.zeros(n, np.uint8)
    check(_lib.lib().wfst_compose_batch(ctx._h, _handles(fst1s), n1, _handles(fst2s), n2, cfg, outs, flags.ctypes.data),
          "wfst_compose_batch")
    res = [DeviceFst(C.c_void_p(outs[i]), ctx) for i in range(n)]
    return (res, flags) if return_in_kernel else res


def compose_batch_stats(ctx: Optional[Context] = None) -> dict:
    """The last compose_batch call of ctx that passed its argument checks (wfst_ctx_get_compose_batch_counters): launches,
    items_in_kernel, items_single, items_no_start, regrown_states, regrown_arcs, regrown_hash."""
    ctx = ctx or default_context()
    vals = [C.c_uint64() for _ in _lib.COMPOSE_BATCH_COUNTERS]
    check(_lib.lib().wfst_ctx_get_compose_batch_counters(ctx._h, *[C.byref(v) for v in vals]),
          "wfst_ctx_get_compose_batch_counters")
    return {k: int(v.value) for k, v in zip(_lib.COMPOSE_BATCH_COUNTERS, vals)}


def optimize_batch(fsts: Sequence[DeviceFst], ctx: Optional[Context] = None, return_in_kernel: bool = False):
    """[f.optimize() for f in fsts] as ONE call (wfst_optimize_batch): rm_epsilon_batch over the items whose word lacks
    NO_EPSILONS, tr_sum_batch over all, determinize_batch and minimize_batch over the acceptors; a transducer takes the
    label encoding of the single call on its own.  return_in_kernel: also the uint8 array that says which items every
    stage ran in its batch kernel (0 for a transducer).  Any item that f.optimize would refuse raises WfstError with
    "item <i>: " in front of that call's message, for the lowest such i."""
    return _batch_call("wfst_optimize_batch", fsts, ctx, return_in_kernel)


def optimize_batch_stats(ctx: Optional[Context] = None) -> dict:
    """The last optimize_batch call of ctx (wfst_ctx_get_optimize_batch_stats): launches per stage, items by flag, and
    the transducers among the items_single."""
    ctx = ctx or default_context()
    launches = (C.c_uint64 * 4)()
    a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
    check(_lib.lib().wfst_ctx_get_optimize_batch_stats(ctx._h, launches, C.byref(a), C.byref(b), C.byref(c)),
          "wfst_ctx_get_optimize_batch_stats")
    return dict(launches=dict(zip(("rm_epsilon", "tr_sum", "determinize", "minimize"), (int(x) for x in launches))),
                items_in_kernel=a.value, items_single=b.value, items_transducer=c.value)


def _take_floats(ptr, count):
    out = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_float)), shape=(count,)).copy() if count else np.zeros(0, np.float32)
    _lib.lib().wfst_bytes_destroy(ptr)
    return out


def determinize_with_distance(fst: DeviceFst, in_dist, delta: float = KDELTA):
    """algorithms::determinize_with_distance (determinize_static.rs:24-39, wfst_determinize_with_distance): the
    determinized acceptor (a NEW FST) and out_dist, where out_dist[s] is the sum over the elements (q, w) of subset s
    of w * in_dist[q]; states beyond len(in_dist) count as +inf."""
    d = np.ascontiguousarray(in_dist, np.float32)
    out, ptr, cnt = C.c_void_p(), C.c_void_p(), C.c_uint64()
    check(_lib.lib().wfst_determinize_with_distance(fst.ctx._h, fst._h, d.ctypes.data if len(d) else None, len(d), delta,
                                                    C.byref(out), C.byref(ptr), C.byref(cnt)),
          "Error during determinize_with_distance")
    return DeviceFst(out, fst.ctx), _take_floats(ptr, cnt.value)


def determinize_with_distance_batch(fsts: Sequence[DeviceFst], in_dists, delta: float = KDELTA,
                                    ctx: Optional[Context] = None, want_flags: bool = False):
    """[determinize_with_distance(f, d, delta) for f, d in zip(fsts, in_dists)] as ONE call
    (wfst_determinize_with_distance_batch): a list of (DeviceFst, np.ndarray)."""
    n = len(fsts)
    if len(in_dists) != n:
        raise ValueError("one in_dist per FST")
    if n == 0:
        return ([], np.zeros(0, np.uint8)) if want_flags else []
    ctx = ctx or _first_ctx(fsts)
    ds = [np.ascontiguousarray(d, np.float32) for d in in_dists]
    ptrs = (C.c_void_p * n)(*[d.ctypes.data if len(d) else None for d in ds])
    lens = (C.c_uint64 * n)(*[len(d) for d in ds])
    outs = (C.c_void_p * n)()
    off = (C.c_uint64 * (n + 1))()
    flags = np.zeros(n, np.uint8)
    ptr = C.c_void_p()
    check(_lib.lib().wfst_determinize_with_distance_batch(ctx._h, _handles(fsts), n, ptrs, lens, delta, outs, C.byref(ptr),
                                                          off, flags.ctypes.data), "wfst_determinize_with_distance_batch")
    cat = _take_floats(ptr, off[n])
    res = [(DeviceFst(C.c_void_p(outs[i]), ctx), cat[off[i]:off[i + 1]].copy()) for i in range(n)]
    return (res, flags) if want_flags else res


def last_nbest_path(ctx: Optional[Context] = None) -> str:
    """Which search the last shortest_path_batch(nshortest > 1) used (wfst_stats.nbest_device_problems)."""
    ctx = ctx or default_context()
    return "wave kernel: %d inputs" % int(ctx.stats()["nbest_device_problems"])


# ------------------------------------------------------------------ configs
class ProjectType(Enum):  # rustfst-python/rustfst/algorithms/project.py:9-24
    PROJECT_INPUT = 0
    PROJECT_OUTPUT = 1


class ComposeFilter(Enum):  # rustfst-python/rustfst/algorithms/compose.py:55-62
    AUTOFILTER = 0
    NULLFILTER = 1
    TRIVIALFILTER = 2
    SEQUENCEFILTER = 3
    ALTSEQUENCEFILTER = 4
    MATCHFILTER = 5
    NOMATCHFILTER = 6


class MatcherRewriteMode(Enum):  # rustfst-python/rustfst/algorithms/compose.py:16-19
    AUTO = 0
    ALWAYS = 1
    NEVER = 2


class MatcherConfig:
    """rustfst-python/rustfst/algorithms/compose.py:26-53: a sigma matcher for one side of a composition.  An arc labelled
    `sigma_label` on the side's matched tape stands for any label the state does not carry explicitly — any of
    `sigma_allowed_matches` when that is given (None or empty: no restriction, as in rustfst-ffi)."""

    def __init__(self, sigma_label: int, rewrite_mode: MatcherRewriteMode = MatcherRewriteMode.AUTO,
                 sigma_allowed_matches: Optional[Sequence[int]] = None):
        if not isinstance(rewrite_mode, MatcherRewriteMode):
            raise TypeError("rewrite_mode must be a MatcherRewriteMode")
        self.sigma_label = int(sigma_label)
        self.rewrite_mode = rewrite_mode
        self.sigma_allowed_matches = [int(x) for x in sigma_allowed_matches] if sigma_allowed_matches is not None else []
        if not 0 <= self.sigma_label <= 0xFFFFFFFF or any(not 0 <= x <= 0xFFFFFFFF for x in self.sigma_allowed_matches):
            raise ValueError("labels are 32-bit unsigned")
        self._arr = (C.c_uint32 * len(self.sigma_allowed_matches))(*self.sigma_allowed_matches)

    def _c(self):
        n = len(self.sigma_allowed_matches)
        return C.pointer(_lib.MatcherConfig(self.sigma_label, self.rewrite_mode.value,
                                            C.cast(self._arr, C.POINTER(C.c_uint32)) if n else None, n))


class ComposeConfig:
    """rustfst-python/rustfst/algorithms/compose.py:65-113.  With a `matcher1_config` / `matcher2_config` (MatcherConfig: the
    sigma matcher of the left / right FST) the composition goes through wfst_compose_with_matchers; AUTOFILTER is then
    refused, as in the reference."""

    def __init__(self, compose_filter: ComposeFilter = ComposeFilter.AUTOFILTER, connect: bool = True,
                 matcher1_config: Optional[MatcherConfig] = None, matcher2_config: Optional[MatcherConfig] = None):
        for m in (matcher1_config, matcher2_config):
            if m is not None and not isinstance(m, MatcherConfig):
                raise TypeError("matcher configs must be MatcherConfig or None")
        self.compose_filter = compose_filter
        self.connect = bool(connect)
        self.matcher1_config = matcher1_config
        self.matcher2_config = matcher2_config

    def _c(self, matchers: bool = False):
        """wfst_compose_config; `matchers`: the caller passes the matcher configs on (DeviceFst.compose and compose_shortest_path_batch do)"""
        if not matchers and (self.matcher1_config is not None or self.matcher2_config is not None):
            raise WfstError("unsupported: a MatcherConfig (sigma matcher) outside compose / compose_with_config")
        return C.pointer(_lib.ComposeConfig(self.compose_filter.value, 1 if self.connect else 0))


class ShortestPathConfig:
    """rustfst-python/rustfst/algorithms/shortest_path.py:14-38."""

    def __init__(self, nshortest: int = 1, unique: bool = False, delta: Union[float, None] = None):
        self.nshortest = int(nshortest)
        self.unique = bool(unique)
        self.delta = KSHORTESTDELTA if delta is None else float(delta)

    def _c(self):
        return C.pointer(_lib.ShortestPathConfig(self.delta, self.nshortest, 1 if self.unique else 0))


class ClosureType(Enum):  # rustfst/src/algorithms/closure/mod.rs:9-12 (enum order = the C-ABI's closure_type)
    CLOSURE_STAR = 0
    CLOSURE_PLUS = 1


class ReweightType(Enum):  # rustfst/src/algorithms/reweight.rs:11-17 (enum order = the C-ABI's reweight_type)
    REWEIGHT_TO_INITIAL = 0
    REWEIGHT_TO_FINAL = 1


class PushWeightsConfig:
    """rustfst/src/algorithms/push.rs:34-68: PushWeightsConfig::default() = {KDELTA, remove_total_weight false}."""

    def __init__(self, delta: float = KDELTA, remove_total_weight: bool = False):
        self.delta = float(delta)
        self.remove_total_weight = bool(remove_total_weight)

    def _c(self):
        return C.pointer(_lib.PushWeightsConfig(self.delta, 1 if self.remove_total_weight else 0))


class DeterminizeType(Enum):  # rustfst-python/rustfst/algorithms/determinize.py:15-33 (the ffi numbering)
    DETERMINIZE_FUNCTIONAL = 0
    DETERMINIZE_NON_FUNCTIONAL = 1
    DETERMINIZE_DISAMBIGUATE = 2


class DeterminizeConfig:
    """rustfst-python determinize.py:36-58: DeterminizeConfig(det_type, delta=None); delta None = KDELTA."""

    def __init__(self, det_type: DeterminizeType, delta: Optional[float] = None):
        self.det_type = DeterminizeType(det_type)
        self.delta = KDELTA if delta is None else float(delta)

    def _c(self):
        return C.pointer(_lib.DeterminizeConfig(self.delta, self.det_type.value))


KSHORTESTDELTA = 1e-6  # rustfst/src/lib.rs


class MinimizeConfig:
    """rustfst-python algorithms/minimize.py: MinimizeConfig(delta=KSHORTESTDELTA, allow_nondet=False)."""

    def __init__(self, delta: Optional[float] = None, allow_nondet: bool = False):
        self.delta = KSHORTESTDELTA if delta is None else float(delta)
        self.allow_nondet = bool(allow_nondet)

    def _c(self):
        return C.pointer(_lib.MinimizeConfig(self.delta, 1 if self.allow_nondet else 0))


# ------------------------------------------------------------------ VectorFst mirror
class VectorFst:
    """Mutable FST stored in vectors (rustfst-python/rustfst/fst/vector_fst.py:29-790, subset on the path)."""

    def __init__(self, ptr=None, ctx: Optional[Context] = None):
        self._ctx = ctx
        self._dev: Optional[DeviceFst] = None
        if ptr is not None:
            self._p = ptr
        else:
            p = C.c_void_p()
            check(_lib.lib().wfst_vec_fst_new(C.byref(p)), "Something went wrong when creating the Fst struct")
            self._p = p

    def __del__(self):
        p = getattr(self, "_p", None)
        if p:
            try:
                _lib.lib().wfst_vec_fst_destroy(p)
            except Exception:
                pass
            self._p = None

    # -- mutation
    def add_state(self) -> int:
        s = C.c_uint32()
        check(_lib.lib().wfst_vec_fst_add_state(self._p, C.byref(s)), "Error during `add_state`")
        self._dev = None
        return s.value

    def add_tr(self, state: int, tr: Tr) -> "VectorFst":
        arr = np.array([(tr.ilabel, tr.olabel, tr.weight, tr.next_state)], dtype=TR_DTYPE)
        check(_lib.lib().wfst_vec_fst_add_tr(self._p, state, arr.ctypes.data), "Error during `add_tr`")
        self._dev = None
        return self

    def set_start(self, state: int):
        check(_lib.lib().wfst_vec_fst_set_start(self._p, state), "Error setting start state")
        self._dev = None

    def set_final(self, state: int, weight: Union[float, None] = None):
        check(_lib.lib().wfst_vec_fst_set_final(self._p, state, 0.0 if weight is None else weight),
              "Error setting final state")
        self._dev = None

    def unset_final(self, state: int):
        check(_lib.lib().wfst_vec_fst_del_final_weight(self._p, state), "Error unsetting final state")
        self._dev = None

    def tr_sort(self, ilabel_cmp: bool = True) -> "VectorFst":
        check(_lib.lib().wfst_vec_fst_tr_sort(self._p, 1 if ilabel_cmp else 0), "Error during tr_sort")
        self._dev = None
        return self

    # -- inspection
    def num_states(self) -> int:
        n = C.c_uint32()
        check(_lib.lib().wfst_vec_fst_num_states(self._p, C.byref(n)), "Error getting number of states")
        return n.value

    def start(self) -> Optional[int]:
        s = C.c_int64()
        check(_lib.lib().wfst_vec_fst_start(self._p, C.byref(s)), "Error getting start state")
        return None if s.value < 0 else s.value

    def final_weight(self, state: int) -> Optional[float]:
        w = C.c_float()
        some = C.c_int()
        check(_lib.lib().wfst_vec_fst_final_weight(self._p, state, C.byref(w), C.byref(some)),
              "Error getting final weight")
        return w.value if some.value else None

    def is_final(self, state: int) -> bool:
        return self.final_weight(state) is not None

    def num_trs(self, state: int) -> int:
        n = C.c_uint64()
        check(_lib.lib().wfst_vec_fst_num_trs(self._p, state, C.byref(n)), "Error getting number of trs")
        return n.value

    def trs(self, state: int) -> List[Tr]:
        n = self.num_trs(state)
        arr = np.zeros(n, dtype=TR_DTYPE)
        got = C.c_uint64()
        check(_lib.lib().wfst_vec_fst_get_trs(self._p, state, arr.ctypes.data, n, C.byref(got)), "Error getting trs")
        return [Tr(int(a["ilabel"]), int(a["olabel"]), float(a["weight"]), int(a["nextstate"])) for a in arr]

    def properties(self) -> int:
        p = C.c_uint64()
        check(_lib.lib().wfst_vec_fst_properties(self._p, C.byref(p)))
        return p.value

    def equals(self, other: "VectorFst") -> bool:
        eq = C.c_int()
        check(_lib.lib().wfst_vec_fst_equals(self._p, other._p, C.byref(eq)), "Error checking equality")
        return bool(eq.value)

    def __eq__(self, other):
        return self.equals(other)

    def copy(self) -> "VectorFst":
        p = C.c_void_p()
        check(_lib.lib().wfst_vec_fst_copy(self._p, C.byref(p)), "Error copying fst")
        return VectorFst(ptr=p, ctx=self._ctx)

    def __str__(self):
        lines = []
        for s in range(self.num_states()):
            for t in self.trs(s):
                lines.append(f"{s}\t{t.next_state}\t{t.ilabel}\t{t.olabel}\t{t.weight}")
            fw = self.final_weight(s)
            if fw is not None:
                lines.append(f"{s}\t{fw}")
        return "\n".join(lines)

    # -- device residency
    def to_device(self, ctx: Optional[Context] = None) -> DeviceFst:
        ctx = ctx or self._ctx or default_context()
        if self._dev is None or self._dev.ctx is not ctx:
            h = C.c_void_p()
            check(_lib.lib().wfst_vec_fst_to_device(ctx._h, self._p, C.byref(h)), "wfst_vec_fst_to_device")
            self._dev = DeviceFst(h, ctx)
        return self._dev

    # -- I/O (rustfst-python vector_fst.py:311-388)
    @classmethod
    def from_bytes(cls, data: bytes, ctx: Optional[Context] = None) -> "VectorFst":
        return DeviceFst.from_bytes(data, ctx).to_vector_fst()

    def to_bytes(self) -> bytes:
        return self.to_device().to_bytes()

    @classmethod
    def read(cls, filename) -> "VectorFst":
        with open(filename, "rb") as f:
            return cls.from_bytes(f.read())

    def write(self, filename):
        with open(filename, "wb") as f:
            f.write(self.to_bytes())

    # -- algorithms (vector_fst.py:419-436, 621-638)
    def compose(self, other: "VectorFst", config: Union[ComposeConfig, None] = None) -> "VectorFst":
        return self.to_device().compose(other.to_device(self.to_device().ctx), config).to_vector_fst()

    def shortest_path(self, config: Union[ShortestPathConfig, None] = None) -> "VectorFst":
        return self.to_device().shortest_path(config).to_vector_fst()

    def rm_epsilon(self) -> "VectorFst":
        """rustfst-python vector_fst.py `rm_epsilon` (algorithms/rm_epsilon.py): in place, returns this FST."""
        res = self.to_device().rm_epsilon().to_vector_fst()
        self._p, res._p = res._p, self._p
        self._dev = None
        return self

    def top_sort(self) -> "VectorFst":
        """rustfst-python vector_fst.py `top_sort` (algorithms/top_sort.py): in place, returns this FST."""
        res = self.to_device().top_sort().to_vector_fst()
        self._p, res._p = res._p, self._p
        self._dev = None
        return self

    def state_sort(self, order) -> "VectorFst":
        """algorithms::state_sort (state_sort.rs:16-78): in place, returns this FST."""
        res = self.to_device().state_sort(order).to_vector_fst()
        self._p, res._p = res._p, self._p
        self._dev = None
        return self

    def connect(self) -> "VectorFst":
        """rustfst-python vector_fst.py `connect` (algorithms/connect.py): trims this FST in place and returns it."""
        trimmed = self.to_device().connect().to_vector_fst()
        self._p, trimmed._p = trimmed._p, self._p  # this object now owns the trimmed FST; the old one dies with `trimmed`
        self._dev = None
        return self

    def push_weights(self, reweight_type: "ReweightType", config: Optional[PushWeightsConfig] = None) -> "VectorFst":
        """push_weights_with_config (push.rs:89-118) in place on the device copy; returns this FST."""
        res = self.to_device().push_weights(reweight_type, config).to_vector_fst()
        self._p, res._p = res._p, self._p
        self._dev = None
        return self

    def reweight(self, potentials, reweight_type: "ReweightType") -> "VectorFst":
        """reweight (reweight.rs:29-154) in place on the device copy; returns this FST."""
        res = self.to_device().reweight(potentials, reweight_type).to_vector_fst()
        self._p, res._p = res._p, self._p
        self._dev = None
        return self

    def determinize(self, config: Optional[DeterminizeConfig] = None) -> "VectorFst":
        """rustfst-python vector_fst.py `determinize`: a NEW VectorFst (this one is left as it is)."""
        return self.to_device().determinize(config).to_vector_fst()

    def minimize(self, config: Optional[MinimizeConfig] = None) -> "VectorFst":
        """rustfst-python vector_fst.py `minimize`: minimizes THIS FST in place on the device copy; returns this FST."""
        res = self.to_device().minimize(config).to_vector_fst()
        self._p, res._p = res._p, self._p
        self._dev = None
        return self

    def tr_sum(self) -> "VectorFst":
        """algorithms::tr_sum (tr_sum.rs:7-22): in place on the device copy; returns this FST."""
        res = self.to_device().tr_sum().to_vector_fst()
        self._p, res._p = res._p, self._p
        self._dev = None
        return self

    def tr_unique(self) -> "VectorFst":
        """rustfst-python vector_fst.py `tr_unique`: keeps a single instance of equal arcs, in place; returns this FST."""
        res = self.to_device().tr_unique().to_vector_fst()
        self._p, res._p = res._p, self._p
        self._dev = None
        return self

    def optimize(self) -> "VectorFst":
        """rustfst-python vector_fst.py `optimize`: determinization and minimization of THIS FST in place on the device
        copy (acyclic inputs); returns this FST."""
        res = self.to_device().optimize().to_vector_fst()
        self._p, res._p = res._p, self._p
        self._dev = None
        return self

    def union(self, other_fst: "VectorFst") -> "VectorFst":
        """rustfst-python vector_fst.py:640 `union` (algorithms/union.py:13-44): THIS FST becomes the union, in place on the
        device copies; returns this FST.  `other_fst` is left as it is."""
        ctx = self.to_device().ctx
        res = self.to_device().union(other_fst.to_device(ctx)).to_vector_fst()
        self._p, res._p = res._p, self._p
        self._dev = None
        return self

    def concat(self, other: "VectorFst") -> "VectorFst":
        """rustfst-python vector_fst.py:438 `concat` (algorithms/concat.py): THIS FST becomes the concatenation, in place on
        the device copies; returns this FST."""
        ctx = self.to_device().ctx
        res = self.to_device().concat(other.to_device(ctx)).to_vector_fst()
        self._p, res._p = res._p, self._p
        self._dev = None
        return self

    def closure(self, closure_type: "ClosureType") -> "VectorFst":
        """algorithms::closure (closure/closure_static.rs:25-73; not in rustfst-python): in place on the device copy;
        returns this FST."""
        res = self.to_device().closure(closure_type).to_vector_fst()
        self._p, res._p = res._p, self._p
        self._dev = None
        return self

    def project(self, proj_type: Union["ProjectType", None] = None) -> "VectorFst":
        """rustfst-python vector_fst.py:525-538 `project` (algorithms/project.py:27-50): projects THIS FST in place and
        returns it (the reference returns self).  The device copy is projected and becomes this object's host data; the
        cached device handle is dropped so that trs(), equality and later compose / shortest_path calls all see the
        projected labels."""
        projected = self.to_device().project(proj_type).to_vector_fst()
        self._p, projected._p = projected._p, self._p
        self._dev = None
        return self

    def invert(self) -> "VectorFst":
        """rustfst-python vector_fst.py:730-740 `invert` (algorithms/inversion.py): inverts THIS FST in place and returns
        it; the device copy is inverted and becomes this object's host data, like project."""
        inverted = self.to_device().invert().to_vector_fst()
        self._p, inverted._p = inverted._p, self._p
        self._dev = None
        return self

    def isomorphic(self, other: "VectorFst") -> bool:
        """rustfst-python vector_fst.py:718-728 `isomorphic` (algorithms/isomorphic.py): both FSTs are uploaded and compared
        on the device."""
        dev = self.to_device()
        return dev.isomorphic(other.to_device(dev.ctx))

    def paths_iter(self, max_paths: int = 1 << 20) -> "PathTable":
        """Fst::paths_iter (fst_traits/paths_iterator.rs:24-62): the FST is uploaded and enumerated on the device; the
        table iterates as FstPath in the reference's order."""
        return self.to_device().paths(max_paths)


# ------------------------------------------------------------------ free functions
def compose(fst: VectorFst, fst2: VectorFst) -> VectorFst:
    """rustfst-python/rustfst/algorithms/compose.py `compose`."""
    return fst.compose(fst2)


def compose_with_config(fst: VectorFst, fst2: VectorFst, config: ComposeConfig) -> VectorFst:
    return fst.compose(fst2, config)


def project(fst: VectorFst, proj_type: ProjectType = ProjectType.PROJECT_INPUT) -> VectorFst:
    """rustfst-python/rustfst/algorithms/project.py:27-50."""
    return fst.project(proj_type)


def invert(fst: Union[VectorFst, DeviceFst]) -> Union[VectorFst, DeviceFst]:
    """rustfst-python/rustfst/algorithms/inversion.py `invert`: in place, returns fst."""
    return fst.invert()


def isomorphic(fst: Union[VectorFst, DeviceFst], other_fst: Union[VectorFst, DeviceFst]) -> bool:
    """rustfst-python/rustfst/algorithms/isomorphic.py `isomorphic`."""
    return fst.isomorphic(other_fst)


def shortestpath(fst: VectorFst) -> VectorFst:
    """rustfst-python/rustfst/algorithms/shortest_path.py:41-56."""
    return fst.shortest_path()


def shortestpath_with_config(fst: VectorFst, config: ShortestPathConfig) -> VectorFst:
    return fst.shortest_path(config)


def acceptor(labels: Sequence[int], weight: float = 0.0) -> VectorFst:
    """utils::acceptor (rustfst/src/utils/labels_to_fst.rs:111-132): L+1 states, unit arc weights,
    last state final with `weight`."""
    fst = VectorFst()
    cur = fst.add_state()
    fst.set_start(cur)
    for l in labels:
        nxt = fst.add_state()
        fst.add_tr(cur, Tr(l, l, 0.0, nxt))
        cur = nxt
    fst.set_final(cur, weight)
    return fst


def shortest_distance(fst: Union[VectorFst, DeviceFst], reverse: bool = False) -> np.ndarray:
    """algorithms::shortest_distance(fst, reverse) (shortest_distance.rs:307-311): the reference's Vec (its length
    included)."""
    dev = fst.to_device() if isinstance(fst, VectorFst) else fst
    dist, n = dev.shortest_distance_with_len(reverse=reverse)
    return dist[:n]


def reweight(fst: VectorFst, potentials, reweight_type: ReweightType) -> VectorFst:
    """algorithms::reweight (reweight.rs:29-154): in place, returns fst."""
    return fst.reweight(potentials, reweight_type)


def push_weights(fst: VectorFst, reweight_type: ReweightType) -> VectorFst:
    """algorithms::push_weights (push.rs:76-82): in place, returns fst."""
    return fst.push_weights(reweight_type)


def push_weights_with_config(fst: VectorFst, reweight_type: ReweightType, config: PushWeightsConfig) -> VectorFst:
    """algorithms::push_weights_with_config (push.rs:89-118): in place, returns fst."""
    return fst.push_weights(reweight_type, config)


def determinize(fst: VectorFst) -> VectorFst:
    """algorithms::determinize (determinize_static.rs:149-156): a new FST (acceptors only)."""
    return fst.determinize()


def determinize_with_config(fst: VectorFst, config: DeterminizeConfig) -> VectorFst:
    """algorithms::determinize_with_config (determinize_static.rs:176-190): a new FST (acceptors only)."""
    return fst.determinize(config)


def minimize(fst: VectorFst) -> VectorFst:
    """algorithms::minimize (minimize.rs:77-87): in place, returns fst (deterministic acyclic acceptors only)."""
    return fst.minimize()


def tr_sum(fst: VectorFst) -> VectorFst:
    """algorithms::tr_sum (tr_sum.rs:7-22): in place, returns fst."""
    return fst.tr_sum()


def tr_unique(fst: VectorFst) -> VectorFst:
    """algorithms::tr_unique (tr_unique.rs:38-51): in place, returns fst."""
    return fst.tr_unique()


def optimize(fst: VectorFst) -> VectorFst:
    """algorithms::optimize (optimize.rs:11-128): in place, returns fst (acyclic inputs only)."""
    return fst.optimize()


def top_sort(fst: VectorFst) -> VectorFst:
    """rustfst-python/rustfst/algorithms/top_sort.py `top_sort`: in place, returns fst."""
    return fst.top_sort()


def state_sort(fst: VectorFst, order) -> VectorFst:
    """algorithms::state_sort (state_sort.rs:16-78): in place, returns fst."""
    return fst.state_sort(order)


def minimize_with_config(fst: VectorFst, config: MinimizeConfig) -> VectorFst:
    """algorithms::minimize_with_config (minimize.rs:92-176): in place, returns fst."""
    return fst.minimize(config)


def union(fst: Union[VectorFst, DeviceFst], other_fst: Union[VectorFst, DeviceFst]) -> Union[VectorFst, DeviceFst]:
    """rustfst-python/rustfst/algorithms/union.py `union`: a VectorFst is changed in place and returned; DeviceFsts give a
    NEW DeviceFst."""
    return fst.union(other_fst)


def concat(fst: Union[VectorFst, DeviceFst], other_fst: Union[VectorFst, DeviceFst]) -> Union[VectorFst, DeviceFst]:
    """rustfst-python/rustfst/algorithms/concat.py `concat`."""
    return fst.concat(other_fst)


def closure(fst: Union[VectorFst, DeviceFst], closure_type: ClosureType) -> Union[VectorFst, DeviceFst]:
    """rustfst::algorithms::closure::closure (closure/closure_static.rs:25-73)."""
    return fst.closure(closure_type)


def _list_form(fsts, device_call):
    if len(fsts) == 0:
        raise ValueError("fsts must be at least of len 1")  # rustfst-python/rustfst/algorithms/union.py:58-59
    if isinstance(fsts, HandleArray) or isinstance(fsts[0], DeviceFst):
        return device_call(fsts)
    ctx = fsts[0].to_device().ctx
    return device_call([f.to_device(ctx) for f in fsts]).to_vector_fst()


def union_list(fsts: Sequence[Union[VectorFst, DeviceFst]]) -> Union[VectorFst, DeviceFst]:
    """rustfst-python/rustfst/algorithms/union.py:47-64 `union_list`: the left fold of union over copies of `fsts`, as ONE
    device call (wfst_union_list).  A NEW FST of the items' kind; the items are left as they are."""
    return _list_form(fsts, _device_union_list)


def concat_list(fsts: Sequence[Union[VectorFst, DeviceFst]]) -> Union[VectorFst, DeviceFst]:
    """rustfst-python/rustfst/algorithms/concat.py `concat_list`: the left fold of concat, as ONE device call
    (wfst_concat_list).  A NEW FST of the items' kind."""
    return _list_form(fsts, _device_concat_list)


def replace(root_idx: int, fst_list: Sequence[Tuple[int, Union[VectorFst, DeviceFst]]],
            epsilon_on_replace: bool) -> Union[VectorFst, DeviceFst]:
    """rustfst-python/rustfst/algorithms/replace.py:19-80 `replace`: the recursive transition network over the (label, fst)
    pairs of `fst_list`, expanded from the FST whose label is `root_idx`, as ONE device call (wfst_replace).  A NEW FST of the
    items' kind; the items are left as they are.  A grammar whose expansion reaches a recursive call raises (the reference
    does not terminate on it)."""
    fst_list = list(fst_list)
    if len(fst_list) == 0 or isinstance(fst_list[0][1], DeviceFst):
        return _device_replace(root_idx, fst_list, epsilon_on_replace)
    ctx = fst_list[0][1].to_device().ctx
    return _device_replace(root_idx, [(label, f.to_device(ctx)) for label, f in fst_list], epsilon_on_replace, ctx).to_vector_fst()
