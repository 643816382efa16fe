// rm_epsilon_batch.hip — wfst_rm_epsilon_batch: rm_epsilon of many small FSTs, one workgroup per FST.
//
// The single call (rm_epsilon.hip) is built for one large machine: it downloads the FST, schedules the rewrites on the host
// (Tarjan), launches once per epsilon depth with two synchronisations each, and then runs connect with several more.  A
// lattice of a few hundred states pays dozens of host round trips for microseconds of device work.  Here ONE workgroup runs
// every stage of rm_epsilon_fst on its item, inside the item's slice of one slab, as workgroup-local passes separated by
// barriers; the number of launches depends neither on the number of items nor on any item's epsilon depth:
//   noneps_in   the start state and the target of every arc that is not epsilon:epsilon (rm_epsilon_static.rs:64-75)
//   depth       sinks of the epsilon graph are peeled level by level over its transpose; the level a state leaves in is its
//               epsilon depth (longest epsilon path to a state without epsilon arcs); states never peeled lie on or before
//               an epsilon cycle, whose order of rewrites the host schedules -> exit "single path"
//   rewrite     depth by depth, a barrier between depths, one thread per state with noneps_in: rm_expand_state (rm_expand.h,
//               the single path's own function) at the last rung of the one-thread kernel (64 closure states, 128 stack
//               entries, 128 arcs) in one of min(n, workgroup size) scratch slices, then the finished arcs are copied into
//               the item's arc arena through a workgroup-wide cursor and published (RmView) to the deeper depths.  A state
//               beyond the rung -> exit "single path" (the wave kernel's business).  Only the arena can overflow -> exit
//               "grow" with the arcs needed so far; the host runs the item again in the next launch with at least twice the
//               arena.
//   csr         states without noneps_in lose their arcs; offsets by a workgroup scan, the arcs into CSR order, and the three
//               facts of rm_write in the same pass
//   connect     forward search from the start, transpose, backward search from the final states, stable renumbering of the
//               survivors, arcs into removed states dropped (connect_and_adopt's result, compose_wide.hip)
// The property word is the host's: rm_epsilon_word(stored word, facts), the single call's own function.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "batch_driver.h"
#include "common.h"
#include "rm_expand.h"
#include "wg_ops.h"

namespace wfst {

namespace {

constexpr uint32_t RB_MAX_STATES = 4096;  // the in_kernel rule (include/wfst.h)
constexpr uint32_t RB_MAX_ARCS = 16384;
constexpr RmCaps RB_CAPS{64, 128, 128};   // ... and its third condition: the last rung of rm_epsilon_fst's one-thread kernel
constexpr size_t RB_MAX_SLAB = (size_t)8 << 30;  // all slices of one launch together; beyond: KO before that launch
// exit codes of an item (RbCtl::exit)
enum : uint32_t { RB_RUNNING = 0, RB_DONE = 1, RB_EMPTY = 2, RB_GROW = 3, RB_SINGLE_CYCLE = 4, RB_SINGLE_CAPS = 5 };

struct RbCtl {  // one per item, at the head of the slab; read back once per launch
  uint32_t exit;
  uint32_t facts;      // rm_write's: 1 some new arc has ilabel != olabel | 2 nextstate <= its state | 4 an arc was added
  uint32_t need_arcs;  // RB_GROW: arena arcs asked for when the item gave up (a lower bound of what it needs)
  uint32_t n_out, e_out, start_out;
  uint32_t pad[2];
};
struct RbItem {
  const uint32_t* off;
  const wfst_tr* arcs;
  const float* fin_in;
  uint32_t n, start;
  uint32_t cap;        // arcs of the arena (and of pre / the result)
  uint32_t n_slices;   // scratch slices of rm_slice_bytes(RB_CAPS): min(n, MB_TPB)
  RbCtl* ctl;
  // the slice; R = max(E, cap) bounds the arcs of both transposes
  uint32_t* noneps;            // [n]
  uint32_t* edeg;              // [n] epsilon arcs into states not yet peeled
  uint32_t *roff, *rcnt;       // [n + 1] the transpose of the epsilon graph, then of the result before connect
  uint32_t* rsrc;              // [R]
  uint32_t* order;             // [n] states in peeling order, level after level; then the queue of the searches
  uint32_t* lend;              // [n] end of level d in order
  uint32_t* done;              // [n] RmView: rewritten ..
  uint32_t* cnt;               // [n + 1] .. its new arc count (0: not rewritten) ..
  unsigned long long* arc_ptr; // [n] .. and where its new arcs are
  float* fin;                  // [n] final weights as the rewrites leave them
  char* scratch;               // [n_slices] closure / stack / arc list of the state a thread is rewriting
  wfst_tr* arena;              // [cap] finished arcs in order of completion; then the result's arcs
  uint32_t* off1;              // [n + 1] the result before connect ..
  wfst_tr* pre;                // [cap]
  uint32_t *acc, *co;          // [n + 1] reached from the start / reaches a final state
  uint32_t *keep, *new_id;     // [n + 1]
  uint32_t* cnt2;              // [n + 1]
  uint32_t* off_out;           // [n + 1] the result
  float* fin_out;              // [n]
};

__global__ void __launch_bounds__(MB_TPB) rm_epsilon_batch_kernel(const RbItem* __restrict__ items) {
  __shared__ uint32_t part[MB_TPB + 1];
  __shared__ uint32_t sh[3];  // wg_search
  __shared__ uint32_t s_tail, s_fail, s_cursor, s_facts;
  const RbItem it = items[blockIdx.x];
  const uint32_t tid = threadIdx.x, lane = tid & 15u;
  const uint32_t n = it.n;
  RbCtl* ctl = it.ctl;
  auto leave = [&](uint32_t code) {
    if (tid == 0) ctl->exit = code;
  };
  // ---- 1. noneps_in, the epsilon out-degrees and the in-degrees of the epsilon graph
  if (tid == 0) s_tail = s_fail = s_cursor = s_facts = 0;
  wg_fill(it.noneps, n, 0u);
  wg_fill(it.rcnt, n + 1, 0u);
  wg_fill(it.done, n, 0u);
  wg_fill(it.cnt, n + 1, 0u);
  for (uint32_t s = tid; s < n; s += MB_TPB) it.fin[s] = it.fin_in[s];
  wg_bar();
  for (uint32_t s = tid >> 4; s < n; s += MB_TPB >> 4) {
    uint32_t e = 0;
    for (uint32_t i = it.off[s] + lane; i < it.off[s + 1]; i += 16) {
      const wfst_tr tr = it.arcs[i];
      if (is_eps(tr)) {
        ++e;
        atomicAdd(&it.rcnt[tr.nextstate], 1u);
      } else {
        it.noneps[tr.nextstate] = 1u;
      }
    }
    for (int d = 8; d >= 1; d >>= 1) e += __shfl_xor(e, d, 16);
    if (lane == 0) it.edeg[s] = e;
  }
  if (tid == 0) it.noneps[it.start] = 1u;
  wg_bar();
  // ---- 2. the transpose of the epsilon graph; epsilon depth by peeling its sinks
  wg_exclusive_scan(it.rcnt, it.roff, n + 1, part);
  wg_fill(it.rcnt, n + 1, 0u);
  wg_bar();
  for (uint32_t s = tid >> 4; s < n; s += MB_TPB >> 4)
    for (uint32_t i = it.off[s] + lane; i < it.off[s + 1]; i += 16) {
      const wfst_tr tr = it.arcs[i];
      if (is_eps(tr)) it.rsrc[it.roff[tr.nextstate] + atomicAdd(&it.rcnt[tr.nextstate], 1u)] = s;
    }
  for (uint32_t s = tid; s < n; s += MB_TPB)
    if (it.edeg[s] == 0u) stg(&it.order[atomicAdd(&s_tail, 1u)], s);
  wg_bar();
  uint32_t lo = 0, n_levels = 0;
  for (;;) {
    const uint32_t hi = s_tail;
    __syncthreads();  // (everybody has read the tail before anybody moves it)
    if (hi == lo) break;
    if (tid == 0) stg(&it.lend[n_levels], hi);
    ++n_levels;
    for (uint32_t k = lo + (tid >> 4); k < hi; k += MB_TPB >> 4) {
      const uint32_t s = ld(&it.order[k]);
      for (uint32_t i = it.roff[s] + lane; i < it.roff[s + 1]; i += 16) {
        const uint32_t p = it.rsrc[i];
        if (atomicSub(&it.edeg[p], 1u) == 1u) stg(&it.order[atomicAdd(&s_tail, 1u)], p);
      }
    }
    wg_bar();
    lo = hi;
  }
  if (lo != n) return leave(RB_SINGLE_CYCLE);  // states left over: an epsilon cycle (a self loop is one)

  // ---- 3. the rewrites, depth by depth: states of one depth do not read each other; a deeper state sees the rewritten
  // ones through their new arcs (RmView::trs)
  const RmView view{it.off, it.arcs, it.done, it.cnt, it.arc_ptr};
  lo = 0;
  for (uint32_t d = 0; d < n_levels; ++d) {
    const uint32_t hi = ld(&it.lend[d]);
    if (tid < it.n_slices) {
      char* slice = it.scratch + (size_t)tid * rm_slice_bytes(RB_CAPS);
      for (uint32_t k = lo + tid; k < hi; k += it.n_slices) {
        const uint32_t s = ld(&it.order[k]);
        if (!it.noneps[s]) continue;
        uint32_t na;
        float final_w;
        if (!rm_expand_state(view, s, RB_CAPS, slice, it.fin, &na, &final_w)) {
          s_fail = 1u;
          break;
        }
        const uint32_t at = atomicAdd(&s_cursor, na);
        if (at + na > it.cap) continue;  // (the cursor keeps what was asked for)
        const wfst_tr* src = (const wfst_tr*)(slice + rm_arcs_offset(RB_CAPS));
        wfst_tr* dst = it.arena + at;
        for (uint32_t a = 0; a < na; ++a) dst[a] = src[a];
        it.arc_ptr[s] = (unsigned long long)dst;
        it.cnt[s] = na;
        it.fin[s] = final_w;
        it.done[s] = 1u;
      }
    }
    wg_bar();
    const uint32_t fail = s_fail, asked = s_cursor;
    __syncthreads();  // (read by everybody before the next depth writes them)
    if (fail) return leave(RB_SINGLE_CAPS);
    if (asked > it.cap) {
      if (tid == 0) ctl->need_arcs = asked;
      return leave(RB_GROW);
    }
    lo = hi;
  }

  // ---- 4. the CSR of the result before connect (states that were not rewritten have cnt 0) and rm_write's facts
  const uint32_t e1 = wg_exclusive_scan(it.cnt, it.off1, n + 1, part);
  {
    uint32_t f = 0;
    for (uint32_t s = tid >> 4; s < n; s += MB_TPB >> 4) {
      const uint32_t na = it.cnt[s];
      if (!na) continue;
      const wfst_tr* src = (const wfst_tr*)it.arc_ptr[s];
      const uint32_t o = it.off1[s];
      for (uint32_t k = lane; k < na; k += 16) {
        const wfst_tr tr = src[k];
        it.pre[o + k] = tr;
        f |= 4u | (tr.ilabel != tr.olabel ? 1u : 0u) | (tr.nextstate <= s ? 2u : 0u);
      }
    }
    if (f) atomicOr(&s_facts, f);
  }
  // ---- 5. connect: reached from the start and reaching a final state
  wg_fill(it.acc, n + 1, 0u);
  wg_fill(it.co, n + 1, 0u);
  if (tid == 0) sh[2] = 0;
  wg_bar();
  if (tid == 0) {
    ctl->facts = s_facts;
    it.acc[it.start] = 1u;
    it.order[0] = it.start;
    sh[2] = 1;
  }
  wg_bar();
  wg_search(it.off1, it.pre, nullptr, it.acc, it.order, sh);
  wg_transpose(it.off1, it.pre, n, e1, it.roff, it.rcnt, it.rsrc, part);
  if (tid == 0) sh[2] = 0;
  wg_bar();
  for (uint32_t s = tid; s < n; s += MB_TPB)
    if (it.fin[s] != INF) {
      it.co[s] = 1u;
      it.order[atomicAdd(&sh[2], 1u)] = s;
    }
  wg_bar();
  wg_search(it.roff, nullptr, it.rsrc, it.co, it.order, sh);
  for (uint32_t s = tid; s <= n; s += MB_TPB) it.keep[s] = s < n ? (ld(&it.acc[s]) & ld(&it.co[s])) : 0u;
  wg_bar();
  // stable renumbering of the survivors (del_states, mutable_fst.rs:132-158).  The start state survives iff it reaches a
  // final state; if it does not, nothing accessible does: everything goes
  const uint32_t tn = wg_exclusive_scan(it.keep, it.new_id, n + 1, part);
  if (tn == 0) return leave(RB_EMPTY);
  wg_fill(it.cnt2, tn + 1, 0u);
  wg_bar();
  for (uint32_t s = tid >> 4; s < n; s += MB_TPB >> 4) {
    if (!it.keep[s]) continue;  // (uniform over the 16 lanes)
    uint32_t k = 0;
    for (uint32_t i = it.off1[s] + lane; i < it.off1[s + 1]; i += 16) k += it.keep[it.pre[i].nextstate];
    for (int d = 8; d >= 1; d >>= 1) k += __shfl_xor(k, d, 16);
    if (lane == 0) {
      const uint32_t ns = it.new_id[s];
      it.cnt2[ns] = k;
      it.fin_out[ns] = it.fin[s];
    }
  }
  wg_bar();
  const uint32_t e_out = wg_exclusive_scan(it.cnt2, it.off_out, tn + 1, part);
  wfst_tr* arcs_out = it.arena;  // (its arcs are in `pre` now)
  for (uint32_t s = tid; s < n; s += MB_TPB) {
    if (!it.keep[s]) continue;
    uint32_t w = it.off_out[it.new_id[s]];
    for (uint32_t i = it.off1[s]; i < it.off1[s + 1]; ++i) {  // (in order: arcs into deleted states drop out)
      const wfst_tr a = it.pre[i];
      if (it.keep[a.nextstate]) arcs_out[w++] = wfst_tr{a.ilabel, a.olabel, a.weight, it.new_id[a.nextstate]};
    }
  }
  if (tid == 0) {
    ctl->n_out = tn;
    ctl->e_out = e_out;
    ctl->start_out = it.new_id[it.start];
    ctl->exit = RB_DONE;
  }
}

// carves one item's arrays out of the slab, every array 64-byte aligned; it == nullptr only measures
size_t carve_rm_slice(Slab s, uint32_t n, uint32_t E, uint32_t cap, RbItem* it) {
  const size_t N = n, N1 = (size_t)n + 1, R = std::max(E, cap);
  const uint32_t n_slices = std::min(n, MB_TPB);
  RbItem v{};
  v.noneps = s.take<uint32_t>(N);
  v.edeg = s.take<uint32_t>(N);
  v.roff = s.take<uint32_t>(N1);
  v.rcnt = s.take<uint32_t>(N1);
  v.rsrc = s.take<uint32_t>(R);
  v.order = s.take<uint32_t>(N);
  v.lend = s.take<uint32_t>(N);
  v.done = s.take<uint32_t>(N);
  v.cnt = s.take<uint32_t>(N1);
  v.arc_ptr = s.take<unsigned long long>(N);
  v.fin = s.take<float>(N);
  v.scratch = s.take<char>(rm_slice_bytes(RB_CAPS) * n_slices);
  v.arena = s.take<wfst_tr>(cap);
  v.off1 = s.take<uint32_t>(N1);
  v.pre = s.take<wfst_tr>(cap);
  v.acc = s.take<uint32_t>(N1);
  v.co = s.take<uint32_t>(N1);
  v.keep = s.take<uint32_t>(N1);
  v.new_id = s.take<uint32_t>(N1);
  v.cnt2 = s.take<uint32_t>(N1);
  v.off_out = s.take<uint32_t>(N1);
  v.fin_out = s.take<float>(N);
  v.n = n;
  v.cap = cap;
  v.n_slices = n_slices;
  if (it) *it = v;  // (the input's side is the caller's)
  return s.at();
}

}  // namespace

// the host loop is batch_driver.h's, with the ownership check, the grow loop and a slab limit per launch
void rm_epsilon_batch(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, wfst_fst** outs, uint8_t* in_kernel) {
  ctx->rm_batch = {};
  check_items_owned(ctx, fsts, n, "rm_epsilon_batch");
  const bool min_arena = arena_min_knob("WFST_RM_EPSILON_BATCH_ARENA");
  hipStream_t st = ctx->stream;
  enum : uint8_t { OPEN, DONE, EMPTY, SINGLE, TRIVIAL };
  struct Result {
    uint32_t facts = 0, n_out = 0, e_out = 0, start_out = 0;
    const uint32_t* off = nullptr;
    const wfst_tr* arcs = nullptr;
    const float* fin = nullptr;
  };
  std::vector<uint8_t> state(n, OPEN);
  std::vector<uint32_t> cap(n, 0);
  std::vector<Result> res(n);
  std::vector<size_t> open;
  for (size_t i = 0; i < n; ++i) {
    const wfst_fst* f = fsts[i];
    ensure_device(const_cast<wfst_fst*>(f));
    if (f->start < 0 || f->n_states == 0) {  // returned as it is (rm_epsilon_static.rs:58-61): never occupies a workgroup
      state[i] = TRIVIAL;
    } else if (f->n_states > RB_MAX_STATES || f->n_arcs > RB_MAX_ARCS) {
      state[i] = SINGLE;
    } else {
      // from the input's sizes alone (no device read): a result before connect of up to twice the input's arcs fits
      cap[i] = min_arena ? 1u : 2u * (uint32_t)f->n_arcs + 64u;
      open.push_back(i);
    }
  }
  auto carve = [&](size_t i, Slab s, RbItem* it) {
    const wfst_fst* f = fsts[i];
    const size_t end = carve_rm_slice(s, f->n_states, (uint32_t)f->n_arcs, cap[i], it);
    if (it) {
      it->off = f->dev.offsets;
      it->arcs = f->dev.arcs;
      it->fin_in = f->dev.finals;
      it->start = (uint32_t)f->start;
    }
    return end;
  };
  auto launch = [&](const RbItem* d_items, uint32_t m) { rm_epsilon_batch_kernel<<<m, MB_TPB, 0, st>>>(d_items); };
  auto classify = [&](size_t i, const RbCtl& c, const RbItem& it) {
    if (c.exit == RB_DONE) {
      state[i] = DONE;
      res[i] = Result{c.facts, c.n_out, c.e_out, c.start_out, it.off_out, it.arena, it.fin_out};
    } else if (c.exit == RB_EMPTY) {
      state[i] = EMPTY;
      res[i].facts = c.facts;
    } else if (c.exit == RB_SINGLE_CYCLE || c.exit == RB_SINGLE_CAPS) {
      state[i] = SINGLE;
      return BatchExit::SINGLE;
    } else if (c.exit == RB_GROW) {
      if (c.need_arcs <= cap[i]) return BatchExit::STUCK;
      cap[i] = (uint32_t)std::max<uint64_t>(2ull * cap[i], c.need_arcs);
      return BatchExit::GREW;
    } else {
      throw Error("rm_epsilon_batch: the kernel left item " + std::to_string(i) + " with exit code " + std::to_string(c.exit));
    }
    return BatchExit::FINISHED;
  };
  // every launch finishes an item, hands it to the single path, or at least doubles its arena, and 4096 states of at most
  // 128 arcs bound the arena: a bounded number of launches
  const auto slabs = batch_launch_loop<RbItem, RbCtl>(ctx, ctx->rm_batch, {"rm_epsilon_batch", BATCH_MAX_LAUNCHES, "an arena", RB_MAX_SLAB, "launch"},
                                                      std::move(open), carve, nullptr, launch, classify);
  auto outcome = [&](size_t i) {
    const wfst_fst* f = fsts[i];
    if (state[i] == SINGLE) return BatchOutcome::single();
    if (state[i] == EMPTY) return BatchOutcome::handle(rm_epsilon_empty(ctx, rm_epsilon_word(f->props, res[i].facts)));
    if (state[i] == TRIVIAL)  // rm_epsilon_fst's own answer: a copy of the input, word included
      return BatchOutcome::adopt({f->n_states, f->n_arcs, -1, f->props, f->dev.offsets, f->dev.arcs, f->dev.finals});
    return BatchOutcome::adopt({res[i].n_out, res[i].e_out, (int64_t)res[i].start_out, rm_epsilon_word(f->props, res[i].facts),
                                res[i].off, res[i].arcs, res[i].fin});
  };
  batch_finish(ctx, ctx->rm_batch, n, outs, in_kernel, outcome, [&](size_t i) { return rm_epsilon_fst(ctx, fsts[i]); });
}

}  // namespace wfst
