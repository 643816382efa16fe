// top_sort.hip — state_sort and top_sort on the device: a NEW handle, the input is left as it is.
// Reference: rustfst/src/algorithms/state_sort.rs:16-78, top_sort.rs:76-94 over dfs_visit.rs:97-187 (TopOrderVisitor:
// order[s] = the rank of s in the REVERSE finishing order of a sequential depth-first search whose roots are the start
// state, then 0, 1, 2, .., and which follows the arcs of a state in their stored order).
//
// That order is computed without a sequential walk.  A virtual super-root S (id n, depth 0) gets the arc
// list [start, 0, 1, .., n - 1]: state v's root slot is 0 if v == start, else 1 + v.  The search of S alone is the
// reference's search.  The ROOT PATH of a slot (u, i) — arc i of state u — is the list of arc positions from S down the
// search tree to u, then i; the tree parent of v is its in-slot with the lexicographically smallest root path, because the
// search reaches v first along it.  On a DAG every source of an in-slot of v lies on a lower Kahn level than v, so level
// after level every tree parent is final when it is read.
//   levels   Kahn peel from the source side: level 1 = the states without an in-arc (S precedes every state), a state
//            joins the level after its last predecessor's.  States left over when the peel ends: a cycle, and the CYCLIC
//            exit — nothing else runs.  level_states holds the levels one after the other, level_off their bounds.
//   select   levels 1, 2, ..: every state takes the minimum of its in-slots by ts_less, then its root slot against the
//            winner (O(1): the slot against rootidx of the winner's source), and writes par, cidx, depth, rootidx and its
//            row of the binary-lifting table up[j][v] = the 2^j-th tree ancestor (J rows, 2^J > levels).
//            ts_less(a, b): same source: the positions; else lift the deeper source to the other's depth + 1 — if its
//            parent IS the other source, that child's cidx against the other slot's position — else lift both to just
//            below their lowest common ancestor and compare the two cidx.
//   sizes    levels last .. 1: size[par[v]] += size[v] (every descendant lies on a higher level).
//   pre      S's row through the device scan, then levels 1, 2, ..: state u walks its row in arc order,
//            run = pre[u] + 1; every arc (u, i) -> t with (par[t], cidx[t]) == (u, i) gives pre[t] = run, run += size[t].
//   order    without S: post(v) = (pre[v] - 1) - (depth[v] - 1) + size[v] - 1, order[v] = n - 1 - post(v); it goes through
//            the permutation check of a caller's order before the apply kernels scatter by it.
//   apply    the state_sort kernels, which wfst_state_sort runs too: new offsets by a scan of the permuted row lengths,
//            arcs copied with nextstate = order[nextstate], finals scattered.
// Two regimes, as in determinize.hip: NARROW = ONE workgroup runs level after level of a phase inside one launch, a
// workgroup barrier between levels (lattices: hundreds of levels of a handful of states); WIDE = one device-wide launch
// per level and phase.  The host switches by the width of the next level (TOP_SORT_NARROW_STATES);
// WFST_TOP_SORT_PATH=narrow|wide pins one.  Work mapping inside a level, the same in both regimes: a lane per state; a
// state with TOP_SORT_WAVE_INDEG in-slots or more (select) or a row of TOP_SORT_WAVE_ROW arcs or more (pre) is handed to
// its whole wave (a strided minimum and a butterfly reduce; a wave scan over the row).  Every route gives the same FST.
// The list form (wfst_top_sort_batch) is ONE launch of top_sort_batch_kernel below, one workgroup per
// item: for items of a few hundred states the reference's sequential search itself (top_sort_dfs.h), run by one lane on
// 16-bit arrays in LDS, then the apply pass by all lanes.  An item beyond 4096 states or 16384 arcs goes through top_sort_fst.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "batch_driver.h"
#include "common.h"
#include "fst_props.h"
#include "top_sort_dfs.h"
#include "wg_ops.h"

namespace wfst {
namespace {

constexpr uint32_t BLOCK = 256;  // threads per workgroup of every kernel here
constexpr uint32_t WAVE = 64;
constexpr uint32_t TOP_SORT_NARROW_STATES = 256;  // a level of at most this many states runs in the one-workgroup kernels
constexpr uint32_t TOP_SORT_WAVE_INDEG = 32;      // select: in-slots from which a state is taken by its wave
constexpr uint32_t TOP_SORT_WAVE_ROW = 64;        // pre: arcs from which a row is walked by its wave
constexpr uint32_t NO_STATE = WFST_NO_STATE_ID;
// statesort_properties() (fst_properties/properties.rs:319-348)
constexpr uint64_t STATESORT_MASK = props::ALL & ~(props::TOP_SORTED | props::NOT_TOP_SORTED | props::STRING | props::NOT_STRING);
constexpr uint64_t TOP_SORTED_BITS = props::ACYCLIC | props::INITIAL_ACYCLIC | props::TOP_SORTED;
constexpr uint64_t CYCLIC_BITS = props::CYCLIC | props::NOT_TOP_SORTED;

// the largest s in [0, hi] with off[s] <= j (off ascending, off[0] = 0)
__device__ __forceinline__ uint32_t row_of(const uint32_t* __restrict__ off, uint32_t hi, uint32_t j) {
  uint32_t lo = 0;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo + 1) / 2;
    if (off[mid] <= j)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

// ---------------------------------------------------------------- state_sort
// bad |= 1 unless order is a permutation of [0, n): a value beyond the states, or one met twice (mark zeroed by the caller)
__global__ __launch_bounds__(BLOCK) void order_check_kernel(const uint32_t* __restrict__ order, uint32_t n, uint32_t* __restrict__ mark,
                                                            uint32_t* __restrict__ bad) {
  for (uint32_t s = blockIdx.x * BLOCK + threadIdx.x; s < n; s += gridDim.x * BLOCK) {
    const uint32_t o = order[s];
    if (o >= n || atomicAdd(&mark[o], 1u) != 0u) atomicOr(bad, 1u);
  }
}
__global__ __launch_bounds__(BLOCK) void sort_state_kernel(const uint32_t* __restrict__ off, const float* __restrict__ fin,
                                                           const uint32_t* __restrict__ order, uint32_t n, uint32_t* __restrict__ deg,
                                                           float* __restrict__ fin_out) {
  if (blockIdx.x == 0 && threadIdx.x == 0) deg[n] = 0u;
  for (uint32_t s = blockIdx.x * BLOCK + threadIdx.x; s < n; s += gridDim.x * BLOCK) {
    const uint32_t o = order[s];
    deg[o] = off[s + 1] - off[s];
    fin_out[o] = fin[s];
  }
}
// one lane per arc: a 16-byte load, nextstate remapped, a 16-byte store at the row's new place
__global__ __launch_bounds__(BLOCK) void sort_copy_kernel(const uint32_t* __restrict__ off, const wfst_tr* __restrict__ arcs,
                                                          const uint32_t* __restrict__ order, const uint32_t* __restrict__ off_out,
                                                          wfst_tr* __restrict__ arcs_out, uint32_t n, uint64_t n_arcs) {
  const uint4* __restrict__ src = reinterpret_cast<const uint4*>(arcs);
  uint4* __restrict__ dst = reinterpret_cast<uint4*>(arcs_out);
  for (uint64_t g = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; g < n_arcs; g += (uint64_t)gridDim.x * BLOCK) {
    const uint32_t j = (uint32_t)g;
    const uint32_t s = row_of(off, n - 1u, j);
    uint4 a = src[j];
    a.w = order[a.w];
    dst[off_out[order[s]] + (j - off[s])] = a;
  }
}

// ---------------------------------------------------------------- top_sort
struct Ts {
  const uint32_t* off;   // [n + 1] the input
  const wfst_tr* arcs;
  const uint32_t* roff;  // [n + 1] in-slots of every state ..
  const uint2* rin;      // [E] .. as {source state, arc position}, in no particular order
  const uint32_t* level_states;  // [n] the levels one after the other
  const uint32_t* level_off;     // [levels + 2] level l = level_states[level_off[l], level_off[l + 1]), l = 1 .. levels
  uint32_t* up;       // [J][N] up[0] = par
  uint32_t* cidx;     // [N] position of the tree arc in the parent's row (a root: its root slot)
  uint32_t* depth;    // [N]
  uint32_t* rootidx;  // [N] root slot of the tree root above the state
  uint32_t* size;     // [N] states of the subtree
  uint32_t* pre;      // [N] preorder number, S = 0
  uint32_t* ctr;      // [3] states_compared, wave_states, max depth
  uint32_t n, N, J, start;
};
enum : int { PH_SELECT = 0, PH_SIZES = 1, PH_PRE = 2 };

__global__ __launch_bounds__(BLOCK) void rin_fill_kernel(const uint32_t* __restrict__ off, const wfst_tr* __restrict__ arcs,
                                                         const uint32_t* __restrict__ roff, uint32_t* __restrict__ cursor,
                                                         uint2* __restrict__ rin, uint32_t n, uint64_t n_arcs) {
  for (uint64_t g = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; g < n_arcs; g += (uint64_t)gridDim.x * BLOCK) {
    const uint32_t j = (uint32_t)g;
    const uint32_t s = row_of(off, n - 1u, j);
    const uint32_t t = arcs[j].nextstate;
    rin[roff[t] + atomicAdd(&cursor[t], 1u)] = make_uint2(s, j - off[s]);
  }
}

// level 1: the states without an in-arc.  ctl[0] = states placed in level_states so far.
__global__ __launch_bounds__(BLOCK) void level_one_kernel(const uint32_t* __restrict__ indeg, uint32_t n, uint32_t* __restrict__ level_states,
                                                          uint32_t* __restrict__ level_off, uint32_t* __restrict__ ctl) {
  if (blockIdx.x == 0 && threadIdx.x == 0) level_off[1] = 0u;
  for (uint32_t v = blockIdx.x * BLOCK + threadIdx.x; v < n; v += gridDim.x * BLOCK)
    if (indeg[v] == 0u) level_states[atomicAdd(&ctl[0], 1u)] = v;
}
// WIDE: level `lvl` = level_states[lo, hi) with ctl[0] == hi: its arcs are taken from indeg, a state that reaches 0 joins
// the next level at ctl[0]++
__global__ __launch_bounds__(BLOCK) void peel_wide_kernel(const uint32_t* __restrict__ off, const wfst_tr* __restrict__ arcs, uint32_t* indeg,
                                                          uint32_t* level_states, uint32_t* __restrict__ level_off, uint32_t* ctl,
                                                          uint32_t lvl, uint32_t lo, uint32_t hi) {
  if (blockIdx.x == 0 && threadIdx.x == 0) level_off[lvl + 1] = hi;
  for (uint32_t idx = lo + blockIdx.x * BLOCK + threadIdx.x; idx < hi; idx += gridDim.x * BLOCK) {
    const uint32_t u = level_states[idx];
    for (uint32_t i = off[u], e = off[u + 1]; i < e; ++i) {
      const uint32_t t = arcs[i].nextstate;
      if (atomicSub(&indeg[t], 1u) == 1u) level_states[atomicAdd(&ctl[0], 1u)] = t;
    }
  }
}
// NARROW: one workgroup peels level after level from `lvl` = [lo, hi) on, until the next level is empty or wider than
// `cap`.  Leaves ctl = {states placed, the next level, its first index}.
__global__ __launch_bounds__(BLOCK) void peel_narrow_kernel(const uint32_t* __restrict__ off, const wfst_tr* __restrict__ arcs, uint32_t* indeg,
                                                            uint32_t* level_states, uint32_t* level_off, uint32_t* ctl, uint32_t lvl,
                                                            uint32_t lo, uint32_t hi, uint32_t cap) {
  __shared__ uint32_t s_cnt;
  for (;;) {
    if (threadIdx.x == 0) s_cnt = 0u;
    __syncthreads();
    for (uint32_t idx = lo + threadIdx.x; idx < hi; idx += BLOCK) {
      const uint32_t u = level_states[idx];
      for (uint32_t i = off[u], e = off[u + 1]; i < e; ++i) {
        const uint32_t t = arcs[i].nextstate;
        if (atomicSub(&indeg[t], 1u) == 1u) level_states[hi + atomicAdd(&s_cnt, 1u)] = t;
      }
    }
    __syncthreads();
    const uint32_t cnt = s_cnt;
    if (threadIdx.x == 0) level_off[lvl + 1] = hi;
    ++lvl;
    lo = hi;
    hi += cnt;
    __syncthreads();  // everybody has read s_cnt
    if (cnt == 0u || cnt > cap) break;
  }
  if (threadIdx.x == 0) ctl[0] = hi, ctl[1] = lvl, ctl[2] = lo;
}

// size = 1 everywhere; S: the root of the tree, its own ancestor in every lifting row
__global__ __launch_bounds__(BLOCK) void tree_init_kernel(Ts ts) {
  for (uint32_t v = blockIdx.x * BLOCK + threadIdx.x; v < ts.N; v += gridDim.x * BLOCK) {
    ts.size[v] = 1u;
    if (v == ts.n) {
      for (uint32_t j = 0; j < ts.J; ++j) ts.up[(size_t)j * ts.N + v] = v;
      ts.cidx[v] = 0u, ts.depth[v] = 0u, ts.rootidx[v] = 0u, ts.pre[v] = 0u;
    }
  }
}

__device__ __forceinline__ uint32_t ts_lift(const Ts& ts, uint32_t x, uint32_t d) {
  for (uint32_t j = 0; d; ++j, d >>= 1)
    if (d & 1u) x = ts.up[(size_t)j * ts.N + x];
  return x;
}
// does slot a = {source, position} come before slot b in root-path order?  (two distinct in-slots of one state)
__device__ bool ts_less(const Ts& ts, uint2 a, uint2 b) {
  if (a.x == b.x) return a.y < b.y;
  uint32_t x = a.x, y = b.x;
  const uint32_t dx = ts.depth[x], dy = ts.depth[y];
  if (dx > dy) {
    x = ts_lift(ts, x, dx - dy - 1u);
    const uint32_t p = ts.up[x];
    if (p == y) return ts.cidx[x] < b.y;  // b's source is an ancestor of a's: the child towards a against b's position
    x = p;
  } else if (dy > dx) {
    y = ts_lift(ts, y, dy - dx - 1u);
    const uint32_t p = ts.up[y];
    if (p == x) return a.y < ts.cidx[y];
    y = p;
  }
  for (uint32_t j = ts.J; j-- > 0u;) {  // equal depths, x != y: to just below the lowest common ancestor
    const uint32_t ux = ts.up[(size_t)j * ts.N + x], uy = ts.up[(size_t)j * ts.N + y];
    if (ux != uy) x = ux, y = uy;
  }
  return ts.cidx[x] < ts.cidx[y];
}
// v's tree arc: the best real in-slot (has_best) against its root slot, then everything that hangs on the parent
__device__ void ts_settle(const Ts& ts, uint32_t v, bool has_best, uint2 best, bool lifted) {
  const uint32_t slot = v == ts.start ? 0u : 1u + v;
  uint32_t p = ts.n, c = slot, d = 1u, r = slot;
  if (has_best && ts.rootidx[best.x] < slot) p = best.x, c = best.y, d = ts.depth[p] + 1u, r = ts.rootidx[p];
  ts.cidx[v] = c, ts.depth[v] = d, ts.rootidx[v] = r;
  uint32_t a = p;
  ts.up[v] = a;
  for (uint32_t j = 1; j < ts.J; ++j) {
    a = ts.up[(size_t)(j - 1u) * ts.N + a];
    ts.up[(size_t)j * ts.N + v] = a;
  }
  atomicMax(&ts.ctr[2], d);
  if (lifted) atomicAdd(&ts.ctr[0], 1u);
}
__device__ void ts_select(const Ts& ts, uint32_t v, bool on, uint32_t lane) {
  uint32_t b = 0, e = 0;
  if (on && v != ts.start) b = ts.roff[v], e = ts.roff[v + 1];  // (the start's slot 0 is the smallest root path there is)
  const bool by_wave = e - b >= TOP_SORT_WAVE_INDEG;
  if (on && !by_wave) {
    uint2 best = make_uint2(0u, 0u);
    bool lifted = false;
    for (uint32_t k = b; k < e; ++k) {
      const uint2 c = ts.rin[k];
      if (k == b) {
        best = c;
        continue;
      }
      lifted |= c.x != best.x;
      if (ts_less(ts, c, best)) best = c;
    }
    ts_settle(ts, v, e > b, best, lifted);
  }
  for (unsigned long long m = __ballot(by_wave); m; m &= m - 1ull) {
    const int src = __ffsll((long long)m) - 1;
    const uint32_t wv = __shfl(v, src), wb = __shfl(b, src), we = __shfl(e, src);
    uint2 best = make_uint2(0u, 0u);
    bool has = false, lifted = false;
    for (uint32_t k = wb + lane; k < we; k += WAVE) {
      const uint2 c = ts.rin[k];
      if (!has) {
        best = c, has = true;
        continue;
      }
      lifted |= c.x != best.x;
      if (ts_less(ts, c, best)) best = c;
    }
    for (uint32_t d = WAVE / 2; d; d >>= 1) {
      const uint2 o = make_uint2(__shfl_xor(best.x, d), __shfl_xor(best.y, d));
      const bool o_has = __shfl_xor((int)has, d) != 0;
      if (o_has && !has) {
        best = o, has = true;
      } else if (o_has && (o.x != best.x || o.y != best.y)) {
        lifted |= o.x != best.x;
        if (ts_less(ts, o, best)) best = o;
      }
    }
    lifted = __any(lifted);
    if (lane == 0u) {
      ts_settle(ts, wv, true, best, lifted);
      atomicAdd(&ts.ctr[1], 1u);
    }
  }
}
__device__ __forceinline__ void ts_sizes(const Ts& ts, uint32_t v, bool on) {
  // (the children's adds are atomics of other lanes: read them where they were made)
  if (on) atomicAdd(&ts.size[ts.up[v]], __hip_atomic_load(&ts.size[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ void ts_pre(const Ts& ts, uint32_t u, bool on, uint32_t lane) {
  uint32_t b = 0, e = 0;
  if (on) b = ts.off[u], e = ts.off[u + 1];
  const bool by_wave = e - b >= TOP_SORT_WAVE_ROW;
  if (on && !by_wave) {
    uint32_t run = ts.pre[u] + 1u;
    for (uint32_t i = b; i < e; ++i) {
      const uint32_t t = ts.arcs[i].nextstate;
      if (ts.up[t] == u && ts.cidx[t] == i - b) ts.pre[t] = run, run += ts.size[t];
    }
  }
  for (unsigned long long m = __ballot(by_wave); m; m &= m - 1ull) {
    const int src = __ffsll((long long)m) - 1;
    const uint32_t wu = __shfl(u, src), wb = __shfl(b, src), we = __shfl(e, src);
    uint32_t run = ts.pre[wu] + 1u;
    for (uint32_t base = wb; base < we; base += WAVE) {
      const uint32_t i = base + lane;
      uint32_t t = NO_STATE, val = 0u;
      if (i < we) {
        t = ts.arcs[i].nextstate;
        if (ts.up[t] == wu && ts.cidx[t] == i - wb)
          val = ts.size[t];
        else
          t = NO_STATE;
      }
      uint32_t x = val;
      for (uint32_t d = 1; d < WAVE; d <<= 1) {
        const uint32_t y = __shfl_up(x, d);
        if (lane >= d) x += y;
      }
      if (t != NO_STATE) ts.pre[t] = run + (x - val);
      run += __shfl(x, (int)WAVE - 1);
    }
  }
}
// one level = level_states[lo, hi): wave w of the launch takes 64 consecutive places per turn (every lane of a wave runs
// the same number of turns, so the cross-lane steps above see the whole wave)
template <int PH>
__device__ __forceinline__ void ts_level(const Ts& ts, uint32_t lo, uint32_t hi, uint32_t first, uint32_t stride) {
  const uint32_t lane = threadIdx.x & (WAVE - 1u);
  for (uint32_t base = lo + first; base < hi; base += stride) {
    const uint32_t idx = base + lane;
    const bool on = idx < hi;
    const uint32_t v = on ? ts.level_states[idx] : NO_STATE;
    if (PH == PH_SELECT) ts_select(ts, v, on, lane);
    if (PH == PH_SIZES) ts_sizes(ts, v, on);
    if (PH == PH_PRE) ts_pre(ts, v, on, lane);
  }
}
template <int PH>
__global__ __launch_bounds__(BLOCK) void sweep_wide_kernel(Ts ts, uint32_t lo, uint32_t hi) {
  ts_level<PH>(ts, lo, hi, blockIdx.x * BLOCK + (threadIdx.x & ~(WAVE - 1u)), gridDim.x * BLOCK);
}
// levels first .. last in ascending (step = 1) or descending order, a workgroup barrier between two of them
template <int PH>
__global__ __launch_bounds__(BLOCK) void sweep_narrow_kernel(Ts ts, uint32_t first, uint32_t last, int descending) {
  for (uint32_t k = 0; k <= last - first; ++k) {
    const uint32_t l = descending ? last - k : first + k;
    ts_level<PH>(ts, ts.level_off[l], ts.level_off[l + 1], threadIdx.x & ~(WAVE - 1u), BLOCK);
    __syncthreads();
  }
}

// S's row: slot k holds the size of the tree whose root took it (0: nobody did)
__global__ __launch_bounds__(BLOCK) void root_sizes_kernel(Ts ts, uint32_t* __restrict__ slot_size) {
  for (uint32_t k = blockIdx.x * BLOCK + threadIdx.x; k <= ts.N; k += gridDim.x * BLOCK) {
    uint32_t val = 0u;
    if (k < ts.N) {
      const uint32_t v = k == 0u ? ts.start : k - 1u;
      if (ts.up[v] == ts.n && ts.cidx[v] == k) val = ts.size[v];
    }
    slot_size[k] = val;
  }
}
__global__ __launch_bounds__(BLOCK) void root_pre_kernel(Ts ts, const uint32_t* __restrict__ slot_pre) {
  for (uint32_t v = blockIdx.x * BLOCK + threadIdx.x; v < ts.n; v += gridDim.x * BLOCK)
    if (ts.up[v] == ts.n) ts.pre[v] = 1u + slot_pre[ts.cidx[v]];
}
__global__ __launch_bounds__(BLOCK) void order_kernel(Ts ts, uint32_t* __restrict__ order) {
  for (uint32_t v = blockIdx.x * BLOCK + threadIdx.x; v < ts.n; v += gridDim.x * BLOCK) {
    const uint32_t post = ts.pre[v] - ts.depth[v] + ts.size[v] - 1u;
    order[v] = ts.n - 1u - post;
  }
}

// ---------------------------------------------------------------- the host side
uint32_t grid_for(const wfst_ctx* ctx, uint64_t items) {
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((items + BLOCK - 1) / BLOCK, (uint64_t)ctx->n_cus * 8));
}

void check_operand(wfst_ctx* ctx, const wfst_fst* f, const char* op) {
  if (f->device != ctx->device) throw Error(std::string(op) + ": the operand lives on another device");
}

wfst_fst* copy_with_word(wfst_ctx* ctx, const wfst_fst* f, uint64_t word) {
  if (f->n_states == 0) {
    HostCsr h;
    h.offsets.push_back(0);
    return make_host_fst(ctx, 0, f->start, word & props::ALL, std::move(h));
  }
  ensure_device(const_cast<wfst_fst*>(f));
  return adopt_device(ctx, f->n_states, f->n_arcs, f->start, word & props::ALL, f->dev.offsets, f->dev.arcs, f->dev.finals);
}

// state_sort.rs:40-75 for an order that is known to be a permutation (d_order on the device); f has a start state
wfst_fst* apply_order(wfst_ctx* ctx, const wfst_fst* f, const uint32_t* d_order, uint32_t new_start, uint64_t word) {
  hipStream_t st = ctx->stream;
  DevicePool& pool = *ctx->pool;
  const uint32_t n = f->n_states;
  DBuf<uint32_t> deg(pool, (size_t)n + 1), off_out(pool, (size_t)n + 1);
  DBuf<float> fin_out(pool, n);
  DBuf<wfst_tr> arcs_out(pool, f->n_arcs);
  sort_state_kernel<<<grid_for(ctx, n), BLOCK, 0, st>>>(f->dev.offsets, f->dev.finals, d_order, n, deg.p, fin_out.p);
  HIP_CHECK(hipGetLastError());
  DBuf<uint8_t> scan_tmp = exclusive_scan_u32(ctx, deg.p, off_out.p, (size_t)n + 1);
  if (f->n_arcs) {
    sort_copy_kernel<<<grid_for(ctx, f->n_arcs), BLOCK, 0, st>>>(f->dev.offsets, f->dev.arcs, d_order, off_out.p, arcs_out.p, n, f->n_arcs);
    HIP_CHECK(hipGetLastError());
  }
  Handle out(adopt_device(ctx, n, f->n_arcs, (int64_t)new_start, word & props::ALL, off_out.p, arcs_out.p, fin_out.p));
  HIP_CHECK(hipStreamSynchronize(st));
  return out.release();
}

struct Seg {
  uint32_t first, last;  // levels
  bool narrow;
};

template <int PH>
void sweep(wfst_ctx* ctx, const Ts& ts, const std::vector<Seg>& segs, const std::vector<uint32_t>& level_off, bool descending) {
  for (size_t k = 0; k < segs.size(); ++k) {
    const Seg& sg = segs[descending ? segs.size() - 1 - k : k];
    if (sg.narrow) {
      sweep_narrow_kernel<PH><<<1, BLOCK, 0, ctx->stream>>>(ts, sg.first, sg.last, descending ? 1 : 0);
      ++ctx->top_sort.narrow_launches;
    } else {
      const uint32_t lo = level_off[sg.first], hi = level_off[sg.first + 1];
      sweep_wide_kernel<PH><<<grid_for(ctx, hi - lo), BLOCK, 0, ctx->stream>>>(ts, lo, hi);
      ++ctx->top_sort.wide_launches;
    }
    HIP_CHECK(hipGetLastError());
  }
}

}  // namespace

wfst_fst* state_sort_fst(wfst_ctx* ctx, const wfst_fst* f, const uint32_t* order, size_t n_order) {
  check_operand(ctx, f, "state_sort");
  const uint32_t n = f->n_states;
  if (n_order != n)  // (state_sort.rs:21-26)
    throw Error("StateSort : Bad order vector size : " + std::to_string(n_order) + ". Expected " + std::to_string(n));
  if (n && !order) throw Error("null pointer");
  hipStream_t st = ctx->stream;
  DevicePool& pool = *ctx->pool;
  // not a permutation: only a debug_assert in the reference; refused here before anything is written
  DBuf<uint32_t> d_order(pool, n), mark(pool, (size_t)n + 1);
  if (n) {
    HIP_CHECK(hipMemcpyAsync(d_order.p, order, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemsetAsync(mark.p, 0, ((size_t)n + 1) * sizeof(uint32_t), st));
    order_check_kernel<<<grid_for(ctx, n), BLOCK, 0, st>>>(d_order.p, n, mark.p, mark.p + n);
    HIP_CHECK(hipGetLastError());
    if (read_u32(ctx, mark.p + n)) throw Error("state_sort: order is not a permutation of the states");
  }
  if (f->start < 0) return copy_with_word(ctx, f, f->props);  // (:27-29) before anything is touched
  ensure_device(const_cast<wfst_fst*>(f));
  return apply_order(ctx, f, d_order.p, order[f->start], f->props & STATESORT_MASK);
}

wfst_fst* top_sort_fst(wfst_ctx* ctx, const wfst_fst* f) {
  ctx->top_sort = wfst_ctx::TopSortStats{};
  wfst_ctx::TopSortStats& stats = ctx->top_sort;
  const Path path = path_knob("WFST_TOP_SORT_PATH");
  check_operand(ctx, f, "top_sort");
  const uint32_t n = f->n_states;
  const uint64_t word = f->props & props::ALL;
  if (f->start < 0) {  // dfs_visit returns an empty order (dfs_visit.rs:104-110), which state_sort takes only without states
    if (n == 0) return copy_with_word(ctx, f, word | TOP_SORTED_BITS);
    throw Error("StateSort : Bad order vector size : 0. Expected " + std::to_string(n));
  }
  ensure_device(const_cast<wfst_fst*>(f));
  hipStream_t st = ctx->stream;
  DevicePool& pool = *ctx->pool;
  const uint32_t N = n + 1u;
  const uint32_t* off = f->dev.offsets;
  const wfst_tr* arcs = f->dev.arcs;

  // ---- levels
  DBuf<uint32_t> indeg(pool, N), roff(pool, N), level_states(pool, n), level_off(pool, (size_t)n + 2), ctl(pool, 4);
  HIP_CHECK(hipMemsetAsync(indeg.p, 0, (size_t)N * sizeof(uint32_t), st));
  HIP_CHECK(hipMemsetAsync(ctl.p, 0, 4 * sizeof(uint32_t), st));
  count_indegrees(ctx, arcs, f->n_arcs, indeg.p);
  DBuf<uint8_t> scan_tmp = exclusive_scan_u32(ctx, indeg.p, roff.p, N);
  level_one_kernel<<<grid_for(ctx, n), BLOCK, 0, st>>>(indeg.p, n, level_states.p, level_off.p, ctl.p);
  HIP_CHECK(hipGetLastError());
  const uint32_t cap = path == Path::Narrow ? 0xFFFFFFFFu : path == Path::Wide ? 0u : TOP_SORT_NARROW_STATES;
  uint32_t lvl = 1, lo = 0, hi = read_u32(ctx, ctl.p);
  while (hi > lo) {
    if (hi - lo <= cap) {
      peel_narrow_kernel<<<1, BLOCK, 0, st>>>(off, arcs, indeg.p, level_states.p, level_off.p, ctl.p, lvl, lo, hi, cap);
      HIP_CHECK(hipGetLastError());
      uint32_t h[3];
      HIP_CHECK(hipMemcpyAsync(h, ctl.p, sizeof(h), hipMemcpyDeviceToHost, st));
      HIP_CHECK(hipStreamSynchronize(st));
      ++stats.narrow_launches;
      stats.narrow_levels += h[1] - lvl;
      hi = h[0], lvl = h[1], lo = h[2];
    } else {
      peel_wide_kernel<<<grid_for(ctx, hi - lo), BLOCK, 0, st>>>(off, arcs, indeg.p, level_states.p, level_off.p, ctl.p, lvl, lo, hi);
      HIP_CHECK(hipGetLastError());
      ++stats.wide_launches;
      ++lvl;
      lo = hi;
      hi = read_u32(ctx, ctl.p);
    }
  }
  const uint32_t levels = lvl - 1u;
  stats.levels = levels;
  std::vector<uint32_t> h_level_off((size_t)levels + 2, 0u);
  HIP_CHECK(hipMemcpyAsync(h_level_off.data() + 1, level_off.p + 1, ((size_t)levels + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  for (uint32_t l = 1; l <= levels; ++l) stats.max_level_width = std::max<uint64_t>(stats.max_level_width, h_level_off[l + 1] - h_level_off[l]);
  if (hi < n) {  // states left over: a cycle somewhere (top_sort.rs:88-91)
    stats.cyclic = 1;
    return copy_with_word(ctx, f, word | CYCLIC_BITS);
  }
  std::vector<Seg> segs;  // as the peel was launched: maximal runs of narrow levels, every wide level alone
  for (uint32_t l = 1; l <= levels; ++l) {
    const bool narrow = h_level_off[l + 1] - h_level_off[l] <= cap;
    if (narrow && !segs.empty() && segs.back().narrow)
      segs.back().last = l;
    else
      segs.push_back(Seg{l, l, narrow});
  }

  // ---- the transpose and the tree
  uint32_t J = 1;
  while ((1ull << J) < (uint64_t)levels + 1) ++J;
  stats.lift_rows = J;
  DBuf<uint2> rin(pool, f->n_arcs);
  DBuf<uint32_t> up(pool, (size_t)J * N), cidx(pool, N), depth(pool, N), rootidx(pool, N), size(pool, N), pre(pool, N), ctr(pool, 4),
      slot_size(pool, (size_t)N + 1), slot_pre(pool, (size_t)N + 1), order(pool, n);
  if (f->n_arcs) {
    HIP_CHECK(hipMemsetAsync(indeg.p, 0, (size_t)N * sizeof(uint32_t), st));  // (the peel left zeros; now the fill's cursors)
    rin_fill_kernel<<<grid_for(ctx, f->n_arcs), BLOCK, 0, st>>>(off, arcs, roff.p, indeg.p, rin.p, n, f->n_arcs);
    HIP_CHECK(hipGetLastError());
  }
  HIP_CHECK(hipMemsetAsync(ctr.p, 0, 4 * sizeof(uint32_t), st));
  const Ts ts{off, arcs, roff.p, rin.p, level_states.p, level_off.p, up.p, cidx.p, depth.p, rootidx.p, size.p, pre.p, ctr.p,
              n, N, J, (uint32_t)f->start};
  tree_init_kernel<<<grid_for(ctx, N), BLOCK, 0, st>>>(ts);
  HIP_CHECK(hipGetLastError());
  sweep<PH_SELECT>(ctx, ts, segs, h_level_off, false);
  sweep<PH_SIZES>(ctx, ts, segs, h_level_off, true);
  root_sizes_kernel<<<grid_for(ctx, (uint64_t)N + 1), BLOCK, 0, st>>>(ts, slot_size.p);
  HIP_CHECK(hipGetLastError());
  DBuf<uint8_t> scan_tmp2 = exclusive_scan_u32(ctx, slot_size.p, slot_pre.p, (size_t)N + 1);
  root_pre_kernel<<<grid_for(ctx, n), BLOCK, 0, st>>>(ts, slot_pre.p);
  HIP_CHECK(hipGetLastError());
  sweep<PH_PRE>(ctx, ts, segs, h_level_off, false);
  order_kernel<<<grid_for(ctx, n), BLOCK, 0, st>>>(ts, order.p);
  HIP_CHECK(hipGetLastError());
  // the apply kernels scatter by `order`: they run only behind the check wfst_state_sort makes of a caller's order
  HIP_CHECK(hipMemsetAsync(slot_size.p, 0, ((size_t)N + 1) * sizeof(uint32_t), st));
  order_check_kernel<<<grid_for(ctx, n), BLOCK, 0, st>>>(order.p, n, slot_size.p, slot_size.p + n);
  HIP_CHECK(hipGetLastError());
  uint32_t h_ctr[3], new_start = 0, bad = 0;
  HIP_CHECK(hipMemcpyAsync(h_ctr, ctr.p, sizeof(h_ctr), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(&new_start, order.p + f->start, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(&bad, slot_size.p + n, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  if (bad) throw Error("top_sort: internal error: the computed order is not a permutation of the states");
  stats.states_compared = h_ctr[0], stats.wave_states = h_ctr[1], stats.max_tree_depth = h_ctr[2];
  // ---- apply (top_sort.rs:84-87): state_sort's word, then the three bits set and nothing cleared
  return apply_order(ctx, f, order.p, new_start, (word & STATESORT_MASK) | TOP_SORTED_BITS);
}

// ================================================================ batch (wfst_top_sort_batch)
namespace {

constexpr uint32_t TSB_MAX_STATES = 4096;  // the in_kernel rule (include/wfst.h): tr_sum_batch's sizes
constexpr uint32_t TSB_MAX_ARCS = 16384;
constexpr size_t TSB_MAX_SLAB = (size_t)8 << 30;  // all slices of a call together; beyond: KO before any launch
constexpr size_t TSB_MAX_LDS = 64u << 10;         // what one launch may ask for
// TsbCtl::exit.  TSB_BAD_ITEM: sizes beyond the rule, a start state or an arc's nextstate beyond the states, offsets beyond
// the arcs (the host never sends one); TSB_STEPS: the search passed its step bound
enum : uint32_t { TSB_RUNNING = 0, TSB_DONE = 1, TSB_BAD_ITEM = 2, TSB_STEPS = 3 };

struct TsbCtl {  // one per item, at the head of the slab; read back once
  uint32_t exit;
  uint32_t cyclic;
  uint32_t new_start;
  uint32_t n_states, n_arcs;
  uint32_t pad[3];
};
struct TsbItem {
  const uint32_t* off;
  const wfst_tr* arcs;
  const float* fin;
  uint32_t n, E, start;
  TsbCtl* ctl;
  // the slice
  uint32_t* deg;      // [n + 1] row lengths by new id
  uint32_t* off_out;  // [n + 1] the result
  float* fin_out;     // [n]
  wfst_tr* arcs_out;  // [E]
};

// the dynamic LDS of an item: next[E], off[n + 1], rank[n], stack[n] of top_sort_dfs.h, 16-bit words one after the other
constexpr size_t tsb_lds_bytes(uint32_t n, uint32_t E) { return ((size_t)E + 3u * (size_t)n + 1u) * sizeof(uint16_t); }
static_assert(tsb_lds_bytes(TSB_MAX_STATES, TSB_MAX_ARCS) + (MB_TPB + 3) * sizeof(uint32_t) <= TSB_MAX_LDS, "the rule's largest item fits");
static_assert(TSB_MAX_STATES < TSD_GREY && TSB_MAX_ARCS <= 0xFFFFu, "ranks, cursors and offsets fit 16 bits");

// one workgroup per item: stage (all threads), the reference's search (one lane, top_sort_dfs.h), apply (all threads:
// state_sort.rs:40-75 for the order the search left in LDS; a cyclic item takes the identity)
__global__ void __launch_bounds__(MB_TPB) top_sort_batch_kernel(const TsbItem* __restrict__ items) {
  extern __shared__ uint16_t tsb_lds[];
  __shared__ uint32_t part[MB_TPB + 1];
  __shared__ uint32_t s_code, s_bad;
  const TsbItem it = items[blockIdx.x];
  const uint32_t tid = threadIdx.x, gl = tid & 15u;
  const uint32_t n = it.n, E = it.E;
  if (n == 0 || n > TSB_MAX_STATES || E > TSB_MAX_ARCS || it.start >= n) {  // (before any index is made of them)
    if (tid == 0) it.ctl->exit = TSB_BAD_ITEM;
    return;
  }
  uint16_t* next = tsb_lds;       // [E]
  uint16_t* off = next + E;       // [n + 1]
  uint16_t* rank = off + n + 1u;  // [n]
  uint16_t* stack = rank + n;     // [n]
  // ---- 1. stage
  if (tid == 0) s_bad = 0u;
  __syncthreads();
  for (uint32_t i = tid; i < E; i += MB_TPB) {
    const uint32_t t = it.arcs[i].nextstate;
    if (t >= n) s_bad = 1u;
    next[i] = (uint16_t)t;
  }
  for (uint32_t s = tid; s <= n; s += MB_TPB) {
    const uint32_t o = it.off[s];
    if (o > E || (s == n ? o != E : it.off[s + 1] < o)) s_bad = 1u;  // (the apply phase places rows by these)
    off[s] = (uint16_t)o;
    if (s < n) rank[s] = TSD_WHITE;
  }
  __syncthreads();
  if (s_bad) {
    if (tid == 0) it.ctl->exit = TSB_BAD_ITEM;
    return;
  }
  // ---- 2. search
  if (tid == 0) s_code = top_sort_dfs(next, off, n, it.start, rank, stack, top_sort_dfs_max_steps(n, E));
  __syncthreads();
  const uint32_t code = s_code;
  if (code == TSD_STEPS) {
    if (tid == 0) it.ctl->exit = TSB_STEPS;
    return;
  }
  if (code == TSD_CYCLIC) {
    for (uint32_t s = tid; s < n; s += MB_TPB) rank[s] = (uint16_t)s;
    __syncthreads();
  }
  // ---- 3. apply: row lengths and finals by new id, the new offsets, the arcs (16 lanes per state, 16-byte words)
  for (uint32_t s = tid; s <= n; s += MB_TPB) {
    if (s == n) {
      stg(&it.deg[n], 0u);
      continue;
    }
    const uint32_t o = rank[s];
    stg(&it.deg[o], (uint32_t)off[s + 1] - (uint32_t)off[s]);
    it.fin_out[o] = it.fin[s];
  }
  wg_bar();
  wg_exclusive_scan(it.deg, it.off_out, n + 1, part);
  const uint4* __restrict__ src = reinterpret_cast<const uint4*>(it.arcs);
  uint4* __restrict__ dst = reinterpret_cast<uint4*>(it.arcs_out);
  for (uint32_t s = tid >> 4; s < n; s += MB_TPB >> 4) {
    const uint32_t b = off[s], e = off[s + 1], base = ld(&it.off_out[rank[s]]);
    for (uint32_t i = b + gl; i < e; i += 16) {
      uint4 a = src[i];
      a.w = rank[next[i]];
      dst[base + (i - b)] = a;
    }
  }
  if (tid == 0) {
    it.ctl->cyclic = code == TSD_CYCLIC ? 1u : 0u;
    it.ctl->new_start = rank[it.start];
    it.ctl->n_states = n;
    it.ctl->n_arcs = E;
    it.ctl->exit = TSB_DONE;
  }
}

// carves one item's arrays out of the slab; it == nullptr only measures
size_t carve_top_sort_slice(Slab s, uint32_t n, uint32_t E, TsbItem* it) {
  TsbItem v{};
  v.deg = s.take<uint32_t>((size_t)n + 1);
  v.off_out = s.take<uint32_t>((size_t)n + 1);
  v.fin_out = s.take<float>(n);
  v.arcs_out = s.take<wfst_tr>(E);
  v.n = n;
  v.E = E;
  if (it) *it = v;  // (the input's side is the caller's)
  return s.at();
}

}  // namespace

// the host loop is batch_driver.h's, with the ownership check and one pass: every size is the input's, nothing grows
void top_sort_batch(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, wfst_fst** outs, uint8_t* in_kernel) {
  ctx->top_sort_batch = {};
  check_items_owned(ctx, fsts, n, "top_sort_batch");
  hipStream_t st = ctx->stream;
  enum : uint8_t { KERNEL, EMPTY, SINGLE };
  struct Ran {
    uint32_t cyclic = 0, new_start = 0;
    const uint32_t* off = nullptr;
    const wfst_tr* arcs = nullptr;
    const float* fin = nullptr;
  };
  std::vector<uint8_t> kind(n);
  std::vector<Ran> ran(n);
  std::vector<size_t> run;  // the items that occupy a workgroup
  size_t lds = 0;           // of the launch: its largest item's
  for (size_t i = 0; i < n; ++i) {
    const wfst_fst* f = fsts[i];
    // no start state: without states the single call's own early answer, with states its KO (both without a launch)
    kind[i] = f->start < 0 ? (f->n_states == 0 ? EMPTY : SINGLE)
              : (f->n_states <= TSB_MAX_STATES && f->n_arcs <= TSB_MAX_ARCS) ? KERNEL : SINGLE;
    if (kind[i] == KERNEL) {
      ensure_device(const_cast<wfst_fst*>(f));
      run.push_back(i);
      lds = std::max(lds, tsb_lds_bytes(f->n_states, (uint32_t)f->n_arcs));
    }
  }
  auto carve = [&](size_t i, Slab s, TsbItem* it) {
    const wfst_fst* f = fsts[i];
    const size_t end = carve_top_sort_slice(s, f->n_states, (uint32_t)f->n_arcs, it);
    if (it) {
      it->off = f->dev.offsets;
      it->arcs = f->dev.arcs;
      it->fin = f->dev.finals;
      it->start = (uint32_t)f->start;
    }
    return end;
  };
  auto launch = [&](const TsbItem* d_items, uint32_t m) { top_sort_batch_kernel<<<m, MB_TPB, lds, st>>>(d_items); };
  auto classify = [&](size_t i, const TsbCtl& c, const TsbItem& it) {
    const wfst_fst* f = fsts[i];
    if (c.exit != TSB_DONE || c.n_states != f->n_states || c.n_arcs != f->n_arcs || c.new_start >= f->n_states)
      throw Error("top_sort_batch: internal error: the kernel left item " + std::to_string(i) + " with exit code " +
                  std::to_string(c.exit));
    ran[i] = Ran{c.cyclic, c.new_start, it.off_out, it.arcs_out, it.fin_out};
    return BatchExit::FINISHED;
  };
  const auto slabs = batch_launch_loop<TsbItem, TsbCtl>(ctx, ctx->top_sort_batch, {"top_sort_batch", 1, nullptr, TSB_MAX_SLAB, "call"},
                                                        std::move(run), carve, nullptr, launch, classify);
  auto outcome = [&](size_t i) {
    const wfst_fst* f = fsts[i];
    const uint64_t word = f->props & props::ALL;
    if (kind[i] == SINGLE) return BatchOutcome::single();
    if (kind[i] == EMPTY) return BatchOutcome::handle(copy_with_word(ctx, f, word | TOP_SORTED_BITS));
    const Ran& r = ran[i];
    return BatchOutcome::adopt({f->n_states, f->n_arcs, (int64_t)r.new_start,
                                r.cyclic ? (word | CYCLIC_BITS) : ((word & STATESORT_MASK) | TOP_SORTED_BITS), r.off, r.arcs, r.fin});
  };
  batch_finish(ctx, ctx->top_sort_batch, n, outs, in_kernel, outcome, [&](size_t i) { return top_sort_fst(ctx, fsts[i]); });
}

}  // namespace wfst
