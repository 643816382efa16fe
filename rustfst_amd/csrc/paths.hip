// paths.hip — paths_iter (rustfst/src/fst_traits/paths_iterator.rs:24-62) of acyclic FSTs on the device: the table of
// all successful paths — input labels, output labels (label 0 dropped per tape, fst_path.rs:35-45) and the weight — in the
// order the reference's FIFO yields them, without replaying the FIFO.
//
// The FIFO holds prefixes sorted by (number of arcs, arc positions read lexicographically), so that is the order of the
// paths.  Four steps:
//   1. count.  Accessibility from the start, then sinks are peeled off the accessible subgraph level by level:
//      cnt[s] = [s final] + sum over the arcs of cnt[nextstate], u64 with saturating addition, and per arc the exclusive
//      prefix of that sum within its state (pre[], the final's 1 included).  Accessible states that are never peeled lie
//      on or before a cycle: KO, the reference would never return.  P = cnt[start] is compared with max_paths BEFORE
//      any per-path memory exists.
//   2. unrank.  Path r of [0, P) in depth-first order ("end here" first, then the arcs in order) is walked from the start
//      by one lane, which binary-searches pre[] of each state; it counts the arcs and the non-epsilon labels per tape.
//   3. reorder.  A stable radix sort (rocPRIM) of the keys (item, arc count) over the paths in (item, r) order: among
//      paths of one length depth-first rank order IS lexicographic arc-position order.
//   4. emit.  Scan of the label counts in final order (64-bit offsets), then every path is walked again and writes its
//      labels and its weight: ((one (x) w1) (x) w2 ...) (x) final with tropical.h's wtimes, in path order.
//
// Two routes for step 1.  wfst_fst_paths / wfst_fst_count_paths: device-wide launches, one per level of the search and
// one per level of the peel (an FST of any size).  wfst_fst_paths_batch: ONE launch of paths_count_batch_kernel, one
// workgroup per item, for every item of at most PB_MAX_STATES = 4096 states and PB_MAX_ARCS = 16384 arcs; an item beyond
// either limit takes the device-wide route and lands in the same table.  Steps 2-4 are grids over all paths of all
// items together, so a batch call's launch count depends neither on the length of the list nor on the items' depths.
#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "batch_driver.h"
#include "wg_ops.h"

namespace wfst {
namespace {

constexpr uint32_t PB_MAX_STATES = WFST_PATHS_BATCH_MAX_STATES;  // the in_kernel rule (include/wfst.h)
constexpr uint32_t PB_MAX_ARCS = WFST_PATHS_BATCH_MAX_ARCS;
constexpr size_t PB_MAX_SLAB = (size_t)8 << 30;      // all slices of a call together; beyond: KO before any launch
constexpr uint64_t SAT = ~0ull;                      // a saturated count
constexpr uint64_t MAX_TABLE_PATHS = 0xFFFFFFFEull;  // positions within a table are 32-bit
constexpr uint32_t TPB = 256;

__host__ __device__ inline uint64_t sat_add(uint64_t a, uint64_t b) {
  const uint64_t s = a + b;
  return s < a ? SAT : s;
}
// counts that other lanes of the same launch wrote (the batch kernel peels level after level in one workgroup)
__device__ inline uint64_t ld64(const uint64_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void st64(uint64_t* p, uint64_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// cnt[s] and the prefixes of its arcs; the count of every successor is final
__device__ inline void count_state(const uint32_t* __restrict__ off, const wfst_tr* __restrict__ arcs, const float* __restrict__ fin,
                                   uint32_t s, uint64_t* cnt, uint64_t* __restrict__ pre) {
  uint64_t run = fin[s] != INF ? 1u : 0u;
  for (uint32_t i = off[s]; i < off[s + 1]; ++i) {
    pre[i] = run;
    run = sat_add(run, ld64(&cnt[arcs[i].nextstate]));
  }
  st64(&cnt[s], run);
}

// ---------------------------------------------------------------- step 1, device-wide
// one level of the search from the start: the states of queue[lo, hi) mark and queue their unmarked successors
__global__ void __launch_bounds__(TPB) paths_search_level_kernel(const uint32_t* __restrict__ off, const wfst_tr* __restrict__ arcs,
                                                                 uint32_t* mark, uint32_t* queue, uint32_t lo, uint32_t hi,
                                                                 uint32_t* tail) {
  for (uint32_t k = lo + blockIdx.x * TPB + threadIdx.x; k < hi; k += gridDim.x * TPB) {
    const uint32_t s = queue[k];
    for (uint32_t i = off[s]; i < off[s + 1]; ++i) {
      const uint32_t t = arcs[i].nextstate;
      if (ld(&mark[t]) == 0u && atomicExch(&mark[t], 1u) == 0u) queue[atomicAdd(tail, 1u)] = t;
    }
  }
}
__global__ void __launch_bounds__(TPB) paths_transpose_kernel(const uint32_t* __restrict__ off, const wfst_tr* __restrict__ arcs,
                                                              uint32_t n, const uint32_t* __restrict__ roff, uint32_t* cursor,
                                                              uint32_t* __restrict__ rsrc) {
  transpose_fill(off, arcs, n, roff, cursor, rsrc, blockIdx.x * TPB + threadIdx.x, gridDim.x * TPB);
}
// the accessible states queue[0, A): arcs left to wait for, and the sinks as the first level of the peel
__global__ void __launch_bounds__(TPB) paths_peel_init_kernel(const uint32_t* __restrict__ off, const uint32_t* __restrict__ queue,
                                                              uint32_t A, uint32_t* __restrict__ rem, uint32_t* lq, uint32_t* tail) {
  for (uint32_t k = blockIdx.x * TPB + threadIdx.x; k < A; k += gridDim.x * TPB) {
    const uint32_t s = queue[k], d = off[s + 1] - off[s];
    rem[s] = d;
    if (d == 0u) lq[atomicAdd(tail, 1u)] = s;
  }
}
// one level of the peel: the states of lq[lo, hi) are counted; an accessible predecessor whose last arc this settles is queued
__global__ void __launch_bounds__(TPB) paths_peel_level_kernel(const uint32_t* __restrict__ off, const wfst_tr* __restrict__ arcs,
                                                               const float* __restrict__ fin, const uint32_t* __restrict__ roff,
                                                               const uint32_t* __restrict__ rsrc, const uint32_t* __restrict__ mark,
                                                               uint32_t* rem, uint32_t* lq, uint32_t lo, uint32_t hi, uint32_t* tail,
                                                               uint64_t* cnt, uint64_t* __restrict__ pre) {
  for (uint32_t k = lo + blockIdx.x * TPB + threadIdx.x; k < hi; k += gridDim.x * TPB) {
    const uint32_t s = lq[k];
    count_state(off, arcs, fin, s, cnt, pre);
    for (uint32_t j = roff[s]; j < roff[s + 1]; ++j) {
      const uint32_t p = rsrc[j];
      if (mark[p] && atomicSub(&rem[p], 1u) == 1u) lq[atomicAdd(tail, 1u)] = p;
    }
  }
}

struct Counted {
  DBuf<uint64_t> cnt, pre;  // (empty without a start state)
  uint64_t paths = 0;
  uint32_t levels = 0;
};

uint32_t grid_for(const wfst_ctx* ctx, uint64_t items) {
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((items + TPB - 1) / TPB, (uint64_t)ctx->n_cus * 8));
}

[[noreturn]] void throw_cyclic() {
  throw Error("paths: a cycle is accessible from the start state: the reference's paths_iter never returns");
}

// step 1 of one FST of any size (on the device already); throws on an accessible cycle
Counted count_single(wfst_ctx* ctx, const wfst_fst* f, uint64_t& launches) {
  Counted r;
  if (f->start < 0 || f->n_states == 0) return r;
  if (f->n_arcs >= 0xFFFFFFFEull) throw Error("paths: input too large (arc positions are 32-bit)");
  hipStream_t st = ctx->stream;
  DevicePool& pool = *ctx->pool;
  const uint32_t n = f->n_states, E = (uint32_t)f->n_arcs, start = (uint32_t)f->start;
  const DeviceCsr& d = f->dev;
  // words: [0] tail of the search queue, [1] tail of the peel queue
  DBuf<uint32_t> tails(pool, 2), mark(pool, n), queue(pool, n), lq(pool, n), rem(pool, n), roff(pool, (size_t)n + 1),
      cursor(pool, (size_t)n + 1), rsrc(pool, E);
  r.cnt = DBuf<uint64_t>(pool, n);
  r.pre = DBuf<uint64_t>(pool, E);
  HIP_CHECK(hipMemsetAsync(mark.p, 0, (size_t)n * sizeof(uint32_t), st));
  HIP_CHECK(hipMemsetAsync(cursor.p, 0, ((size_t)n + 1) * sizeof(uint32_t), st));
  const uint32_t seed[3] = {1u, 0u, start};  // tails, and the queue's first entry
  HIP_CHECK(hipMemcpyAsync(tails.p, seed, 2 * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  HIP_CHECK(hipMemcpyAsync(queue.p, seed + 2, sizeof(uint32_t), hipMemcpyHostToDevice, st));
  HIP_CHECK(hipMemcpyAsync(mark.p + start, seed, sizeof(uint32_t), hipMemcpyHostToDevice, st));
  // the transpose (queued ahead of the search: nothing of it waits for the host)
  count_indegrees(ctx, d.arcs, E, cursor.p);
  auto scan_scratch = exclusive_scan_u32(ctx, cursor.p, roff.p, (size_t)n + 1);
  HIP_CHECK(hipMemsetAsync(cursor.p, 0, ((size_t)n + 1) * sizeof(uint32_t), st));
  launches += E ? 2 : 1;
  if (E) {
    paths_transpose_kernel<<<grid_for(ctx, (uint64_t)n * 16), TPB, 0, st>>>(d.offsets, d.arcs, n, roff.p, cursor.p, rsrc.p);
    HIP_CHECK(hipGetLastError());
    launches += 1;
  }
  // the search
  uint32_t lo = 0, hi = 1;
  while (lo < hi) {
    paths_search_level_kernel<<<grid_for(ctx, hi - lo), TPB, 0, st>>>(d.offsets, d.arcs, mark.p, queue.p, lo, hi, tails.p);
    HIP_CHECK(hipGetLastError());
    launches += 1;
    const uint32_t t = read_u32(ctx, tails.p);
    if (t < hi || t > n) throw Error("paths: internal error: the search queue ran past the states");
    lo = hi;
    hi = t;
  }
  const uint32_t A = hi;
  // the peel
  paths_peel_init_kernel<<<grid_for(ctx, A), TPB, 0, st>>>(d.offsets, queue.p, A, rem.p, lq.p, tails.p + 1);
  HIP_CHECK(hipGetLastError());
  launches += 1;
  lo = 0;
  hi = read_u32(ctx, tails.p + 1);
  while (lo < hi) {
    if (hi > A) throw Error("paths: internal error: the peel queue ran past the accessible states");
    paths_peel_level_kernel<<<grid_for(ctx, hi - lo), TPB, 0, st>>>(d.offsets, d.arcs, d.finals, roff.p, rsrc.p, mark.p, rem.p, lq.p,
                                                                     lo, hi, tails.p + 1, r.cnt.p, r.pre.p);
    HIP_CHECK(hipGetLastError());
    launches += 1;
    r.levels += 1;
    const uint32_t t = read_u32(ctx, tails.p + 1);
    lo = hi;
    hi = t;
  }
  if (hi != A) throw_cyclic();  // (hi < A: accessible states wait for a state that is never peeled)
  HIP_CHECK(hipMemcpyAsync(&r.paths, r.cnt.p + start, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  return r;
}

// ---------------------------------------------------------------- step 1, one workgroup per item
enum : uint32_t { PB_RUNNING = 0, PB_DONE = 1, PB_BAD_ITEM = 2 };
struct PbCtl {  // one per item, at the head of the slab; read back once
  uint32_t exit, cyclic, levels, pad;
  uint64_t paths;
};
struct PbItem {
  const uint32_t* off;
  const wfst_tr* arcs;
  const float* fin;
  uint32_t n, E, start;
  PbCtl* ctl;
  // the slice
  uint32_t* mark;   // [n] accessible from the start
  uint32_t* queue;  // [n] the accessible states
  uint32_t* lq;     // [n] the peel's levels, one after the other
  uint32_t* rem;    // [n] arcs whose destination is not counted yet
  uint32_t* roff;   // [n + 1] transpose
  uint32_t* rcnt;   // [n + 1]
  uint32_t* rsrc;   // [E]
  uint64_t* cnt;    // [n]
  uint64_t* pre;    // [E]
};

__global__ void __launch_bounds__(MB_TPB) paths_count_batch_kernel(const PbItem* __restrict__ items) {
  __shared__ uint32_t part[MB_TPB + 1];
  __shared__ uint32_t q[3], lv[3], s_bad;
  const PbItem it = items[blockIdx.x];
  const uint32_t tid = threadIdx.x;
  const uint32_t n = it.n, E = it.E;
  if (n == 0 || n > PB_MAX_STATES || E > PB_MAX_ARCS || it.start >= n) {  // (before any index is made of them)
    if (tid == 0) it.ctl->exit = PB_BAD_ITEM;
    return;
  }
  if (tid == 0) s_bad = 0u;
  __syncthreads();
  for (uint32_t i = tid; i < E; i += MB_TPB)
    if (it.arcs[i].nextstate >= n) s_bad = 1u;
  for (uint32_t s = tid; s <= n; s += MB_TPB) {
    const uint32_t o = it.off[s];
    if (o > E || (s == n ? o != E : it.off[s + 1] < o)) s_bad = 1u;
    if (s < n) it.mark[s] = 0u;
  }
  wg_bar();
  if (s_bad) {
    if (tid == 0) it.ctl->exit = PB_BAD_ITEM;
    return;
  }
  // ---- accessible from the start
  if (tid == 0) {
    stg(&it.mark[it.start], 1u);
    stg(&it.queue[0], it.start);
    q[2] = 1u;
  }
  wg_bar();
  wg_search(it.off, it.arcs, nullptr, it.mark, it.queue, q);
  const uint32_t A = q[2];
  wg_transpose(it.off, it.arcs, n, E, it.roff, it.rcnt, it.rsrc, part);
  // ---- the peel: sinks first
  if (tid == 0) lv[2] = 0u;
  __syncthreads();
  for (uint32_t k = tid; k < A; k += MB_TPB) {
    const uint32_t s = ld(&it.queue[k]), d = it.off[s + 1] - it.off[s];
    stg(&it.rem[s], d);
    if (d == 0u) stg(&it.lq[atomicAdd(&lv[2], 1u)], s);
  }
  wg_bar();
  if (tid == 0) {
    lv[0] = 0u;
    lv[1] = lv[2];
  }
  __syncthreads();
  uint32_t levels = 0;
  for (;;) {
    const uint32_t lo = lv[0], hi = lv[1];
    if (lo == hi) break;
    for (uint32_t k = lo + tid; k < hi; k += MB_TPB) {
      const uint32_t s = ld(&it.lq[k]);
      count_state(it.off, it.arcs, it.fin, s, it.cnt, it.pre);
      for (uint32_t j = ld(&it.roff[s]); j < ld(&it.roff[s + 1]); ++j) {
        const uint32_t p = ld(&it.rsrc[j]);
        if (ld(&it.mark[p]) && atomicSub(&it.rem[p], 1u) == 1u) stg(&it.lq[atomicAdd(&lv[2], 1u)], p);
      }
    }
    wg_bar();
    levels += 1;
    if (tid == 0) {
      lv[0] = hi;
      lv[1] = lv[2];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const bool cyclic = lv[2] != A;
    it.ctl->cyclic = cyclic ? 1u : 0u;
    it.ctl->levels = levels;
    it.ctl->paths = cyclic ? 0u : ld64(&it.cnt[it.start]);
    it.ctl->exit = PB_DONE;
  }
}

size_t carve_paths_slice(Slab s, uint32_t n, uint32_t E, PbItem* it) {
  PbItem v{};
  v.mark = s.take<uint32_t>(n);
  v.queue = s.take<uint32_t>(n);
  v.lq = s.take<uint32_t>(n);
  v.rem = s.take<uint32_t>(n);
  v.roff = s.take<uint32_t>((size_t)n + 1);
  v.rcnt = s.take<uint32_t>((size_t)n + 1);
  v.rsrc = s.take<uint32_t>(E);
  v.cnt = s.take<uint64_t>(n);
  v.pre = s.take<uint64_t>(E);
  v.n = n;
  v.E = E;
  if (it) *it = v;  // (the input's side is the caller's)
  return s.at();
}

// ---------------------------------------------------------------- steps 2-4: grids over all paths of all items
struct PathItem {  // what a walk needs of its item
  const uint32_t* off;
  const wfst_tr* arcs;
  const float* fin;
  const uint64_t* pre;
  uint32_t start, n;
  uint64_t base;  // the item's first path among the call's, in (item, depth-first rank) order
};
struct Walked {
  uint32_t arcs, nil, nol;
  float weight;
};
// path `r` of the item in depth-first order; EMIT: the non-epsilon labels go to il / ol
template <bool EMIT>
__device__ inline Walked walk_path(const PathItem& it, uint64_t r, uint32_t* __restrict__ il, uint32_t* __restrict__ ol) {
  Walked w{0u, 0u, 0u, 0.0f};
  uint32_t s = it.start;
  while (w.arcs < it.n) {  // (a path of an acyclic FST has fewer arcs than the FST has states)
    const uint32_t b = it.off[s], e = it.off[s + 1];
    if ((r == 0 && it.fin[s] != INF) || b == e) break;
    uint32_t lo = b, hi = e;  // the last arc with pre <= r: pre[b] <= r holds, the final's 1 included
    while (hi - lo > 1u) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (it.pre[mid] <= r)
        lo = mid;
      else
        hi = mid;
    }
    const wfst_tr a = it.arcs[lo];
    r -= it.pre[lo];
    w.weight = wtimes(w.weight, a.weight);
    w.arcs += 1;
    if (a.ilabel != WFST_EPS_LABEL) {
      if (EMIT) il[w.nil] = a.ilabel;
      w.nil += 1;
    }
    if (a.olabel != WFST_EPS_LABEL) {
      if (EMIT) ol[w.nol] = a.olabel;
      w.nol += 1;
    }
    s = a.nextstate;
  }
  w.weight = wtimes(w.weight, it.fin[s]);
  return w;
}
// the last item whose base is <= g (items without paths share their successor's base)
__device__ inline uint32_t item_of(const PathItem* __restrict__ items, uint32_t n_items, uint64_t g) {
  uint32_t lo = 0, hi = n_items;
  while (hi - lo > 1u) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (items[mid].base <= g)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(TPB) paths_measure_kernel(const PathItem* __restrict__ items, uint32_t n_items, uint32_t P,
                                                            uint64_t* __restrict__ key, uint32_t* __restrict__ val,
                                                            uint32_t* __restrict__ nil, uint32_t* __restrict__ nol, uint32_t* max_arcs) {
  const uint64_t g = (uint64_t)blockIdx.x * TPB + threadIdx.x;
  if (g >= P) return;
  const uint32_t i = item_of(items, n_items, g);
  const PathItem it = items[i];
  const Walked w = walk_path<false>(it, g - it.base, nullptr, nullptr);
  key[g] = ((uint64_t)i << 32) | w.arcs;
  val[g] = (uint32_t)g;
  nil[g] = w.nil;
  nol[g] = w.nol;
  atomicMax(max_arcs, w.arcs);
}
// the label counts in final order, as the 64-bit words the scans take (entry P: 0)
__global__ void __launch_bounds__(TPB) paths_gather_counts_kernel(const uint32_t* __restrict__ perm, const uint32_t* __restrict__ nil,
                                                                  const uint32_t* __restrict__ nol, uint32_t P,
                                                                  uint64_t* __restrict__ cil, uint64_t* __restrict__ col) {
  const uint64_t k = (uint64_t)blockIdx.x * TPB + threadIdx.x;
  if (k > P) return;
  cil[k] = k < P ? nil[perm[k]] : 0u;
  col[k] = k < P ? nol[perm[k]] : 0u;
}
__global__ void __launch_bounds__(TPB) paths_emit_kernel(const PathItem* __restrict__ items, uint32_t n_items, uint32_t P,
                                                         const uint32_t* __restrict__ perm, const uint64_t* __restrict__ iloff,
                                                         const uint64_t* __restrict__ oloff, uint32_t* __restrict__ il,
                                                         uint32_t* __restrict__ ol, float* __restrict__ weights) {
  const uint64_t k = (uint64_t)blockIdx.x * TPB + threadIdx.x;
  if (k >= P) return;
  const uint64_t g = perm[k];
  const PathItem it = items[item_of(items, n_items, g)];
  const Walked w = walk_path<true>(it, g - it.base, il + iloff[k], ol + oloff[k]);
  weights[k] = w.weight;
}

void exclusive_scan_u64(wfst_ctx* ctx, const uint64_t* in, uint64_t* out, size_t count, DBuf<uint8_t>& temp) {
  size_t bytes = 0;
  HIP_CHECK(rocprim::exclusive_scan(nullptr, bytes, in, out, (uint64_t)0, count, rocprim::plus<uint64_t>(), ctx->stream));
  temp = DBuf<uint8_t>(*ctx->pool, bytes);
  HIP_CHECK(rocprim::exclusive_scan(temp.p, bytes, in, out, (uint64_t)0, count, rocprim::plus<uint64_t>(), ctx->stream));
}

// one item's count against the caller's bound (the table is not begun before every item has passed)
void check_count(wfst_ctx* ctx, uint64_t paths, uint64_t max_paths) {
  PathsCounters& c = ctx->paths;
  if (paths == SAT) c.saturated += 1;
  c.paths = sat_add(c.paths, paths);
  if (paths > max_paths || paths == SAT)  // (one text for both; a saturated count is its N = UINT64_MAX, and says so behind it)
    throw Error("paths: the FST has " + std::to_string(paths) + " paths, more than max_paths (" + std::to_string(max_paths) + ")" +
                (paths == SAT ? ": the count is saturated" : ""));
}

// steps 2-4 over the counted items (items[i].base not yet set; counts[i] paths each)
wfst_paths* build_table(wfst_ctx* ctx, std::vector<PathItem>& items, const std::vector<uint64_t>& counts) {
  PathsCounters& c = ctx->paths;
  hipStream_t st = ctx->stream;
  DevicePool& pool = *ctx->pool;
  const size_t n_items = items.size();
  std::unique_ptr<wfst_paths> t(new wfst_paths);
  t->pool = ctx->pool;
  t->device = ctx->device;
  t->item_off.assign(n_items + 1, 0);
  for (size_t i = 0; i < n_items; ++i) {
    items[i].base = t->item_off[i];
    if (counts[i] > MAX_TABLE_PATHS - t->item_off[i])  // (asked before the sum: a count near 2^64 would wrap it)
      throw Error("paths: the table would hold more than " + std::to_string(MAX_TABLE_PATHS) + " paths: split the list");
    t->item_off[i + 1] = t->item_off[i] + counts[i];
  }
  const uint32_t P = (uint32_t)t->item_off[n_items];
  t->n_paths = P;
  if (P == 0) return t.release();  // (no device arrays: paths_download writes the two lone offsets itself)
  t->iloff = DBuf<uint64_t>(pool, (size_t)P + 1);
  t->oloff = DBuf<uint64_t>(pool, (size_t)P + 1);
  if (n_items > 0xFFFFFFFFull) throw Error("paths: the list is too long");
  t->weights = DBuf<float>(pool, P);
  DBuf<PathItem> d_items(pool, n_items);
  DBuf<uint64_t> key(pool, P), key_sorted(pool, P), cil(pool, (size_t)P + 1), col(pool, (size_t)P + 1);
  DBuf<uint32_t> val(pool, P), perm(pool, P), nil(pool, P), nol(pool, P), max_arcs(pool, 1);
  HIP_CHECK(hipMemcpyAsync(d_items.p, items.data(), n_items * sizeof(PathItem), hipMemcpyHostToDevice, st));
  HIP_CHECK(hipMemsetAsync(max_arcs.p, 0, sizeof(uint32_t), st));
  const uint32_t blocks = (uint32_t)(((uint64_t)P + TPB - 1) / TPB), blocks1 = (uint32_t)(((uint64_t)P + 1 + TPB - 1) / TPB);
  // ---- 2. unrank
  paths_measure_kernel<<<blocks, TPB, 0, st>>>(d_items.p, (uint32_t)n_items, P, key.p, val.p, nil.p, nol.p, max_arcs.p);
  HIP_CHECK(hipGetLastError());
  // ---- 3. reorder: stable, so equal (item, arc count) keep their depth-first rank order
  unsigned end_bit = 32;
  while (end_bit < 64 && (n_items - 1) >> (end_bit - 32)) ++end_bit;
  size_t sort_bytes = 0;
  HIP_CHECK(rocprim::radix_sort_pairs(nullptr, sort_bytes, key.p, key_sorted.p, val.p, perm.p, (size_t)P, 0u, end_bit, st));
  DBuf<uint8_t> sort_temp(pool, sort_bytes);
  HIP_CHECK(rocprim::radix_sort_pairs(sort_temp.p, sort_bytes, key.p, key_sorted.p, val.p, perm.p, (size_t)P, 0u, end_bit, st));
  // ---- 4. emit
  paths_gather_counts_kernel<<<blocks1, TPB, 0, st>>>(perm.p, nil.p, nol.p, P, cil.p, col.p);
  HIP_CHECK(hipGetLastError());
  DBuf<uint8_t> scan_temp_i, scan_temp_o;
  exclusive_scan_u64(ctx, cil.p, t->iloff.p, (size_t)P + 1, scan_temp_i);
  exclusive_scan_u64(ctx, col.p, t->oloff.p, (size_t)P + 1, scan_temp_o);
  uint64_t totals[2] = {0, 0};
  uint32_t deepest = 0;
  HIP_CHECK(hipMemcpyAsync(&totals[0], t->iloff.p + P, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(&totals[1], t->oloff.p + P, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(&deepest, max_arcs.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  t->n_il = totals[0];
  t->n_ol = totals[1];
  t->il = DBuf<uint32_t>(pool, t->n_il);
  t->ol = DBuf<uint32_t>(pool, t->n_ol);
  paths_emit_kernel<<<blocks, TPB, 0, st>>>(d_items.p, (uint32_t)n_items, P, perm.p, t->iloff.p, t->oloff.p, t->il.p, t->ol.p,
                                            t->weights.p);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(st));  // (the scratch above goes back to the pool behind this)
  c.launches += 6;  // measure, sort, gather, two scans, emit
  c.max_path_arcs = deepest;
  return t.release();
}

void check_owned(const wfst_ctx* ctx, const wfst_fst* f, const char* op) {
  if (f->device != ctx->device) throw Error(std::string(op) + ": the FST lives on another device");
  if (f->ctx != ctx) throw Error(std::string(op) + ": the FST belongs to another context");
}

struct Src {  // the three arrays of an item on the device
  const uint32_t* off;
  const wfst_tr* arcs;
  const float* fin;
};
PathItem path_item(const wfst_fst* f, const Src& s, const uint64_t* pre) {
  return PathItem{s.off, s.arcs, s.fin, pre, f->start < 0 ? 0u : (uint32_t)f->start, f->n_states, 0};
}
Src device_arrays(const wfst_fst* f) { return Src{f->dev.offsets, f->dev.arcs, f->dev.finals}; }

}  // namespace

uint64_t count_paths_fst(wfst_ctx* ctx, const wfst_fst* f) {
  check_owned(ctx, f, "count_paths");
  ensure_device(const_cast<wfst_fst*>(f));
  PathsCounters& c = ctx->paths;
  c.items_single = 1;
  const Counted r = count_single(ctx, f, c.launches);
  c.levels = r.levels;
  c.paths = r.paths;
  c.saturated = r.paths == SAT ? 1 : 0;
  return r.paths;
}

wfst_paths* paths_fst(wfst_ctx* ctx, const wfst_fst* f, uint64_t max_paths) {
  check_owned(ctx, f, "paths");
  ensure_device(const_cast<wfst_fst*>(f));
  PathsCounters& c = ctx->paths;
  c.items_single = 1;
  const Counted r = count_single(ctx, f, c.launches);
  c.levels = r.levels;
  check_count(ctx, r.paths, max_paths);
  std::vector<PathItem> items{path_item(f, device_arrays(f), r.pre.p)};
  return build_table(ctx, items, {r.paths});
}

wfst_paths* paths_batch(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, uint64_t max_paths, uint8_t* in_kernel) {
  check_items_owned(ctx, fsts, n, "paths_batch");
  PathsCounters& c = ctx->paths;
  hipStream_t st = ctx->stream;
  enum : uint8_t { KERNEL, EMPTY, SINGLE };
  std::vector<uint8_t> kind(n);
  std::vector<size_t> run;  // the items that occupy a workgroup
  for (size_t i = 0; i < n; ++i) {
    const wfst_fst* f = fsts[i];
    kind[i] = (f->start < 0 || f->n_states == 0) ? EMPTY
              : (f->n_states <= PB_MAX_STATES && f->n_arcs <= PB_MAX_ARCS) ? KERNEL : SINGLE;
    if (kind[i] != EMPTY) ensure_device(const_cast<wfst_fst*>(f));  // (a host-resident handle is uploaded and keeps the copy)
    if (kind[i] == KERNEL) run.push_back(i);
  }
  std::vector<Src> src(n, Src{nullptr, nullptr, nullptr});
  for (size_t i = 0; i < n; ++i)
    if (kind[i] != EMPTY) src[i] = device_arrays(fsts[i]);
  std::vector<PbCtl> ctl(n);
  std::vector<const uint64_t*> pre(n, nullptr);
  auto carve = [&](size_t i, Slab s, PbItem* it) {
    const wfst_fst* f = fsts[i];
    const size_t end = carve_paths_slice(s, f->n_states, (uint32_t)f->n_arcs, it);
    if (it) {
      it->off = src[i].off;
      it->arcs = src[i].arcs;
      it->fin = src[i].fin;
      it->start = (uint32_t)f->start;
    }
    return end;
  };
  auto launch = [&](const PbItem* d_items, uint32_t m) { paths_count_batch_kernel<<<m, MB_TPB, 0, st>>>(d_items); };
  auto classify = [&](size_t i, const PbCtl& k, const PbItem& it) {
    if (k.exit != PB_DONE)
      throw Error("paths_batch: internal error: the kernel left item " + std::to_string(i) + " with exit code " + std::to_string(k.exit));
    ctl[i] = k;
    pre[i] = it.pre;
    return BatchExit::FINISHED;
  };
  BatchStats bs;
  const auto slabs = batch_launch_loop<PbItem, PbCtl>(ctx, bs, {"paths_batch", 1, nullptr, PB_MAX_SLAB, "call"}, std::move(run), carve,
                                                      nullptr, launch, classify);
  c.launches += bs.launches;
  // in index order, so that the first KO is the lowest failing index
  std::vector<Counted> singles;
  std::vector<PathItem> items(n);
  std::vector<uint64_t> counts(n, 0);
  singles.reserve(n);
  for (size_t i = 0; i < n; ++i) {
    const wfst_fst* f = fsts[i];
    try {
      if (kind[i] == SINGLE) {
        singles.push_back(count_single(ctx, f, c.launches));
        const Counted& r = singles.back();
        c.items_single += 1;
        c.levels = std::max<uint64_t>(c.levels, r.levels);
        counts[i] = r.paths;
        pre[i] = r.pre.p;
      } else {
        c.items_in_kernel += 1;
        if (kind[i] == KERNEL) {
          if (ctl[i].cyclic) throw_cyclic();
          c.levels = std::max<uint64_t>(c.levels, ctl[i].levels);
          counts[i] = ctl[i].paths;
        }
      }
      check_count(ctx, counts[i], max_paths);
    } catch (const std::exception& e) {
      throw Error("item " + std::to_string(i) + ": " + e.what());
    }
    items[i] = path_item(f, src[i], pre[i]);
  }
  wfst_paths* t = build_table(ctx, items, counts);
  if (in_kernel)
    for (size_t i = 0; i < n; ++i) in_kernel[i] = kind[i] == SINGLE ? 0 : 1;
  return t;
}

void paths_download(wfst_ctx* ctx, const wfst_paths* t, uint64_t* item_off, float* weights, uint64_t* ilabel_off, uint32_t* ilabels,
                    uint64_t* olabel_off, uint32_t* olabels) {
  if (t->device != ctx->device) throw Error("paths_download: the table lives on another device");
  hipStream_t st = ctx->stream;
  if (item_off) std::copy(t->item_off.begin(), t->item_off.end(), item_off);
  const size_t P = t->n_paths;
  if (P == 0) {
    if (ilabel_off) ilabel_off[0] = 0;
    if (olabel_off) olabel_off[0] = 0;
    return;
  }
  if (weights) HIP_CHECK(hipMemcpyAsync(weights, t->weights.p, P * sizeof(float), hipMemcpyDeviceToHost, st));
  if (ilabel_off) HIP_CHECK(hipMemcpyAsync(ilabel_off, t->iloff.p, (P + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  if (olabel_off) HIP_CHECK(hipMemcpyAsync(olabel_off, t->oloff.p, (P + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  if (ilabels && t->n_il) HIP_CHECK(hipMemcpyAsync(ilabels, t->il.p, t->n_il * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  if (olabels && t->n_ol) HIP_CHECK(hipMemcpyAsync(olabels, t->ol.p, t->n_ol * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
}

}  // namespace wfst
