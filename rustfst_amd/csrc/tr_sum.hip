// tr_sum.hip — tr_sum(fst) and tr_unique(fst) on the device: a NEW handle, the input is left as it is.
// Reference: rustfst/src/algorithms/tr_sum.rs:7-22 with sum_trs_unchecked (fst_impls/vector_fst/mutable_fst.rs:380-405),
// tr_unique.rs:8-51 with unique_trs_unchecked (:358-377).  Per state both do a STABLE sort by tr_compare — the key
// (ilabel, olabel, nextstate), compared unsigned, the weight not in it — and then
//   tr_sum     the first arc of a run of equal keys survives; its weight is folded with plus_assign over the run in
//              sorted order (tropical: `if rhs < self { self = rhs }`, tropical_weight.rs:53-58: a tie keeps the earlier
//              arc's bits, NaN never replaces).  The fold is NOT associative once a NaN sits inside a run
//              (a + (NaN + c) = a, (a + NaN) + c = a + c), so it is done serially, by the lane of the run's head.
//   tr_unique  Vec::dedup on Tr's ==: an arc goes when its key equals that of the last KEPT arc and its weight is equal
//              under TropicalWeight's PartialEq, which is the KDELTA approximation (semiring.rs:161-168).  A chain along
//              the run, walked serially by the lane of the run's head as well.
// Passes (every arc is read as one 16-byte record; 16 lanes own one state, so a chunk of 16 arcs is one 256-byte line):
//   sort   states with <= RANK_MAX arcs: rank sort on the key extended by the arc's position (tr_sort.hip's scheme with
//          the full key): one register per lane up to 16 arcs, chunks of 16 beyond.  Larger states are listed.
//   big    the listed states: two stable rocPRIM segmented radix passes over exactly those segments, least significant
//          part first (nextstate, then ilabel:olabel), carrying the arc's index; then a gather.
//   flag   over the sorted arcs: keep[p] (head of a run / survivor of the chain), survivors per state
//   scan   one rocPRIM exclusive scan of the counts = the new offsets
//   write  survivors to their place (a 16-lane ballot prefix per chunk); tr_sum folds the run's weights on the way
// The list forms (wfst_tr_sum_batch / wfst_tr_unique_batch) run the same passes in ONE workgroup per item
// (tr_sum_batch_kernel below), with a workgroup scan in place of the device-wide one and no radix sort: an item with a
// state beyond RANK_MAX arcs goes through tr_sum_fst.
#include <algorithm>
#include <cstring>

#include <rocprim/device/device_segmented_radix_sort.hpp>

#pragma clang fp contract(off)  // (before tropical.h comes in: its functions compile without contraction here too)

#include "batch_driver.h"
#include "common.h"
#include "fst_props.h"
#include "wg_ops.h"

namespace wfst {
namespace {

constexpr int GROUP = 16;
constexpr uint32_t RANK_MAX = 256;
constexpr uint32_t TPB = 256;

// the key as two words: (ilabel, olabel) and (nextstate, position)
__device__ __forceinline__ uint64_t key_lo(const wfst_tr& a) { return ((uint64_t)a.ilabel << 32) | a.olabel; }
__device__ __forceinline__ uint64_t key_hi(const wfst_tr& a, uint32_t pos) { return ((uint64_t)a.nextstate << 32) | pos; }
__device__ __forceinline__ bool key_less(uint64_t lo_a, uint64_t hi_a, uint64_t lo_b, uint64_t hi_b) {
  return lo_a < lo_b || (lo_a == lo_b && hi_a < hi_b);
}
__device__ __forceinline__ bool same_key(const wfst_tr& a, const wfst_tr& b) {
  return a.ilabel == b.ilabel && a.olabel == b.olabel && a.nextstate == b.nextstate;
}

// The per-state bodies of the sort, flag and write passes: 16 lanes (lane gl of its group) own one state.  The single call's
// kernels stride over the states of one FST with a whole grid, tr_sum_batch_kernel over those of its item with one workgroup.

// the arcs [b, b + deg) of a state of at most RANK_MAX arcs in (ilabel, olabel, nextstate, position) order into `out`
__device__ __forceinline__ void rank_sort_state(const wfst_tr* __restrict__ in, wfst_tr* __restrict__ out, uint32_t b, uint32_t deg,
                                                uint32_t gl) {
  if (deg <= GROUP) {  // the whole state lives in one register per lane
    const bool live = gl < deg;
    wfst_tr a{};
    if (live) a = in[b + gl];
    const uint64_t lo = key_lo(a), hi = key_hi(a, gl);
    uint32_t rank = 0;
#pragma unroll
    for (int t = 0; t < GROUP; ++t) {
      const uint64_t lo_t = __shfl(lo, t, GROUP), hi_t = __shfl(hi, t, GROUP);
      rank += ((uint32_t)t < deg) && key_less(lo_t, hi_t, lo, hi);
    }
    if (live) out[b + rank] = a;
    return;
  }
  for (uint32_t i0 = 0; i0 < deg; i0 += GROUP) {
    const bool live = i0 + gl < deg;
    wfst_tr a{};
    if (live) a = in[b + i0 + gl];
    const uint64_t lo = key_lo(a), hi = key_hi(a, i0 + gl);
    uint32_t rank = 0;
    for (uint32_t j0 = 0; j0 < deg; j0 += GROUP) {
      wfst_tr o{};
      if (j0 + gl < deg) o = in[b + j0 + gl];
      const uint64_t lo_j = key_lo(o), hi_j = key_hi(o, j0 + gl);
#pragma unroll
      for (int t = 0; t < GROUP; ++t) {
        const uint64_t lo_t = __shfl(lo_j, t, GROUP), hi_t = __shfl(hi_j, t, GROUP);
        rank += (j0 + (uint32_t)t < deg) && key_less(lo_t, hi_t, lo, hi);
      }
    }
    if (live) out[b + rank] = a;
  }
}

// keep[p] of the sorted arcs [b, e) of a state; returns its survivors (to every lane of the group)
__device__ __forceinline__ uint32_t flag_state(const wfst_tr* __restrict__ sorted, uint8_t* __restrict__ keep, uint32_t b, uint32_t e,
                                               int unique, uint32_t gl) {
  uint32_t k = 0;
  for (uint32_t p = b + gl; p < e; p += GROUP) {
    const wfst_tr a = sorted[p];
    const bool head = p == b || !same_key(sorted[p - 1], a);
    if (!unique) {
      keep[p] = head ? 1 : 0;
      k += head;
    } else if (head) {  // dedup: compare with the last KEPT arc of the run
      keep[p] = 1;
      ++k;
      float last = a.weight;
      for (uint32_t q = p + 1; q < e; ++q) {
        const wfst_tr c = sorted[q];
        if (!same_key(a, c)) break;
        const bool stay = !weq(last, c.weight);
        keep[q] = stay ? 1 : 0;
        if (stay) {
          last = c.weight;
          ++k;
        }
      }
    }
  }
  for (int d = GROUP / 2; d >= 1; d >>= 1) k += __shfl_xor(k, d, GROUP);
  return k;
}

// the survivors of the sorted arcs [b, e) of a state to out[base ..], in order; tr_sum: the head folds the weights of its
// run.  shift: the group's first lane in its wave
__device__ __forceinline__ void write_state(const wfst_tr* __restrict__ sorted, const uint8_t* __restrict__ keep, uint32_t b,
                                            uint32_t e, uint32_t base, int unique, uint32_t gl, uint32_t shift,
                                            wfst_tr* __restrict__ out) {
  for (uint32_t p0 = b; p0 < e; p0 += GROUP) {  // (uniform over the group)
    const uint32_t p = p0 + gl;
    const bool kp = p < e && keep[p] != 0;
    const uint32_t m = (uint32_t)(__ballot(kp) >> shift) & 0xFFFFu;
    if (kp) {
      wfst_tr a = sorted[p];
      if (!unique)
        for (uint32_t q = p + 1; q < e && keep[q] == 0; ++q) {
          const float w = sorted[q].weight;
          if (w < a.weight) a.weight = w;  // plus_assign
        }
      out[base + __popc(m & ((1u << gl) - 1u))] = a;
    }
    base += __popc(m);
  }
}

// one 16-lane group per state: the state's arcs in key order into `out`; states beyond RANK_MAX arcs are listed
__global__ __launch_bounds__(TPB) void trsum_sort_kernel(const uint32_t* __restrict__ offsets, const wfst_tr* __restrict__ in,
                                                         wfst_tr* __restrict__ out, uint32_t n_states,
                                                         uint32_t* __restrict__ big_list, uint32_t* __restrict__ big_count) {
  const uint32_t gl = threadIdx.x & (GROUP - 1);
  const uint32_t groups = (gridDim.x * blockDim.x) / GROUP;
  for (uint32_t s = (blockIdx.x * blockDim.x + threadIdx.x) / GROUP; s < n_states; s += groups) {
    const uint32_t b = offsets[s], e = offsets[s + 1], deg = e - b;
    if (deg > RANK_MAX) {
      if (gl == 0) big_list[atomicAdd(big_count, 1u)] = s;
      continue;
    }
    rank_sort_state(in, out, b, deg, gl);
  }
}

// big states only, one workgroup per state.  Pass 1 sorts the arc indices on nextstate, pass 2 on (ilabel, olabel):
// both stable, so equal keys stay in stored order.
__global__ __launch_bounds__(TPB) void trsum_bigkeys1_kernel(const uint32_t* __restrict__ offsets, const wfst_tr* __restrict__ in,
                                                             const uint32_t* __restrict__ big_list, uint32_t n_big,
                                                             uint32_t* __restrict__ keys, uint32_t* __restrict__ idx,
                                                             uint32_t* __restrict__ seg_begin, uint32_t* __restrict__ seg_end) {
  for (uint32_t i = blockIdx.x; i < n_big; i += gridDim.x) {
    const uint32_t s = big_list[i], b = offsets[s], e = offsets[s + 1];
    if (threadIdx.x == 0) {
      seg_begin[i] = b;
      seg_end[i] = e;
    }
    for (uint32_t p = b + threadIdx.x; p < e; p += blockDim.x) {
      keys[p] = in[p].nextstate;
      idx[p] = p;
    }
  }
}
__global__ __launch_bounds__(TPB) void trsum_bigkeys2_kernel(const uint32_t* __restrict__ offsets, const wfst_tr* __restrict__ in,
                                                             const uint32_t* __restrict__ big_list, uint32_t n_big,
                                                             const uint32_t* __restrict__ idx, uint64_t* __restrict__ keys) {
  for (uint32_t i = blockIdx.x; i < n_big; i += gridDim.x) {
    const uint32_t s = big_list[i], b = offsets[s], e = offsets[s + 1];
    for (uint32_t p = b + threadIdx.x; p < e; p += blockDim.x) keys[p] = key_lo(in[idx[p]]);
  }
}
__global__ __launch_bounds__(TPB) void trsum_biggather_kernel(const uint32_t* __restrict__ offsets, const wfst_tr* __restrict__ in,
                                                              wfst_tr* __restrict__ out, const uint32_t* __restrict__ big_list,
                                                              uint32_t n_big, const uint32_t* __restrict__ idx) {
  for (uint32_t i = blockIdx.x; i < n_big; i += gridDim.x) {
    const uint32_t s = big_list[i], b = offsets[s], e = offsets[s + 1];
    for (uint32_t p = b + threadIdx.x; p < e; p += blockDim.x) out[p] = in[idx[p]];
  }
}

// keep[p] of the sorted arcs and the survivors per state (cnt[n_states] = 0 closes the scan)
__global__ __launch_bounds__(TPB) void trsum_flag_kernel(const uint32_t* __restrict__ offsets, const wfst_tr* __restrict__ sorted,
                                                         uint32_t n_states, int unique, uint8_t* __restrict__ keep,
                                                         uint32_t* __restrict__ cnt) {
  const uint32_t gl = threadIdx.x & (GROUP - 1);
  const uint32_t groups = (gridDim.x * blockDim.x) / GROUP;
  for (uint32_t s = (blockIdx.x * blockDim.x + threadIdx.x) / GROUP; s <= n_states; s += groups) {
    if (s == n_states) {
      if (gl == 0) cnt[s] = 0;
      continue;
    }
    const uint32_t k = flag_state(sorted, keep, offsets[s], offsets[s + 1], unique, gl);
    if (gl == 0) cnt[s] = k;
  }
}

// survivors to off_out[s] + (survivors before them in the state); tr_sum: the head folds the weights of its run
__global__ __launch_bounds__(TPB) void trsum_write_kernel(const uint32_t* __restrict__ offsets, const wfst_tr* __restrict__ sorted,
                                                          const uint8_t* __restrict__ keep, uint32_t n_states, int unique,
                                                          const uint32_t* __restrict__ off_out, wfst_tr* __restrict__ out) {
  const uint32_t gl = threadIdx.x & (GROUP - 1);
  const uint32_t shift = threadIdx.x & 63u & ~(uint32_t)(GROUP - 1);  // the group's first lane in its wave
  const uint32_t groups = (gridDim.x * blockDim.x) / GROUP;
  for (uint32_t s = (blockIdx.x * blockDim.x + threadIdx.x) / GROUP; s < n_states; s += groups)
    write_state(sorted, keep, offsets[s], offsets[s + 1], off_out[s], unique, gl, shift, out);
}

}  // namespace

uint64_t tr_sum_props(uint64_t in, bool unique, bool no_states) {
  using namespace props;
  uint64_t out = in & ALL & ARCSORT_MASK & DELETE_ARCS_MASK;
  if (!unique) out &= WEIGHT_INVARIANT;
  if (no_states) out |= NULL_PROPS;
  return out;
}

wfst_fst* tr_sum_fst(wfst_ctx* ctx, const wfst_fst* f, bool unique) {
  ensure_device(const_cast<wfst_fst*>(f));
  hipStream_t st = ctx->stream;
  DevicePool& pool = *ctx->pool;
  const uint32_t n = f->n_states;
  const uint64_t E = f->n_arcs;
  const uint64_t out_props = tr_sum_props(f->props, unique, n == 0);
  if (n == 0) {
    HostCsr hc;
    hc.offsets.push_back(0);
    return make_host_fst(ctx, 0, f->start, out_props, std::move(hc));
  }
  if (E <= 1) return adopt_device(ctx, n, E, f->start, out_props, f->dev.offsets, f->dev.arcs, f->dev.finals);
  if (E >= (1ull << 32)) throw Error(unique ? "tr_unique: input too large" : "tr_sum: input too large");

  DBuf<wfst_tr> sorted(pool, E);
  DBuf<uint32_t> big_list(pool, n), big_count(pool, 1);
  HIP_CHECK(hipMemsetAsync(big_count.p, 0, sizeof(uint32_t), st));
  const uint32_t blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(((uint64_t)n * GROUP + TPB - 1) / TPB, (uint64_t)ctx->n_cus * 32));
  trsum_sort_kernel<<<blocks, TPB, 0, st>>>(f->dev.offsets, f->dev.arcs, sorted.p, n, big_list.p, big_count.p);
  HIP_CHECK(hipGetLastError());
  const uint32_t n_big = read_u32(ctx, big_count.p);
  if (n_big) {
    DBuf<uint32_t> k1(pool, E), k1_out(pool, E), idx(pool, E), idx1(pool, E), idx2(pool, E), seg_b(pool, n_big), seg_e(pool, n_big);
    DBuf<uint64_t> k2(pool, E), k2_out(pool, E);
    const uint32_t bblocks = std::min<uint32_t>(n_big, (uint32_t)ctx->n_cus * 8);
    trsum_bigkeys1_kernel<<<bblocks, TPB, 0, st>>>(f->dev.offsets, f->dev.arcs, big_list.p, n_big, k1.p, idx.p, seg_b.p, seg_e.p);
    HIP_CHECK(hipGetLastError());
    size_t t1 = 0, t2 = 0;
    HIP_CHECK(rocprim::segmented_radix_sort_pairs(nullptr, t1, k1.p, k1_out.p, idx.p, idx1.p, (unsigned)E, n_big, seg_b.p, seg_e.p,
                                                  0u, 32u, st));
    HIP_CHECK(rocprim::segmented_radix_sort_pairs(nullptr, t2, k2.p, k2_out.p, idx1.p, idx2.p, (unsigned)E, n_big, seg_b.p, seg_e.p,
                                                  0u, 64u, st));
    DBuf<uint8_t> temp(pool, std::max(t1, t2));
    HIP_CHECK(rocprim::segmented_radix_sort_pairs(temp.p, t1, k1.p, k1_out.p, idx.p, idx1.p, (unsigned)E, n_big, seg_b.p, seg_e.p,
                                                  0u, 32u, st));
    trsum_bigkeys2_kernel<<<bblocks, TPB, 0, st>>>(f->dev.offsets, f->dev.arcs, big_list.p, n_big, idx1.p, k2.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(rocprim::segmented_radix_sort_pairs(temp.p, t2, k2.p, k2_out.p, idx1.p, idx2.p, (unsigned)E, n_big, seg_b.p, seg_e.p,
                                                  0u, 64u, st));
    trsum_biggather_kernel<<<bblocks, TPB, 0, st>>>(f->dev.offsets, f->dev.arcs, sorted.p, big_list.p, n_big, idx2.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(st));  // the sort buffers go back to the pool
  }
  DBuf<uint8_t> keep(pool, E);
  DBuf<uint32_t> cnt(pool, (size_t)n + 1), off_out(pool, (size_t)n + 1);
  trsum_flag_kernel<<<blocks, TPB, 0, st>>>(f->dev.offsets, sorted.p, n, unique ? 1 : 0, keep.p, cnt.p);
  HIP_CHECK(hipGetLastError());
  const DBuf<uint8_t> scan_tmp = exclusive_scan_u32(ctx, cnt.p, off_out.p, (size_t)n + 1);
  const uint32_t e_out = read_u32(ctx, off_out.p + n);
  DBuf<wfst_tr> arcs_out(pool, e_out);
  trsum_write_kernel<<<blocks, TPB, 0, st>>>(f->dev.offsets, sorted.p, keep.p, n, unique ? 1 : 0, off_out.p, arcs_out.p);
  HIP_CHECK(hipGetLastError());
  return adopt_device(ctx, n, e_out, f->start, out_props, off_out.p, arcs_out.p, f->dev.finals);
}

// ================================================================ batch (wfst_tr_sum_batch / wfst_tr_unique_batch)
namespace {

constexpr uint32_t TB_MAX_STATES = 4096;  // the in_kernel rule (include/wfst.h); its third condition is RANK_MAX
constexpr uint32_t TB_MAX_ARCS = 16384;
constexpr size_t TB_MAX_SLAB = (size_t)8 << 30;  // all slices of a call together; beyond: KO before any launch
enum : uint32_t { TB_RUNNING = 0, TB_DONE = 1, TB_SINGLE_WIDE = 2 };  // TbCtl::exit

struct TbCtl {  // one per item, at the head of the slab; read back once
  uint32_t exit;
  uint32_t e_out;
  uint32_t pad[2];
};
struct TbItem {
  const uint32_t* off;
  const wfst_tr* arcs;
  uint32_t n, unique;
  TbCtl* ctl;
  // the slice
  wfst_tr* sorted;    // [E] every state's arcs in key order
  uint8_t* keep;      // [E] the arc survives
  uint32_t* cnt;      // [n + 1] survivors per state
  uint32_t* off_out;  // [n + 1] the result
  wfst_tr* arcs_out;  // [E]
};

// one workgroup per item: the passes of tr_sum_fst (sort, flag, scan, write) over the same per-state functions, a barrier
// between them
__global__ void __launch_bounds__(MB_TPB) tr_sum_batch_kernel(const TbItem* __restrict__ items) {
  __shared__ uint32_t part[MB_TPB + 1];
  __shared__ uint32_t s_wide;
  const TbItem it = items[blockIdx.x];
  const uint32_t tid = threadIdx.x, gl = tid & (GROUP - 1);
  const uint32_t shift = tid & 63u & ~(uint32_t)(GROUP - 1);  // the group's first lane in its wave
  const uint32_t n = it.n;
  const int unique = (int)it.unique;
  // ---- 0. a state beyond the rank sort: the single call's business
  if (tid == 0) s_wide = 0;
  __syncthreads();
  for (uint32_t s = tid; s < n; s += MB_TPB)
    if (it.off[s + 1] - it.off[s] > RANK_MAX) s_wide = 1u;
  __syncthreads();
  if (s_wide) {
    if (tid == 0) it.ctl->exit = TB_SINGLE_WIDE;
    return;
  }
  // ---- 1. rank sort on (ilabel, olabel, nextstate, position), 16 lanes per state
  for (uint32_t s = tid >> 4; s < n; s += MB_TPB >> 4) rank_sort_state(it.arcs, it.sorted, it.off[s], it.off[s + 1] - it.off[s], gl);
  wg_bar();
  // ---- 2. keep[p] of the sorted arcs and the survivors per state; cnt[n] = 0 closes the scan
  for (uint32_t s = tid >> 4; s <= n; s += MB_TPB >> 4) {
    const uint32_t k = s < n ? flag_state(it.sorted, it.keep, it.off[s], it.off[s + 1], unique, gl) : 0u;
    if (gl == 0) it.cnt[s] = k;
  }
  wg_bar();
  // ---- 3. the new offsets
  const uint32_t e_out = wg_exclusive_scan(it.cnt, it.off_out, n + 1, part);
  // ---- 4. survivors to their place; tr_sum: the head folds the weights of its run
  for (uint32_t s = tid >> 4; s < n; s += MB_TPB >> 4)
    write_state(it.sorted, it.keep, it.off[s], it.off[s + 1], ld(&it.off_out[s]), unique, gl, shift, it.arcs_out);
  if (tid == 0) {
    it.ctl->e_out = e_out;
    it.ctl->exit = TB_DONE;
  }
}

// carves one item's arrays out of the slab; it == nullptr only measures
size_t carve_tr_sum_slice(Slab s, uint32_t n, uint32_t E, TbItem* it) {
  TbItem v{};
  v.sorted = s.take<wfst_tr>(E);
  v.keep = s.take<uint8_t>(E);
  v.cnt = s.take<uint32_t>((size_t)n + 1);
  v.off_out = s.take<uint32_t>((size_t)n + 1);
  v.arcs_out = s.take<wfst_tr>(E);
  v.n = n;
  if (it) *it = v;  // (the input's side is the caller's)
  return s.at();
}

}  // namespace

// the host loop is batch_driver.h's, with the ownership check, one pass (the result never has more arcs than the input:
// nothing grows) and a slab limit per call
void tr_sum_batch(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, bool unique, wfst_fst** outs, uint8_t* in_kernel) {
  ctx->trsum_batch = {};
  check_items_owned(ctx, fsts, n, unique ? "tr_unique_batch" : "tr_sum_batch");
  hipStream_t st = ctx->stream;
  enum : uint8_t { KERNEL, TRIVIAL, SINGLE };
  struct Ran {
    uint32_t e_out = 0;
    const uint32_t* off = nullptr;
    const wfst_tr* arcs = nullptr;
  };
  std::vector<uint8_t> kind(n);
  std::vector<Ran> ran(n);
  std::vector<size_t> run;  // the items that occupy a workgroup
  for (size_t i = 0; i < n; ++i) {
    const wfst_fst* f = fsts[i];
    // without states or with at most one arc: tr_sum_fst's own early answers (no launch)
    kind[i] = (f->n_states == 0 || f->n_arcs <= 1) ? TRIVIAL
              : (f->n_states <= TB_MAX_STATES && f->n_arcs <= TB_MAX_ARCS) ? KERNEL : SINGLE;
    if (kind[i] == KERNEL) {
      ensure_device(const_cast<wfst_fst*>(f));
      run.push_back(i);
    }
  }
  auto carve = [&](size_t i, Slab s, TbItem* it) {
    const wfst_fst* f = fsts[i];
    const size_t end = carve_tr_sum_slice(s, f->n_states, (uint32_t)f->n_arcs, it);
    if (it) {
      it->off = f->dev.offsets;
      it->arcs = f->dev.arcs;
      it->unique = unique ? 1u : 0u;
    }
    return end;
  };
  auto launch = [&](const TbItem* d_items, uint32_t m) { tr_sum_batch_kernel<<<m, MB_TPB, 0, st>>>(d_items); };
  auto classify = [&](size_t i, const TbCtl& c, const TbItem& it) {
    if (c.exit == TB_SINGLE_WIDE) {
      kind[i] = SINGLE;
      return BatchExit::SINGLE;
    }
    if (c.exit != TB_DONE || c.e_out > fsts[i]->n_arcs)
      throw Error(std::string(unique ? "tr_unique_batch" : "tr_sum_batch") + ": the kernel left item " + std::to_string(i) +
                  " with exit code " + std::to_string(c.exit));
    ran[i] = Ran{c.e_out, it.off_out, it.arcs_out};
    return BatchExit::FINISHED;
  };
  const auto slabs = batch_launch_loop<TbItem, TbCtl>(ctx, ctx->trsum_batch,
                                                      {unique ? "tr_unique_batch" : "tr_sum_batch", 1, nullptr, TB_MAX_SLAB, "call"},
                                                      std::move(run), carve, nullptr, launch, classify);
  auto outcome = [&](size_t i) {
    const wfst_fst* f = fsts[i];
    if (kind[i] == SINGLE) return BatchOutcome::single();
    if (kind[i] == TRIVIAL) return BatchOutcome::handle(tr_sum_fst(ctx, f, unique));
    return BatchOutcome::adopt({f->n_states, ran[i].e_out, f->start, tr_sum_props(f->props, unique, false), ran[i].off, ran[i].arcs,
                                f->dev.finals});
  };
  batch_finish(ctx, ctx->trsum_batch, n, outs, in_kernel, outcome, [&](size_t i) { return tr_sum_fst(ctx, fsts[i], unique); });
}

}  // namespace wfst
