// isomorphic.hip — isomorphic_with_config on the device: a verdict (or the reference's error) for two handles, both left as
// they are.  Reference: rustfst/src/algorithms/isomorphic.rs:22-48 (tr_compare), :64-73 (pair_state), :75-132
// (ismorphic_state), :134-158 (the FIFO search).
//
// The reference pops pairs (s1, s2) from a queue; per pair it compares final weights and arc counts, sorts both arc lists by
// tr_compare and walks them index by index: labels, approx_equal weights, pair_state(next1, next2) — the first pairing of a
// state of fst1 wins and queues the pair — and only then the non-determinism mark (arc i and arc i - 1 of fst1 agree in
// labels and approx-equal weight).  The first failure ends the search: an error naming the pair if a mark was set before it
// in sequential order, else false.  Here the same search runs level by level:
//   set-up   a sorted copy of each operand's arcs in tr_compare order, offsets unchanged (tr_sum.hip's scheme: 16 lanes per
//            state rank-sort up to ISO_RANK_MAX arcs on the four-part key, larger states by three stable segmented radix
//            passes, least significant part first, and a gather); pair[s1] = all ones (unpaired), the start pair at
//            position 0.
//   events   a level is the queue of its pairs in order.  Arc slot i of queue entry q has the position
//            e = 1 + (arc slots of all entries before it, over all levels) + i: the order in which the reference would reach
//            it.  A failure in front of the walk (finals, counts) sits at the position of the pair's slot 0.
//   check    per pair: the first static failure (finals, counts, labels, weights) goes by atomicMin of (e << 32 | q) into the
//            level's failure word; every slot in front of it emits atomicMin(&pair[next1], e << 32 | next2) and, where it
//            agrees with its predecessor, atomicMin(mark, e) into a word that lives for the whole call.
//   resolve  per emitted slot: the winner of pair[next1] names another next2: a pairing failure at e; it carries this e: the
//            state is newly paired.
//   compact  the newly paired slots in slot order are the next queue.
// The verdict of a level with a failure: the least (e, q); KO iff mark < e (strictly: the mark of the failing slot itself
// is set by `check` although the reference never reaches it), else 0.  A slot behind the failure has a larger position: it
// cannot win an atomicMin against an earlier one nor lower the minimum, so nothing is undone.
// Two regimes, as in top_sort.hip: NARROW = one workgroup runs level after level inside one launch, queue, offsets and flags
// in LDS, until a level exceeds ISOMORPHIC_NARROW_PAIRS pairs or ISOMORPHIC_NARROW_EVENTS slots or the search ends; WIDE =
// one device-wide launch per phase and level, one control block read per level.  WFST_ISOMORPHIC_PATH=narrow|wide pins one
// (narrow then keeps what does not fit LDS in the call's global scratch).  In both a pair whose fst1 state has
// ISOMORPHIC_WAVE_ARCS arcs or more is walked by its whole wave.  Every route gives the same verdict and message.
#include <algorithm>
#include <string>

#include <rocprim/device/device_segmented_radix_sort.hpp>

#include "common.h"
#include "fst_props.h"

namespace wfst {
namespace {

constexpr uint32_t BLOCK = 256;  // threads per workgroup of every kernel here
constexpr uint32_t WAVE = 64;
constexpr uint32_t GROUP = 16;          // lanes per state of the rank sort
constexpr uint32_t ISO_RANK_MAX = 256;  // arcs up to which a state is rank-sorted
// the narrow limits: 2 x 256 queue entries of 8 B, 257 + 256 offset / count words and 2048 flag words are 15 KB of LDS
constexpr uint32_t ISOMORPHIC_NARROW_PAIRS = 256;    // a level of at most this many pairs ..
constexpr uint32_t ISOMORPHIC_NARROW_EVENTS = 2048;  // .. and at most this many arc slots runs in the one-workgroup kernel
constexpr uint32_t ISOMORPHIC_WAVE_ARCS = 64;        // arcs from which a pair is walked by its wave
static_assert(ISOMORPHIC_NARROW_PAIRS == WFST_ISOMORPHIC_NARROW_PAIRS && ISOMORPHIC_NARROW_EVENTS == WFST_ISOMORPHIC_NARROW_EVENTS,
              "include/wfst.h states the same limits");
constexpr unsigned long long NO_FAIL = ~0ull;

// ---------------------------------------------------------------- the sorted copies
// OrderedFloat's total order as a u32: -0.0 == +0.0, every NaN one key above +inf's
__device__ __forceinline__ uint32_t weight_key(float w) {
  if (w != w) return 0xFFFFFFFFu;
  return f32_key(w == 0.0f ? 0.0f : w);
}
__device__ __forceinline__ uint64_t key_hi(const wfst_tr& a) { return ((uint64_t)a.ilabel << 32) | a.olabel; }
__device__ __forceinline__ uint64_t key_lo(const wfst_tr& a) { return ((uint64_t)weight_key(a.weight) << 32) | a.nextstate; }

// one 16-lane group per state: rank = arcs before this one by (key, position); states beyond ISO_RANK_MAX arcs are listed
__global__ __launch_bounds__(BLOCK) void iso_sort_kernel(const uint32_t* __restrict__ offsets, const wfst_tr* __restrict__ in,
                                                         wfst_tr* __restrict__ out, uint32_t n_states, uint32_t* __restrict__ big_list,
                                                         uint32_t* __restrict__ big_count) {
  const uint32_t gl = threadIdx.x & (GROUP - 1);
  const uint32_t groups = (gridDim.x * blockDim.x) / GROUP;
  for (uint32_t s = (blockIdx.x * blockDim.x + threadIdx.x) / GROUP; s < n_states; s += groups) {
    const uint32_t b = offsets[s], deg = offsets[s + 1] - b;
    if (deg > ISO_RANK_MAX) {
      if (gl == 0) big_list[atomicAdd(big_count, 1u)] = s;
      continue;
    }
    for (uint32_t i0 = 0; i0 < deg; i0 += GROUP) {
      const uint32_t pos = i0 + gl;
      const bool live = pos < deg;
      wfst_tr a{};
      if (live) a = in[b + pos];
      const uint64_t hi = key_hi(a), lo = key_lo(a);
      uint32_t rank = 0;
      for (uint32_t j0 = 0; j0 < deg; j0 += GROUP) {
        uint64_t hj = 0, lj = 0;
        if (j0 + gl < deg) {
          const wfst_tr o = in[b + j0 + gl];
          hj = key_hi(o), lj = key_lo(o);
        }
#pragma unroll
        for (uint32_t t = 0; t < GROUP; ++t) {
          const uint64_t h = __shfl(hj, (int)t, GROUP), l = __shfl(lj, (int)t, GROUP);
          const uint32_t pj = j0 + t;
          rank += pj < deg && (h < hi || (h == hi && (l < lo || (l == lo && pj < pos))));
        }
      }
      if (live) out[b + rank] = a;
    }
  }
}
// big states only, one workgroup per state and turn.  part 0: nextstate and the identity permutation, 1: the weight key,
// 2: ilabel:olabel — each of the arcs in the order the pass before left them
__global__ __launch_bounds__(BLOCK) void iso_bigkeys_kernel(const uint32_t* __restrict__ offsets, const wfst_tr* __restrict__ in,
                                                            const uint32_t* __restrict__ big_list, uint32_t n_big, int part,
                                                            uint32_t* __restrict__ idx, uint32_t* __restrict__ k32,
                                                            uint64_t* __restrict__ k64, uint32_t* __restrict__ seg_begin,
                                                            uint32_t* __restrict__ seg_end) {
  for (uint32_t i = blockIdx.x; i < n_big; i += gridDim.x) {
    const uint32_t s = big_list[i], b = offsets[s], e = offsets[s + 1];
    if (part == 0 && threadIdx.x == 0) seg_begin[i] = b, seg_end[i] = e;
    for (uint32_t p = b + threadIdx.x; p < e; p += blockDim.x) {
      if (part == 0) {
        idx[p] = p;
        k32[p] = in[p].nextstate;
      } else if (part == 1) {
        k32[p] = weight_key(in[idx[p]].weight);
      } else {
        k64[p] = key_hi(in[idx[p]]);
      }
    }
  }
}
__global__ __launch_bounds__(BLOCK) void iso_biggather_kernel(const uint32_t* __restrict__ offsets, const wfst_tr* __restrict__ in,
                                                              wfst_tr* __restrict__ out, const uint32_t* __restrict__ big_list,
                                                              uint32_t n_big, const uint32_t* __restrict__ idx) {
  for (uint32_t i = blockIdx.x; i < n_big; i += gridDim.x) {
    const uint32_t s = big_list[i], b = offsets[s], e = offsets[s + 1];
    for (uint32_t p = b + threadIdx.x; p < e; p += blockDim.x) out[p] = in[idx[p]];
  }
}

// ---------------------------------------------------------------- the search
struct Iso {
  const uint32_t* off1;  // [n1 + 1], [n2 + 1] the operands' offsets
  const uint32_t* off2;
  const wfst_tr* a1;  // their arcs in tr_compare order
  const wfst_tr* a2;
  const float* fin1;
  const float* fin2;
  unsigned long long* pair;  // [n1] (position << 32 | state of fst2), all ones = unpaired; atomics and agent-scope loads only
  uint32_t* cnt;             // [0] the mark word (least position of a mark), [1] pairs walked by a wave, [2] marks made
  float delta;
};
// the control block the host reads: one per narrow launch, one per wide level
enum : uint32_t {
  CTL_FAIL = 0,    // (and 1) the level's least failure, position << 32 | queue entry; all ones = none
  CTL_STATUS = 2,  // ISO_*
  CTL_W = 3,       // pairs of the level that runs next
  CTL_T = 4,       // its arc slots
  CTL_E0 = 5,      // position of its slot 0
  CTL_LEVELS = 6,  // narrow: levels this launch ran, the widest of them, their pairs and slots
  CTL_MAXW = 7,
  CTL_PAIRS = 8,
  CTL_EVENTS = 9,
  CTL_FS1 = 10,  // the failing pair
  CTL_FS2 = 11,
  CTL_PARITY = 12,  // which of the two queues holds the level that runs next
  CTL_WORDS = 16
};
enum : uint32_t { ISO_NEXT = 0, ISO_DONE = 1, ISO_FAILED = 2 };

// the largest q in [0, hi] with base[q] <= j (base ascending, base[0] = 0): behind a run of pairs without arcs, the owner
__device__ __forceinline__ uint32_t entry_of(const uint32_t* base, uint32_t hi, uint32_t j) {
  uint32_t lo = 0;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo + 1) / 2;
    if (base[mid] <= j)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}
__device__ __forceinline__ bool slot_agrees(const wfst_tr& x, const wfst_tr& y, float delta) {
  return x.ilabel == y.ilabel && x.olabel == y.olabel && approx_equal(x.weight, y.weight, delta);
}
// slot i of a pair, in front of its first static failure: the pairing event and the mark (row1 = the fst1 state's sorted arcs)
__device__ __forceinline__ void slot_emit(const Iso& g, const wfst_tr* __restrict__ row1, uint32_t i, const wfst_tr& x,
                                          const wfst_tr& y, uint32_t e) {
  atomicMin(&g.pair[x.nextstate], ((unsigned long long)e << 32) | y.nextstate);
  if (i > 0u && slot_agrees(x, row1[i - 1u], g.delta)) {
    atomicMin(&g.cnt[0], e);
    atomicAdd(&g.cnt[2], 1u);
  }
}
// `check` for queue entry q = (s1, s2), whose slot 0 has position e_base: every lane of the wave calls it (on: the lane has
// an entry).  nemit[q] = slots in front of the first static failure; the failure goes into *fail (LDS or global).
__device__ void iso_check(const Iso& g, uint32_t s1, uint32_t s2, bool on, uint32_t e_base, uint32_t q, uint32_t lane,
                          uint32_t* nemit, unsigned long long* fail) {
  uint32_t b1 = 0, b2 = 0, deg = 0;
  bool by_wave = false;
  if (on) {
    b1 = g.off1[s1], b2 = g.off2[s2];
    deg = g.off1[s1 + 1] - b1;
    const float f1 = g.fin1[s1], f2 = g.fin2[s2];  // +inf = not final (None)
    const bool fin_ok = (f1 == INF && f2 == INF) || (f1 != INF && f2 != INF && approx_equal(f1, f2, g.delta));
    if (!fin_ok || deg != g.off2[s2 + 1] - b2) {
      atomicMin(fail, ((unsigned long long)e_base << 32) | q);
      nemit[q] = 0u;
      on = false;
    }
    by_wave = on && deg >= ISOMORPHIC_WAVE_ARCS;
  }
  if (on && !by_wave) {
    uint32_t i = 0;
    for (; i < deg; ++i) {
      const wfst_tr x = g.a1[b1 + i], y = g.a2[b2 + i];
      if (!slot_agrees(x, y, g.delta)) {
        atomicMin(fail, ((unsigned long long)(e_base + i) << 32) | q);
        break;
      }
      slot_emit(g, g.a1 + b1, i, x, y, e_base + i);
    }
    nemit[q] = i;
  }
  for (unsigned long long m = __ballot(by_wave); m; m &= m - 1ull) {
    const int src = __ffsll((long long)m) - 1;
    const uint32_t wb1 = __shfl(b1, src), wb2 = __shfl(b2, src), wdeg = __shfl(deg, src), we = __shfl(e_base, src), wq = __shfl(q, src);
    uint32_t first = wdeg;  // the first slot that disagrees
    for (uint32_t i0 = 0; i0 < wdeg; i0 += WAVE) {
      const uint32_t i = i0 + lane;
      const bool in = i < wdeg;
      wfst_tr x{}, y{};
      if (in) x = g.a1[wb1 + i], y = g.a2[wb2 + i];
      const unsigned long long bad = __ballot(in && !slot_agrees(x, y, g.delta));
      const uint32_t lim = bad ? i0 + (uint32_t)__ffsll((long long)bad) - 1u : wdeg;
      if (in && i < lim) slot_emit(g, g.a1 + wb1, i, x, y, we + i);
      if (bad) {
        first = lim;
        break;
      }
    }
    if (lane == 0u) {
      if (first < wdeg) atomicMin(fail, ((unsigned long long)(we + first) << 32) | wq);
      nemit[wq] = first;
      atomicAdd(&g.cnt[1], 1u);
    }
  }
}
// `resolve` for slot `slot` of a level of w entries whose slot 0 has position e0: 1 = newly paired (then *np is the pair)
__device__ __forceinline__ uint32_t iso_resolve(const Iso& g, const uint2* queue, const uint32_t* base, const uint32_t* nemit, uint32_t w,
                                                uint32_t slot, uint32_t e0, unsigned long long* fail, uint2* np) {
  const uint32_t q = entry_of(base, w - 1u, slot), i = slot - base[q];
  if (i >= nemit[q]) return 0u;
  const uint2 pr = queue[q];
  const uint32_t n1 = g.a1[g.off1[pr.x] + i].nextstate, n2 = g.a2[g.off2[pr.y] + i].nextstate, e = e0 + slot;
  const unsigned long long win = __hip_atomic_load(&g.pair[n1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if ((uint32_t)win != n2) {
    if (fail) atomicMin(fail, ((unsigned long long)e << 32) | q);
    return 0u;
  }
  *np = make_uint2(n1, n2);
  return (uint32_t)(win >> 32) == e ? 1u : 0u;
}

// exclusive scan of one value per thread over the workgroup; part: 4 words of LDS
__device__ __forceinline__ uint32_t wg_scan_threads(uint32_t v, uint32_t* part, uint32_t* total) {
  const uint32_t lane = threadIdx.x & (WAVE - 1u), wv = threadIdx.x / WAVE;
  uint32_t x = v;
  for (uint32_t d = 1; d < WAVE; d <<= 1) {
    const uint32_t y = __shfl_up(x, d);
    if (lane >= d) x += y;
  }
  if (lane == WAVE - 1u) part[wv] = x;
  __syncthreads();
  uint32_t add = 0, sum = 0;
  for (uint32_t k = 0; k < BLOCK / WAVE; ++k) {
    if (k < wv) add += part[k];
    sum += part[k];
  }
  *total = sum;
  __syncthreads();  // part may be written again
  return add + x - v;
}

struct NarrowArgs {
  uint2* queue[2];   // [n1] each: the level that runs and the next one
  uint32_t* g_base;  // [n1 + 1], [n1 + 1], [E1 + 1]: where a level keeps what does not fit LDS (spill only)
  uint32_t* g_nemit;
  uint32_t* g_flag;
  uint32_t* ctl;
  uint32_t parity, w, e0;
  uint32_t spill;  // 1: never hand a level back for its size (WFST_ISOMORPHIC_PATH=narrow)
};
// NARROW: level after level from the w entries of queue[parity] on, until the search ends or (without spill) a level
// exceeds the narrow limits; leaves the control block
__global__ __launch_bounds__(BLOCK) void iso_narrow_kernel(const Iso g, const NarrowArgs a) {
  __shared__ uint2 s_queue[2][ISOMORPHIC_NARROW_PAIRS];
  __shared__ uint32_t s_base[ISOMORPHIC_NARROW_PAIRS + 1], s_nemit[ISOMORPHIC_NARROW_PAIRS], s_flag[ISOMORPHIC_NARROW_EVENTS];
  __shared__ unsigned long long s_fail;
  __shared__ uint32_t s_part[BLOCK / WAVE];
  const uint32_t tid = threadIdx.x, lane = tid & (WAVE - 1u);
  uint32_t w = a.w, e0 = a.e0, par = a.parity;
  bool in_lds = false;  // the running level's queue is (also) in s_queue[par]
  uint32_t levels = 0, maxw = 0, pairs = 0, events = 0, status = ISO_NEXT, T = 0;
  if (tid == 0) s_fail = NO_FAIL;
  __syncthreads();
  for (;;) {
    const bool small_w = w <= ISOMORPHIC_NARROW_PAIRS;
    const uint2* queue = in_lds ? s_queue[par] : a.queue[par];
    uint32_t* base = small_w ? s_base : a.g_base;
    uint32_t* nemit = small_w ? s_nemit : a.g_nemit;
    // ---- the slots of every entry: base[q] = arcs of the entries before q, base[w] = T
    const uint32_t chunk = (w + BLOCK - 1u) / BLOCK, cb = min(w, tid * chunk), ce = min(w, cb + chunk);
    uint32_t sum = 0;
    for (uint32_t q = cb; q < ce; ++q) {
      const uint32_t s1 = queue[q].x;
      sum += g.off1[s1 + 1] - g.off1[s1];
    }
    uint32_t run = wg_scan_threads(sum, s_part, &T);
    for (uint32_t q = cb; q < ce; ++q) {
      const uint32_t s1 = queue[q].x;
      base[q] = run;
      run += g.off1[s1 + 1] - g.off1[s1];
    }
    if (tid == 0) base[w] = T;
    if (!a.spill && (!small_w || T > ISOMORPHIC_NARROW_EVENTS)) break;  // the host runs this level WIDE
    uint32_t* flag = T <= ISOMORPHIC_NARROW_EVENTS ? s_flag : a.g_flag;
    __syncthreads();
    // ---- check
    for (uint32_t qb = tid & ~(WAVE - 1u); qb < w; qb += BLOCK) {
      const uint32_t q = qb + lane;
      const bool on = q < w;
      const uint2 pr = on ? queue[q] : make_uint2(0u, 0u);
      iso_check(g, pr.x, pr.y, on, e0 + (on ? base[q] : 0u), q, lane, nemit, &s_fail);
    }
    __syncthreads();
    // ---- resolve
    for (uint32_t slot = tid; slot < T; slot += BLOCK) {
      uint2 np;
      flag[slot] = iso_resolve(g, queue, base, nemit, w, slot, e0, &s_fail, &np);
    }
    __syncthreads();
    ++levels, pairs += w, events += T, maxw = max(maxw, w);
    const unsigned long long fail = s_fail;
    if (fail != NO_FAIL) {
      if (tid == 0) {
        const uint2 pr = queue[(uint32_t)fail];
        a.ctl[CTL_FAIL] = (uint32_t)fail, a.ctl[CTL_FAIL + 1] = (uint32_t)(fail >> 32);
        a.ctl[CTL_FS1] = pr.x, a.ctl[CTL_FS2] = pr.y;
      }
      status = ISO_FAILED;
      break;
    }
    // ---- compact: the newly paired slots, in slot order, are the next level
    const uint32_t fchunk = (T + BLOCK - 1u) / BLOCK, fb = min(T, tid * fchunk), fe = min(T, fb + fchunk);
    uint32_t mine = 0, nw = 0;
    for (uint32_t slot = fb; slot < fe; ++slot) mine += flag[slot];
    uint32_t pos = wg_scan_threads(mine, s_part, &nw);
    const bool next_in_lds = nw <= ISOMORPHIC_NARROW_PAIRS;
    for (uint32_t slot = fb; slot < fe; ++slot) {
      if (!flag[slot]) continue;
      uint2 np = make_uint2(0u, 0u);
      (void)iso_resolve(g, queue, base, nemit, w, slot, e0, nullptr, &np);
      a.queue[par ^ 1u][pos] = np;  // (the host's copy, should the next level go WIDE)
      if (next_in_lds) s_queue[par ^ 1u][pos] = np;
      ++pos;
    }
    __syncthreads();
    e0 += T, w = nw, par ^= 1u, in_lds = next_in_lds;
    if (w == 0u) {
      status = ISO_DONE;
      break;
    }
  }
  if (tid == 0) {
    a.ctl[CTL_STATUS] = status, a.ctl[CTL_W] = w, a.ctl[CTL_T] = T, a.ctl[CTL_E0] = e0, a.ctl[CTL_PARITY] = par;
    a.ctl[CTL_LEVELS] = levels, a.ctl[CTL_MAXW] = maxw, a.ctl[CTL_PAIRS] = pairs, a.ctl[CTL_EVENTS] = events;
  }
}

// the start pair at position 0, queue[0] of level 1, the words of the call
__global__ void iso_init_kernel(const Iso g, uint2* queue, uint32_t* ctl, uint32_t start1, uint32_t start2) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  g.pair[start1] = (unsigned long long)start2;
  queue[0] = make_uint2(start1, start2);
  g.cnt[0] = 0xFFFFFFFFu, g.cnt[1] = 0u, g.cnt[2] = 0u;
  for (uint32_t k = 0; k < CTL_WORDS; ++k) ctl[k] = 0u;
  ctl[CTL_FAIL] = ctl[CTL_FAIL + 1] = 0xFFFFFFFFu;
  ctl[CTL_W] = 1u, ctl[CTL_T] = g.off1[start1 + 1] - g.off1[start1], ctl[CTL_E0] = 1u;
}
// WIDE, one launch per phase.  deg[q] = arcs of entry q (deg[w] = 0 closes the scan); the next level's slot count restarts
__global__ __launch_bounds__(BLOCK) void iso_deg_kernel(const Iso g, const uint2* __restrict__ queue, uint32_t w, uint32_t* __restrict__ deg,
                                                        uint32_t* __restrict__ ctl) {
  if (blockIdx.x == 0 && threadIdx.x == 0) ctl[CTL_T] = 0u;
  for (uint32_t q = blockIdx.x * BLOCK + threadIdx.x; q <= w; q += gridDim.x * BLOCK) {
    uint32_t d = 0;
    if (q < w) {
      const uint32_t s1 = queue[q].x;
      d = g.off1[s1 + 1] - g.off1[s1];
    }
    deg[q] = d;
  }
}
__global__ __launch_bounds__(BLOCK) void iso_check_kernel(const Iso g, const uint2* __restrict__ queue, const uint32_t* __restrict__ base,
                                                          uint32_t* nemit, uint32_t w, uint32_t e0, uint32_t* ctl) {
  const uint32_t lane = threadIdx.x & (WAVE - 1u);
  for (uint32_t qb = blockIdx.x * BLOCK + (threadIdx.x & ~(WAVE - 1u)); qb < w; qb += gridDim.x * BLOCK) {
    const uint32_t q = qb + lane;
    const bool on = q < w;
    const uint2 pr = on ? queue[q] : make_uint2(0u, 0u);
    iso_check(g, pr.x, pr.y, on, e0 + (on ? base[q] : 0u), q, lane, nemit, reinterpret_cast<unsigned long long*>(ctl + CTL_FAIL));
  }
}
__global__ __launch_bounds__(BLOCK) void iso_resolve_kernel(const Iso g, const uint2* __restrict__ queue, const uint32_t* __restrict__ base,
                                                            const uint32_t* __restrict__ nemit, uint32_t w, uint32_t T, uint32_t e0,
                                                            uint32_t* __restrict__ flag, uint32_t* ctl) {
  for (uint32_t slot = blockIdx.x * BLOCK + threadIdx.x; slot <= T; slot += gridDim.x * BLOCK) {
    uint2 np;
    flag[slot] = slot < T ? iso_resolve(g, queue, base, nemit, w, slot, e0, reinterpret_cast<unsigned long long*>(ctl + CTL_FAIL), &np) : 0u;
  }
}
// pos = the exclusive scan of flag over T + 1 words: pos[T] newly paired states; the control block of the level
__global__ __launch_bounds__(BLOCK) void iso_compact_kernel(const Iso g, const uint2* __restrict__ queue, const uint32_t* __restrict__ base,
                                                            const uint32_t* __restrict__ nemit, uint32_t w, uint32_t T, uint32_t e0,
                                                            const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos,
                                                            uint2* __restrict__ next, uint32_t* ctl) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const unsigned long long fail = *reinterpret_cast<const unsigned long long*>(ctl + CTL_FAIL);
    ctl[CTL_W] = pos[T];
    ctl[CTL_E0] = e0 + T;
    ctl[CTL_STATUS] = fail != NO_FAIL ? ISO_FAILED : pos[T] == 0u ? ISO_DONE : ISO_NEXT;
    if (fail != NO_FAIL) {
      const uint2 pr = queue[(uint32_t)fail];
      ctl[CTL_FS1] = pr.x, ctl[CTL_FS2] = pr.y;
    }
  }
  for (uint32_t slot = blockIdx.x * BLOCK + threadIdx.x; slot < T; slot += gridDim.x * BLOCK) {
    if (!flag[slot]) continue;
    uint2 np = make_uint2(0u, 0u);
    (void)iso_resolve(g, queue, base, nemit, w, slot, e0, nullptr, &np);
    next[pos[slot]] = np;
    atomicAdd(&ctl[CTL_T], g.off1[np.x + 1] - g.off1[np.x]);
  }
}

// ---------------------------------------------------------------- the host side
uint32_t grid_for(const wfst_ctx* ctx, uint64_t items) {
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((items + BLOCK - 1) / BLOCK, (uint64_t)ctx->n_cus * 8));
}
void check_operand(wfst_ctx* ctx, const wfst_fst* f, const char* which) {
  if (f->device != ctx->device) throw Error(std::string("isomorphic: ") + which + " lives on another device");
  if (f->ctx != ctx) throw Error(std::string("isomorphic: ") + which + " belongs to another context");
}

// the arcs of f in tr_compare order per state; returns the states that took the radix route
uint64_t sort_operand(wfst_ctx* ctx, const wfst_fst* f, wfst_tr* sorted) {
  hipStream_t st = ctx->stream;
  DevicePool& pool = *ctx->pool;
  const uint32_t n = f->n_states;
  const uint64_t E = f->n_arcs;
  if (E == 0) return 0;
  DBuf<uint32_t> big_list(pool, n), big_count(pool, 1);
  HIP_CHECK(hipMemsetAsync(big_count.p, 0, sizeof(uint32_t), st));
  const uint32_t blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(((uint64_t)n * GROUP + BLOCK - 1) / BLOCK, (uint64_t)ctx->n_cus * 32));
  iso_sort_kernel<<<blocks, BLOCK, 0, st>>>(f->dev.offsets, f->dev.arcs, sorted, n, big_list.p, big_count.p);
  HIP_CHECK(hipGetLastError());
  const uint32_t n_big = read_u32(ctx, big_count.p);
  if (n_big) {
    DBuf<uint32_t> k32(pool, E), k32_out(pool, E), idx_a(pool, E), idx_b(pool, E), seg_b(pool, n_big), seg_e(pool, n_big);
    DBuf<uint64_t> k64(pool, E), k64_out(pool, E);
    const uint32_t bblocks = std::min<uint32_t>(n_big, (uint32_t)ctx->n_cus * 8);
    size_t t32 = 0, t64 = 0;
    HIP_CHECK(rocprim::segmented_radix_sort_pairs(nullptr, t32, k32.p, k32_out.p, idx_a.p, idx_b.p, (unsigned)E, n_big, seg_b.p, seg_e.p,
                                                  0u, 32u, st));
    HIP_CHECK(rocprim::segmented_radix_sort_pairs(nullptr, t64, k64.p, k64_out.p, idx_a.p, idx_b.p, (unsigned)E, n_big, seg_b.p, seg_e.p,
                                                  0u, 64u, st));
    DBuf<uint8_t> temp(pool, std::max(t32, t64));
    // nextstate: idx_a -> idx_b; the weight key: idx_b -> idx_a; ilabel:olabel: idx_a -> idx_b (stable passes)
    iso_bigkeys_kernel<<<bblocks, BLOCK, 0, st>>>(f->dev.offsets, f->dev.arcs, big_list.p, n_big, 0, idx_a.p, k32.p, k64.p, seg_b.p, seg_e.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(rocprim::segmented_radix_sort_pairs(temp.p, t32, k32.p, k32_out.p, idx_a.p, idx_b.p, (unsigned)E, n_big, seg_b.p, seg_e.p,
                                                  0u, 32u, st));
    iso_bigkeys_kernel<<<bblocks, BLOCK, 0, st>>>(f->dev.offsets, f->dev.arcs, big_list.p, n_big, 1, idx_b.p, k32.p, k64.p, seg_b.p, seg_e.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(rocprim::segmented_radix_sort_pairs(temp.p, t32, k32.p, k32_out.p, idx_b.p, idx_a.p, (unsigned)E, n_big, seg_b.p, seg_e.p,
                                                  0u, 32u, st));
    iso_bigkeys_kernel<<<bblocks, BLOCK, 0, st>>>(f->dev.offsets, f->dev.arcs, big_list.p, n_big, 2, idx_a.p, k32.p, k64.p, seg_b.p, seg_e.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(rocprim::segmented_radix_sort_pairs(temp.p, t64, k64.p, k64_out.p, idx_a.p, idx_b.p, (unsigned)E, n_big, seg_b.p, seg_e.p,
                                                  0u, 64u, st));
    iso_biggather_kernel<<<bblocks, BLOCK, 0, st>>>(f->dev.offsets, f->dev.arcs, sorted, big_list.p, n_big, idx_b.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(st));  // the sort buffers go back to the pool
  }
  return n_big;
}

}  // namespace

bool isomorphic_fsts(wfst_ctx* ctx, const wfst_fst* f1, const wfst_fst* f2, float delta) {
  check_operand(ctx, f1, "fst1");
  check_operand(ctx, f2, "fst2");
  const Path path = path_knob("WFST_ISOMORPHIC_PATH");
  ctx->isomorphic = wfst_ctx::IsomorphicCounters{};
  wfst_ctx::IsomorphicCounters& stats = ctx->isomorphic;
  if (f1->start < 0 && f2->start < 0) return true;   // (isomorphic.rs:136-138)
  if (f1->start < 0 || f2->start < 0) return false;  // (:141-143)
  if (f1->n_arcs >= 0xFFFFFFFEull || f2->n_arcs >= 0xFFFFFFFEull) throw Error("isomorphic: input too large: positions must fit in 32 bits");
  ensure_device(const_cast<wfst_fst*>(f1));
  ensure_device(const_cast<wfst_fst*>(f2));
  hipStream_t st = ctx->stream;
  DevicePool& pool = *ctx->pool;
  const uint32_t n1 = f1->n_states;
  const uint64_t E1 = f1->n_arcs;

  // ---- scratch of the call: every buffer goes back to the pool on every exit
  DBuf<wfst_tr> sorted1(pool, E1), sorted2(pool, f2->n_arcs);
  DBuf<unsigned long long> pair(pool, n1);
  DBuf<uint2> queue_a(pool, n1), queue_b(pool, n1);
  DBuf<uint32_t> base(pool, (size_t)n1 + 1), nemit(pool, (size_t)n1 + 1), flag(pool, E1 + 1), pos(pool, E1 + 1), cnt(pool, 4), ctl(pool, CTL_WORDS);
  stats.big_states_sorted = sort_operand(ctx, f1, sorted1.p) + sort_operand(ctx, f2, sorted2.p);
  HIP_CHECK(hipMemsetAsync(pair.p, 0xFF, (size_t)n1 * sizeof(unsigned long long), st));
  const Iso g{f1->dev.offsets, f2->dev.offsets, sorted1.p, sorted2.p, f1->dev.finals, f2->dev.finals, pair.p, cnt.p, delta};
  uint2* const queues[2] = {queue_a.p, queue_b.p};
  iso_init_kernel<<<1, 64, 0, st>>>(g, queues[0], ctl.p, (uint32_t)f1->start, (uint32_t)f2->start);
  HIP_CHECK(hipGetLastError());
  uint32_t h[CTL_WORDS];
  auto read_ctl = [&] {
    HIP_CHECK(hipMemcpyAsync(h, ctl.p, sizeof(h), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
  };
  read_ctl();
  uint32_t w = h[CTL_W], T = h[CTL_T], e0 = h[CTL_E0], parity = 0, status = ISO_NEXT;
  while (status == ISO_NEXT) {
    const bool fits = w <= ISOMORPHIC_NARROW_PAIRS && T <= ISOMORPHIC_NARROW_EVENTS;
    if (path == Path::Narrow || (path == Path::Auto && fits)) {
      const NarrowArgs a{{queues[0], queues[1]}, base.p, nemit.p, flag.p, ctl.p, parity, w, e0, path == Path::Narrow ? 1u : 0u};
      iso_narrow_kernel<<<1, BLOCK, 0, st>>>(g, a);
      HIP_CHECK(hipGetLastError());
      read_ctl();
      ++stats.narrow_launches;
      stats.narrow_levels += h[CTL_LEVELS], stats.levels += h[CTL_LEVELS];
      stats.pairs += h[CTL_PAIRS], stats.events += h[CTL_EVENTS];
      stats.max_level_width = std::max<uint64_t>(stats.max_level_width, h[CTL_MAXW]);
      parity = h[CTL_PARITY];
    } else {
      const uint2* queue = queues[parity];
      iso_deg_kernel<<<grid_for(ctx, (uint64_t)w + 1), BLOCK, 0, st>>>(g, queue, w, nemit.p, ctl.p);
      HIP_CHECK(hipGetLastError());
      const DBuf<uint8_t> scan1 = exclusive_scan_u32(ctx, nemit.p, base.p, (size_t)w + 1);
      iso_check_kernel<<<grid_for(ctx, w), BLOCK, 0, st>>>(g, queue, base.p, nemit.p, w, e0, ctl.p);
      HIP_CHECK(hipGetLastError());
      iso_resolve_kernel<<<grid_for(ctx, (uint64_t)T + 1), BLOCK, 0, st>>>(g, queue, base.p, nemit.p, w, T, e0, flag.p, ctl.p);
      HIP_CHECK(hipGetLastError());
      const DBuf<uint8_t> scan2 = exclusive_scan_u32(ctx, flag.p, pos.p, (size_t)T + 1);
      iso_compact_kernel<<<grid_for(ctx, T), BLOCK, 0, st>>>(g, queue, base.p, nemit.p, w, T, e0, flag.p, pos.p, queues[parity ^ 1u], ctl.p);
      HIP_CHECK(hipGetLastError());
      read_ctl();
      stats.wide_launches += 4;
      ++stats.levels;
      stats.pairs += w, stats.events += T;
      stats.max_level_width = std::max<uint64_t>(stats.max_level_width, w);
      parity ^= 1u;
    }
    status = h[CTL_STATUS], w = h[CTL_W], T = h[CTL_T], e0 = h[CTL_E0];
  }
  uint32_t h_cnt[3];
  HIP_CHECK(hipMemcpyAsync(h_cnt, cnt.p, sizeof(h_cnt), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  stats.wave_pairs = h_cnt[1], stats.nondet_marks = h_cnt[2];
  if (status == ISO_DONE) return true;
  // the first failure in queue order (isomorphic.rs:149-154): an error iff a mark lies strictly in front of it
  if (h_cnt[0] < h[CTL_FAIL + 1])
    throw Error("Isomorphic: Non-determinism as an unweighted automaton. state1 = " + std::to_string(h[CTL_FS1]) +
                " state2 = " + std::to_string(h[CTL_FS2]));
  return false;
}

}  // namespace wfst
