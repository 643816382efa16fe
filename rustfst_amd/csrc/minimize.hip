// minimize.hip — minimize_with_config (rustfst/src/algorithms/minimize.rs:92-211) of an input-deterministic ACYCLIC
// acceptor on the device: the AcyclicMinimizer branch (Revuz: partition by height, refine height by height), which is a
// pure function of its input.  Transducers, non-deterministic and cyclic inputs are KO (the caller keeps rustfst).
//   facts          ACCEPTOR / I_DETERMINISTIC / WEIGHTED as compute_and_update_properties finds them (minimize.rs:101-106):
//                  the stored word where it knows them, else facts_kernel (16 lanes per state) + idet_kernel (a device hash
//                  set of (state, ilabel))
//   weighted       push_weights(ToInitial) (push.hip), then the ENCODED FST is built on the device (:162-171): every arc and
//                  every final weight quantized (tuple_kernel) and given the scan position of the FIRST occurrence of its
//                  tuple (label, quantized weight) — device hash table keyed by the exact tuple, atomicMin of the position.
//                  The position stands for the encode label (only the order of labels is ever used); it travels in the
//                  arc's olabel.  Final weights become arcs into an appended superfinal state (tr_map.rs:80-181).
//   connect        connect_and_adopt (compose_wide.hip), then tr_sort on the label key (tr_sort.hip)
//   heights        sinks are peeled level by level over a transpose built here (out-degree counters, atomicSub); a state
//                  never peeled lies on or before a cycle -> KO.  The frontier of level h IS the bucket of height h.
//   refine         fused with the peeling, height by height: signature = (final key, arc count, (label key, class of
//                  nextstate) in label-key order); hash table on a 64-bit hash with a FULL compare on every hit; survivor of
//                  a class by atomicMin / atomicMax of the state id: the class holding the height's highest id keeps its
//                  highest id, any other class its lowest (Partition::add prepends and refine() moves members in list
//                  order: partition.rs:46-92, minimize.rs:340-376).  A lane per state up to 64 arcs, a wave per state beyond.
//   regimes        NARROW: one 1024-thread workgroup runs level after level inside one launch (lattices: thousands of
//                  heights of a few states); WIDE: one device-wide launch per phase.  The host switches by the size of the
//                  next level; WFST_MINIMIZE_PATH=auto|narrow|wide pins one.
//   emit           survivors scanned into new ids, their arcs redirected in tr_unique's order (label key, then nextstate:
//                  tr_unique.rs:8-35), labels / weights decoded from the first occurrence, the arcs into the superfinal state
//                  folded back into final weights (rm_final_epsilon.rs), the property word, adopt_device.
// Tuple identity is EXACT (equal label, equal quantized value, -0.0 == +0.0); the reference's HashMap hashes the bits but
// compares with KDELTA, so there two near-equal tuples may or may not merge depending on a random seed.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#pragma clang fp contract(off)  // (before tropical.h comes in: its functions compile without contraction here too)

#include "common.h"
#include "fst_props.h"

namespace wfst {

uint64_t tr_sort_props(uint64_t in, bool ilabel_cmp);  // tr_sort.hip

namespace {

constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint64_t EMPTY_KEY = ~0ull;
constexpr uint32_t TPB = 256;
constexpr uint32_t NARROW_TPB = 1024;   // the narrow regime is one such workgroup
constexpr uint32_t NARROW_MAX = 4096;   // levels of at most this many states stay in the one-workgroup kernel
constexpr uint32_t LANE_MAX_DEG = 64;   // beyond: a wave per state
constexpr uint64_t HI32 = 0xFFFFFFFF00000000ull;
// ctl words
constexpr uint32_t C_LO = 0, C_HI = 1, C_TAIL = 2, C_LEVEL = 3, C_CURMAX = 4, C_NEXTMAX = 5, C_NBIG = 6, C_WORDS = 8;

__device__ inline uint32_t wkey(float f) { return f == 0.0f ? 0u : __float_as_uint(f); }  // -0.0 == +0.0
// words that other lanes of the SAME launch wrote (narrow regime: level after level in one workgroup): device-scope
// accesses, which do not stay in a compute unit's vector L1
__device__ inline uint32_t ld(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void stg(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline uint64_t ld64(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// insert `key` into an open-addressing set of 64-bit keys (EMPTY_KEY = free); returns the slot, *existed = was there
__device__ inline uint32_t set_insert(unsigned long long* keys, uint32_t mask, uint64_t key, bool* existed) {
  uint32_t i = (uint32_t)mix64(key) & mask;
  for (;;) {
    uint64_t cur = ld64(&keys[i]);
    if (cur == EMPTY_KEY) {
      cur = atomicCAS(&keys[i], (unsigned long long)EMPTY_KEY, (unsigned long long)key);
      if (cur == EMPTY_KEY) {
        *existed = false;
        return i;
      }
    }
    if (cur == key) {
      *existed = true;
      return i;
    }
    i = (i + 1) & mask;
  }
}

// ---------------------------------------------------------------- facts of the content (compute_fst_properties.rs:60-190)
// 16 lanes per state.  The union of props::arc_facts over every arc, and FACT_FINAL_WEIGHTED for a final weight that is not one
__global__ void __launch_bounds__(TPB) facts_kernel(const uint32_t* __restrict__ off, const wfst_tr* __restrict__ arcs,
                                                    const float* __restrict__ fin, uint32_t n, uint32_t* __restrict__ out) {
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lane = tid & 15u;
  uint32_t facts = 0;
  for (uint32_t s = tid >> 4; s < n; s += (gridDim.x * blockDim.x) >> 4) {
    const uint32_t b = off[s], e = off[s + 1];
    for (uint32_t i = b + lane; i < e; i += 16) {
      const wfst_tr a = arcs[i];
      facts |= props::arc_facts(a, i > b ? &arcs[i - 1] : nullptr, s);
    }
    if (lane == 0) {
      const float f = fin[s];
      if (f != INF && !is_one(f)) facts |= props::FACT_FINAL_WEIGHTED;
    }
  }
  for (int d = 32; d >= 1; d >>= 1) facts |= __shfl_xor(facts, d);
  if ((threadIdx.x & 63) == 0 && facts) atomicOr(out, facts);
}
// I_DETERMINISTIC: no state has two arcs with one ilabel (a set of (state, ilabel) pairs); *out = 1 when one has
__global__ void __launch_bounds__(TPB) idet_kernel(const uint32_t* __restrict__ off, const wfst_tr* __restrict__ arcs, uint32_t n,
                                                   unsigned long long* __restrict__ keys, uint32_t mask,
                                                   uint32_t* __restrict__ out) {
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lane = tid & 15u;
  bool dup = false;
  for (uint32_t s = tid >> 4; s < n; s += (gridDim.x * blockDim.x) >> 4)
    for (uint32_t i = off[s] + lane; i < off[s + 1]; i += 16) {
      bool existed;
      set_insert(keys, mask, ((uint64_t)s << 32) | arcs[i].ilabel, &existed);
      dup |= existed;
    }
  if (dup) atomicOr(out, 1u);
}

// ---------------------------------------------------------------- the encoded FST (weighted branch)
__global__ void final_flags_kernel(const float* __restrict__ fin, uint32_t n, uint32_t* __restrict__ flag) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s <= n + 1) flag[s] = (s < n && fin[s] != INF) ? 1u : 0u;
}
// offsets of the encoded FST: state s gains one arc when it is final; state n = the superfinal state (no arcs)
__global__ void enc_offsets_kernel(const uint32_t* __restrict__ off, const uint32_t* __restrict__ fcnt, uint32_t n,
                                   uint32_t* __restrict__ off2, float* __restrict__ fin2) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s <= n) {
    off2[s] = off[s] + fcnt[s];
    fin2[s] = s == n ? 0.0f : INF;
  }
  if (s == n) off2[n + 1] = off[n] + fcnt[n];
}
// QuantizeMapper + the encode table in scan order (states in id order, a state's arcs in arc order, then its final weight):
// the encoded arc at scan position p keeps its label in ilabel, its quantized weight in weight, and in olabel the SLOT of its
// tuple; minpos[slot] becomes the smallest scan position that holds the tuple (rank_kernel then swaps slot for position)
__global__ void __launch_bounds__(TPB) tuple_kernel(const uint32_t* __restrict__ off, const wfst_tr* __restrict__ arcs,
                                                    const float* __restrict__ fin, uint32_t n, float delta,
                                                    const uint32_t* __restrict__ off2, wfst_tr* __restrict__ enc,
                                                    unsigned long long* __restrict__ keys, uint32_t mask,
                                                    uint32_t* __restrict__ minpos) {
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lane = tid & 15u;
  for (uint32_t s = tid >> 4; s < n; s += (gridDim.x * blockDim.x) >> 4) {
    const uint32_t b = off[s], deg = off[s + 1] - b, b2 = off2[s];
    for (uint32_t j = lane; j < deg; j += 16) {
      const wfst_tr a = arcs[b + j];
      const float q = quantize(a.weight, delta);
      bool existed;
      const uint32_t slot = set_insert(keys, mask, ((uint64_t)a.ilabel << 32) | wkey(q), &existed);
      atomicMin(&minpos[slot], b2 + j);
      enc[b2 + j] = wfst_tr{a.ilabel, slot, q, a.nextstate};
    }
    const float f = fin[s];
    if (lane == 0 && f != INF) {  // the tuple (0, 0, final weight): one arc into the superfinal state, after the others
      const float q = quantize(f, delta);
      bool existed;
      const uint32_t slot = set_insert(keys, mask, (uint64_t)wkey(q), &existed);
      atomicMin(&minpos[slot], b2 + deg);
      enc[b2 + deg] = wfst_tr{0u, slot, q, n};
    }
  }
}
__global__ void rank_kernel(wfst_tr* __restrict__ enc, uint32_t e2, const uint32_t* __restrict__ minpos) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < e2) enc[i].olabel = minpos[enc[i].olabel];
}
// label order / topological order of the encoded FST (only asked for when connect leaves nothing): FACT_NOT_I_SORTED (its labels
// are equal pairs, carried in olabel) | FACT_NOT_TOP_SORTED
__global__ void __launch_bounds__(TPB) enc_facts_kernel(const uint32_t* __restrict__ off2, const wfst_tr* __restrict__ enc,
                                                        uint32_t n, uint32_t* __restrict__ out) {
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lane = tid & 15u;
  uint32_t facts = 0;
  for (uint32_t s = tid >> 4; s < n; s += (gridDim.x * blockDim.x) >> 4)
    for (uint32_t i = off2[s] + lane; i < off2[s + 1]; i += 16) {
      if (i > off2[s] && enc[i].olabel < enc[i - 1].olabel) facts |= props::FACT_NOT_I_SORTED;
      if (enc[i].nextstate <= s) facts |= props::FACT_NOT_TOP_SORTED;
    }
  for (int d = 32; d >= 1; d >>= 1) facts |= __shfl_xor(facts, d);
  if ((threadIdx.x & 63) == 0 && facts) atomicOr(out, facts);
}

// ---------------------------------------------------------------- transpose
__global__ void __launch_bounds__(TPB) transpose_fill_kernel(const uint32_t* __restrict__ off, const wfst_tr* __restrict__ arcs,
                                                             uint32_t n, const uint32_t* __restrict__ roff,
                                                             uint32_t* __restrict__ cursor, uint32_t* __restrict__ rsrc) {
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lane = tid & 15u;
  for (uint32_t s = tid >> 4; s < n; s += (gridDim.x * blockDim.x) >> 4)
    for (uint32_t i = off[s] + lane; i < off[s + 1]; i += 16) {
      const uint32_t t = arcs[i].nextstate;
      rsrc[roff[t] + atomicAdd(&cursor[t], 1u)] = s;
    }
}

// ---------------------------------------------------------------- heights + refinement
struct Core {
  const uint32_t* off;
  const wfst_tr* arcs;  // sorted on the label key
  const float* fin;
  uint32_t n;
  const uint32_t* roff;
  const uint32_t* rsrc;
  uint32_t* outdeg;  // arcs into states not yet peeled
  uint32_t* order;   // states in peeling order: level after level
  uint32_t* ctl;
  uint32_t* cls;      // survivor of the state's class
  uint32_t* slot_of;  // the state's slot in tab
  unsigned long long* tab;  // 0 = free, else (high half of the signature hash) << 32 | representative + 1
  uint32_t* smin;
  uint32_t* smax;
  uint32_t tmask;
  uint32_t* big;  // states of the level with more than LANE_MAX_DEG arcs
  uint32_t by_olabel;
  uint32_t refine;  // 0: heights only (the cycle check of an untrimmed input)
};

__global__ void core_init_kernel(Core c) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= c.n) return;
  const uint32_t deg = c.off[s + 1] - c.off[s];
  c.outdeg[s] = deg;
  if (deg == 0) {
    c.order[atomicAdd(&c.ctl[C_TAIL], 1u)] = s;
    atomicMax(&c.ctl[C_CURMAX], s);
  }
}
__global__ void core_advance_kernel(Core c) {
  c.ctl[C_LO] = c.ctl[C_HI];
  c.ctl[C_HI] = c.ctl[C_TAIL];
  c.ctl[C_LEVEL] += 1;
  if (c.ctl[C_LEVEL] > 1) {  // (the first call only opens level 0, whose maximum core_init_kernel found)
    c.ctl[C_CURMAX] = c.ctl[C_NEXTMAX];
    c.ctl[C_NEXTMAX] = 0;
  }
  c.ctl[C_NBIG] = 0;
}

__device__ inline uint32_t label_key(const Core& c, const wfst_tr& a) { return c.by_olabel ? a.olabel : a.ilabel; }
__device__ inline uint64_t entry_hash(const Core& c, const wfst_tr& a, uint32_t j) {
  return mix64((((uint64_t)label_key(c, a) << 32) | ld(&c.cls[a.nextstate])) + (uint64_t)(j + 1) * 0x9E3779B97F4A7C15ull);
}
__device__ inline uint64_t head_hash(uint32_t fk, uint32_t deg) { return mix64(((uint64_t)fk << 32) | deg); }
__device__ inline bool entry_equal(const Core& c, const wfst_tr& x, const wfst_tr& y) {
  return label_key(c, x) == label_key(c, y) && ld(&c.cls[x.nextstate]) == ld(&c.cls[y.nextstate]);
}

// a lane per state: signature hash, slot (claimed or joined after a full compare), survivor candidates
__device__ void refine_small(const Core& c, uint32_t lo, uint32_t hi, uint32_t tid, uint32_t nth) {
  for (uint32_t k = lo + tid; k < hi; k += nth) {
    const uint32_t s = ld(&c.order[k]);
    const uint32_t b = c.off[s], deg = c.off[s + 1] - b;
    if (deg > LANE_MAX_DEG) {
      stg(&c.big[atomicAdd(&c.ctl[C_NBIG], 1u)], s);
      continue;
    }
    const uint32_t fk = wkey(c.fin[s]);
    uint64_t h = head_hash(fk, deg);
    for (uint32_t j = 0; j < deg; ++j) h += entry_hash(c, c.arcs[b + j], j);
    h = mix64(h);
    const uint64_t word = (h & HI32) | (uint64_t)(s + 1);
    uint32_t i = (uint32_t)h & c.tmask;
    for (;;) {
      uint64_t cur = ld64(&c.tab[i]);
      if (cur == 0) {
        cur = atomicCAS(&c.tab[i], 0ull, (unsigned long long)word);
        if (cur == 0) break;
      }
      if ((cur & HI32) == (h & HI32)) {  // a hash collision must not merge states: compare everything
        const uint32_t r = (uint32_t)cur - 1u;
        const uint32_t rb = c.off[r];
        bool eq = c.off[r + 1] - rb == deg && wkey(c.fin[r]) == fk;
        for (uint32_t j = 0; eq && j < deg; ++j) eq = entry_equal(c, c.arcs[b + j], c.arcs[rb + j]);
        if (eq) break;
      }
      i = (i + 1) & c.tmask;
    }
    stg(&c.slot_of[s], i);
    atomicMin(&c.smin[i], s);
    atomicMax(&c.smax[i], s);
  }
}
// a wave per state (fan-out above LANE_MAX_DEG): the same hash as a sum of per-arc terms, the compare in strides of 64
__device__ void refine_big(const Core& c, uint32_t nbig, uint32_t wave, uint32_t nwaves, uint32_t lane) {
  for (uint32_t k = wave; k < nbig; k += nwaves) {
    const uint32_t s = ld(&c.big[k]);
    const uint32_t b = c.off[s], deg = c.off[s + 1] - b;
    const uint32_t fk = wkey(c.fin[s]);
    uint64_t part = 0;
    for (uint32_t j = lane; j < deg; j += 64) part += entry_hash(c, c.arcs[b + j], j);
    for (int d = 32; d >= 1; d >>= 1) part += __shfl_xor(part, d);
    const uint64_t h = mix64(head_hash(fk, deg) + part);
    const uint64_t word = (h & HI32) | (uint64_t)(s + 1);
    uint32_t i = (uint32_t)h & c.tmask;
    for (;;) {
      uint64_t cur = 0;
      if (lane == 0) {
        cur = ld64(&c.tab[i]);
        if (cur == 0) {
          cur = atomicCAS(&c.tab[i], 0ull, (unsigned long long)word);
          if (cur == 0) cur = word;
        }
      }
      cur = __shfl(cur, 0);
      if (cur == word) break;
      if ((cur & HI32) == (h & HI32)) {
        const uint32_t r = (uint32_t)cur - 1u;
        const uint32_t rb = c.off[r];
        bool diff = !(c.off[r + 1] - rb == deg && wkey(c.fin[r]) == fk);
        if (!diff)
          for (uint32_t j = lane; j < deg; j += 64) diff |= !entry_equal(c, c.arcs[b + j], c.arcs[rb + j]);
        if (!__any(diff)) break;
      }
      i = (i + 1) & c.tmask;
    }
    if (lane == 0) {
      stg(&c.slot_of[s], i);
      atomicMin(&c.smin[i], s);
      atomicMax(&c.smax[i], s);
    }
  }
}
// the level's classes get their survivors; its states leave the graph: a predecessor whose last arc goes joins the next level
__device__ void assign_peel(const Core& c, uint32_t lo, uint32_t hi, uint32_t tid, uint32_t nth) {
  const uint32_t cnt = hi - lo;
  uint32_t g = 16;  // lanes per state: more when the level is thin (the superfinal state has one in-arc per final state)
  while (g < blockDim.x && (uint64_t)g * 2u * cnt <= nth) g *= 2;
  const uint32_t lane = tid & (g - 1);
  const uint32_t top = c.refine ? ld(&c.slot_of[ld(&c.ctl[C_CURMAX])]) : 0u;
  uint32_t mx = 0;
  for (uint32_t k = lo + tid / g; k < hi; k += nth / g) {
    const uint32_t s = ld(&c.order[k]);
    if (c.refine && lane == 0) {
      const uint32_t sl = ld(&c.slot_of[s]);
      stg(&c.cls[s], sl == top ? ld(&c.smax[sl]) : ld(&c.smin[sl]));
    }
    for (uint32_t i = c.roff[s] + lane; i < c.roff[s + 1]; i += g) {
      const uint32_t p = c.rsrc[i];
      if (atomicSub(&c.outdeg[p], 1u) == 1u) {
        stg(&c.order[atomicAdd(&c.ctl[C_TAIL], 1u)], p);
        mx = max(mx, p);
      }
    }
  }
  for (int d = 32; d >= 1; d >>= 1) mx = max(mx, (uint32_t)__shfl_xor(mx, d));
  if ((threadIdx.x & 63) == 0 && mx) atomicMax(&c.ctl[C_NEXTMAX], mx);
}

// WIDE: one launch per phase of one level
__global__ void __launch_bounds__(TPB) wide_small_kernel(Core c) {
  refine_small(c, c.ctl[C_LO], c.ctl[C_HI], blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}
__global__ void __launch_bounds__(TPB) wide_big_kernel(Core c) {
  refine_big(c, c.ctl[C_NBIG], (blockIdx.x * blockDim.x + threadIdx.x) >> 6, (gridDim.x * blockDim.x) >> 6, threadIdx.x & 63u);
}
__global__ void __launch_bounds__(TPB) wide_peel_kernel(Core c) {
  assign_peel(c, c.ctl[C_LO], c.ctl[C_HI], blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}
// NARROW: one workgroup, level after level while the level holds at most `narrow_max` states
__global__ void __launch_bounds__(NARROW_TPB) narrow_kernel(Core c, uint32_t narrow_max) {
  __shared__ uint32_t s_lo, s_hi, s_nbig;
  const uint32_t tid = threadIdx.x;
  if (tid == 0) {
    s_lo = c.ctl[C_LO];
    s_hi = c.ctl[C_HI];
  }
  __syncthreads();
  for (;;) {
    const uint32_t lo = s_lo, hi = s_hi;
    if (hi == lo || hi - lo > narrow_max) break;
    if (c.refine) {
      refine_small(c, lo, hi, tid, NARROW_TPB);
      __threadfence();
      __syncthreads();
      if (tid == 0) s_nbig = ld(&c.ctl[C_NBIG]);
      __syncthreads();
      if (s_nbig) refine_big(c, s_nbig, tid >> 6, NARROW_TPB >> 6, tid & 63u);
      __threadfence();
      __syncthreads();
    }
    assign_peel(c, lo, hi, tid, NARROW_TPB);
    __threadfence();
    __syncthreads();
    if (tid == 0) {
      s_lo = hi;
      s_hi = ld(&c.ctl[C_TAIL]);
      stg(&c.ctl[C_LO], s_lo);
      stg(&c.ctl[C_HI], s_hi);
      stg(&c.ctl[C_LEVEL], ld(&c.ctl[C_LEVEL]) + 1u);
      stg(&c.ctl[C_CURMAX], ld(&c.ctl[C_NEXTMAX]));
      stg(&c.ctl[C_NEXTMAX], 0u);
      stg(&c.ctl[C_NBIG], 0u);
    }
    __threadfence();
    __syncthreads();
  }
}

// ---------------------------------------------------------------- emit
// the unweighted branch compares no weights (minimize.rs:389-456), merge_states appends the members' arcs to the survivor
// and tr_unique drops those EQUAL to the survivor's (Tr's ==: approximate on the weight).  Flag a member arc that would stay.
__global__ void weight_check_kernel(Core c, uint32_t* __restrict__ flag) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= c.n) return;
  const uint32_t r = c.cls[s];
  if (r == s) return;
  const uint32_t b = c.off[s], rb = c.off[r], deg = c.off[s + 1] - b;
  bool bad = false;
  for (uint32_t j = 0; j < deg; ++j) bad |= !weq(c.arcs[b + j].weight, c.arcs[rb + j].weight);
  if (bad) atomicOr(flag, 1u);
}
// keep[s]: s survives (the superfinal state of the weighted branch, the last state, goes)
__global__ void keep_kernel(const uint32_t* __restrict__ cls, uint32_t n, uint32_t superfinal, uint32_t* __restrict__ keep) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s <= n) keep[s] = (s < n && cls[s] == s && s != superfinal) ? 1u : 0u;
}
// arcs the survivor keeps: all but the one into the superfinal state
__global__ void __launch_bounds__(TPB) emit_count_kernel(const uint32_t* __restrict__ off, const wfst_tr* __restrict__ arcs,
                                                         uint32_t n, uint32_t superfinal, const uint32_t* __restrict__ keep,
                                                         const uint32_t* __restrict__ new_id, uint32_t* __restrict__ cnt) {
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lane = tid & 15u;
  for (uint32_t s = tid >> 4; s < n; s += (gridDim.x * blockDim.x) >> 4) {
    if (!keep[s]) continue;  // (uniform over the 16 lanes)
    uint32_t k = 0;
    for (uint32_t i = off[s] + lane; i < off[s + 1]; i += 16) k += arcs[i].nextstate != superfinal;
    for (int d = 8; d >= 1; d >>= 1) k += __shfl_xor(k, d, 16);
    if (lane == 0) cnt[new_id[s]] = k;
  }
}
// the survivor's arcs in their sorted order, redirected to survivors' new ids; weighted branch (enc != null): label and
// weight decoded from the first occurrence of the tuple (its scan position sits in olabel), the arc into the superfinal state
// becomes the final weight: zero (+) (final(superfinal) = one (x) w) (rm_final_epsilon.rs:45-60)
__global__ void __launch_bounds__(TPB) emit_kernel(const uint32_t* __restrict__ off, const wfst_tr* __restrict__ arcs,
                                                   const float* __restrict__ fin, uint32_t n, uint32_t superfinal,
                                                   const uint32_t* __restrict__ keep, const uint32_t* __restrict__ new_id,
                                                   const uint32_t* __restrict__ cls, const wfst_tr* __restrict__ enc,
                                                   const uint32_t* __restrict__ off_out, wfst_tr* __restrict__ arcs_out,
                                                   float* __restrict__ fin_out) {
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lane = tid & 15u;
  for (uint32_t s = tid >> 4; s < n; s += (gridDim.x * blockDim.x) >> 4) {
    if (!keep[s]) continue;
    const uint32_t b = off[s], deg = off[s + 1] - b, ns = new_id[s], ob = off_out[ns];
    uint32_t pf = NONE;  // position of the arc into the superfinal state (at most one per state)
    if (enc) {
      for (uint32_t j = lane; j < deg; j += 16)
        if (arcs[b + j].nextstate == superfinal) pf = min(pf, j);
      for (int d = 8; d >= 1; d >>= 1) pf = min(pf, (uint32_t)__shfl_xor(pf, d, 16));
    }
    for (uint32_t j = lane; j < deg; j += 16) {
      const wfst_tr a = arcs[b + j];
      if (j == pf) continue;
      const uint32_t o = ob + j - (j > pf ? 1u : 0u);
      const uint32_t t = new_id[cls[a.nextstate]];
      if (enc) {
        const wfst_tr first = enc[a.olabel];
        arcs_out[o] = wfst_tr{first.ilabel, first.ilabel, first.weight, t};
      } else {
        arcs_out[o] = wfst_tr{a.ilabel, a.olabel, a.weight, t};
      }
    }
    if (lane == 0) {
      float f = fin[s];
      if (enc) {
        f = INF;
        if (pf != NONE) {
          const float w = 0.0f + enc[arcs[b + pf].olabel].weight;  // one (x) w
          f = w < f ? w : f;                                         // zero (+) ..
        }
      }
      fin_out[ns] = f;
    }
  }
}

// ---------------------------------------------------------------- host side
enum class Path { Auto, Narrow, Wide };
Path path_knob() {
  const char* e = std::getenv("WFST_MINIMIZE_PATH");
  if (!e || !*e || !std::strcmp(e, "auto")) return Path::Auto;
  if (!std::strcmp(e, "narrow")) return Path::Narrow;
  if (!std::strcmp(e, "wide")) return Path::Wide;
  throw Error(std::string("WFST_MINIMIZE_PATH: expected auto, narrow or wide, not '") + e + "'");
}

uint32_t grid16(wfst_ctx* ctx, uint32_t n) {  // 16 lanes per state
  return std::max<uint32_t>(1, std::min<uint32_t>((n + 15) / 16, (uint32_t)ctx->n_cus * 32));
}
// (the scratch goes back to the pool at once: synchronise first)
void scan_sync(wfst_ctx* ctx, const uint32_t* in, uint32_t* out, size_t count) {
  const DBuf<uint8_t> temp = exclusive_scan_u32(ctx, in, out, count);
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
}

// facts of the content, gathered once
struct Facts {
  bool have = false, have_idet = false;
  uint32_t bits = 0;
  bool nondet = false;
};
void content_facts(wfst_ctx* ctx, const wfst_fst* f, Facts& fa) {
  if (fa.have) return;
  DBuf<uint32_t> out(*ctx->pool, 1);
  HIP_CHECK(hipMemsetAsync(out.p, 0, sizeof(uint32_t), ctx->stream));
  if (f->n_states) {
    facts_kernel<<<grid16(ctx, f->n_states), TPB, 0, ctx->stream>>>(f->dev.offsets, f->dev.arcs, f->dev.finals, f->n_states, out.p);
    HIP_CHECK(hipGetLastError());
  }
  fa.bits = read_u32(ctx, out.p);
  fa.have = true;
}
void content_idet(wfst_ctx* ctx, const wfst_fst* f, Facts& fa) {
  if (fa.have_idet) return;
  uint32_t dup = 0;
  if (f->n_arcs > 1) {
    const uint32_t size = pow2_at_least(2 * f->n_arcs, "minimize");
    DBuf<unsigned long long> keys(*ctx->pool, size);
    DBuf<uint32_t> out(*ctx->pool, 1);
    HIP_CHECK(hipMemsetAsync(keys.p, 0xFF, (size_t)size * sizeof(unsigned long long), ctx->stream));
    HIP_CHECK(hipMemsetAsync(out.p, 0, sizeof(uint32_t), ctx->stream));
    idet_kernel<<<grid16(ctx, f->n_states), TPB, 0, ctx->stream>>>(f->dev.offsets, f->dev.arcs, f->n_states, keys.p, size - 1, out.p);
    HIP_CHECK(hipGetLastError());
    dup = read_u32(ctx, out.p);
  }
  fa.nondet = dup != 0;
  fa.have_idet = true;
}
struct CoreBufs {
  DBuf<uint32_t> rcnt, roff, rsrc, outdeg, order, ctl, cls, slot_of, smin, smax, big;
  DBuf<unsigned long long> tab;
  Core c{};
  uint32_t peeled = 0;
};
// heights (and, with `refine`, the classes) of the graph (off, arcs, fin) with n states and E arcs
void run_core(wfst_ctx* ctx, CoreBufs& B, uint32_t n, uint64_t E, const uint32_t* off, const wfst_tr* arcs, const float* fin,
              bool refine, bool by_olabel, Path path) {
  hipStream_t st = ctx->stream;
  DevicePool& pool = *ctx->pool;
  B.rcnt = DBuf<uint32_t>(pool, (size_t)n + 1);
  B.roff = DBuf<uint32_t>(pool, (size_t)n + 1);
  B.rsrc = DBuf<uint32_t>(pool, E);
  B.outdeg = DBuf<uint32_t>(pool, n);
  B.order = DBuf<uint32_t>(pool, n);
  B.ctl = DBuf<uint32_t>(pool, C_WORDS);
  HIP_CHECK(hipMemsetAsync(B.rcnt.p, 0, ((size_t)n + 1) * sizeof(uint32_t), st));
  HIP_CHECK(hipMemsetAsync(B.ctl.p, 0, C_WORDS * sizeof(uint32_t), st));
  count_indegrees(ctx, arcs, E, B.rcnt.p);
  scan_sync(ctx, B.rcnt.p, B.roff.p, (size_t)n + 1);
  HIP_CHECK(hipMemsetAsync(B.rcnt.p, 0, ((size_t)n + 1) * sizeof(uint32_t), st));
  if (E) {
    transpose_fill_kernel<<<grid16(ctx, n), TPB, 0, st>>>(off, arcs, n, B.roff.p, B.rcnt.p, B.rsrc.p);
    HIP_CHECK(hipGetLastError());
  }
  Core& c = B.c;
  c.off = off;
  c.arcs = arcs;
  c.fin = fin;
  c.n = n;
  c.roff = B.roff.p;
  c.rsrc = B.rsrc.p;
  c.outdeg = B.outdeg.p;
  c.order = B.order.p;
  c.ctl = B.ctl.p;
  c.by_olabel = by_olabel ? 1u : 0u;
  c.refine = refine ? 1u : 0u;
  if (refine) {
    const uint32_t size = pow2_at_least(2 * (uint64_t)n, "minimize");
    B.cls = DBuf<uint32_t>(pool, n);
    B.slot_of = DBuf<uint32_t>(pool, n);
    B.big = DBuf<uint32_t>(pool, n);
    B.smin = DBuf<uint32_t>(pool, size);
    B.smax = DBuf<uint32_t>(pool, size);
    B.tab = DBuf<unsigned long long>(pool, size);
    HIP_CHECK(hipMemsetAsync(B.tab.p, 0, (size_t)size * sizeof(unsigned long long), st));
    HIP_CHECK(hipMemsetAsync(B.smin.p, 0xFF, (size_t)size * sizeof(uint32_t), st));
    HIP_CHECK(hipMemsetAsync(B.smax.p, 0, (size_t)size * sizeof(uint32_t), st));
    c.cls = B.cls.p;
    c.slot_of = B.slot_of.p;
    c.big = B.big.p;
    c.smin = B.smin.p;
    c.smax = B.smax.p;
    c.tab = B.tab.p;
    c.tmask = size - 1;
  }
  core_init_kernel<<<(n + TPB - 1) / TPB, TPB, 0, st>>>(c);
  core_advance_kernel<<<1, 1, 0, st>>>(c);
  HIP_CHECK(hipGetLastError());
  uint32_t h[C_WORDS];
  const uint32_t narrow_max = path == Path::Narrow ? NONE : NARROW_MAX;
  for (;;) {
    HIP_CHECK(hipMemcpyAsync(h, B.ctl.p, sizeof(h), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    const uint32_t cnt = h[C_HI] - h[C_LO];
    if (cnt == 0) break;
    if (path != Path::Wide && cnt <= narrow_max) {
      narrow_kernel<<<1, NARROW_TPB, 0, st>>>(c, narrow_max);
    } else {
      const uint32_t cap = (uint32_t)ctx->n_cus * 16;
      if (refine) {
        wide_small_kernel<<<std::max(1u, std::min((cnt + TPB - 1) / TPB, cap)), TPB, 0, st>>>(c);
        wide_big_kernel<<<std::max(1u, std::min((cnt + 3) / 4, cap)), TPB, 0, st>>>(c);
      }
      wide_peel_kernel<<<std::max(1u, std::min((cnt + 15) / 16, cap)), TPB, 0, st>>>(c);
      core_advance_kernel<<<1, 1, 0, st>>>(c);
    }
    HIP_CHECK(hipGetLastError());
  }
  B.peeled = h[C_TAIL];
}

wfst_fst* empty_fst(wfst_ctx* ctx, uint64_t p) {
  HostCsr hc;
  hc.offsets.push_back(0);
  return make_host_fst(ctx, 0, -1, p & props::ALL, std::move(hc));
}

// AcyclicMinimizer + merge_states + tr_unique (+ decode for the weighted branch, enc != null) of the connected, sorted T
wfst_fst* minimize_connected(wfst_ctx* ctx, const wfst_fst* T, const wfst_tr* enc, uint64_t out_props, Path path) {
  hipStream_t st = ctx->stream;
  DevicePool& pool = *ctx->pool;
  const uint32_t n = T->n_states;
  const uint64_t E = T->n_arcs;
  const uint32_t superfinal = enc ? n - 1 : NONE;
  CoreBufs B;
  run_core(ctx, B, n, E, T->dev.offsets, T->dev.arcs, T->dev.finals, true, enc != nullptr, path);
  if (B.peeled != n) throw Error("minimize: cyclic inputs are not supported; use rustfst's minimize");
  if (!enc && E) {
    DBuf<uint32_t> flag(pool, 1);
    HIP_CHECK(hipMemsetAsync(flag.p, 0, sizeof(uint32_t), st));
    weight_check_kernel<<<(n + TPB - 1) / TPB, TPB, 0, st>>>(B.c, flag.p);
    HIP_CHECK(hipGetLastError());
    if (read_u32(ctx, flag.p))
      throw Error("minimize: an unweighted input whose merged states carry arc weights further than 1/1024 apart is not "
                  "supported (the reference keeps both arcs); use rustfst's minimize");
  }
  DBuf<uint32_t> keep(pool, (size_t)n + 1), new_id(pool, (size_t)n + 1);
  keep_kernel<<<(n + 1 + TPB - 1) / TPB, TPB, 0, st>>>(B.c.cls, n, superfinal, keep.p);
  HIP_CHECK(hipGetLastError());
  scan_sync(ctx, keep.p, new_id.p, (size_t)n + 1);
  uint32_t n_out = 0, start_cls = 0;
  HIP_CHECK(hipMemcpyAsync(&n_out, new_id.p + n, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(&start_cls, B.c.cls + T->start, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  uint32_t new_start = 0;
  HIP_CHECK(hipMemcpyAsync(&new_start, new_id.p + start_cls, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  DBuf<uint32_t> cnt(pool, (size_t)n_out + 1), off_out(pool, (size_t)n_out + 1);
  HIP_CHECK(hipMemsetAsync(cnt.p, 0, ((size_t)n_out + 1) * sizeof(uint32_t), st));
  emit_count_kernel<<<grid16(ctx, n), TPB, 0, st>>>(T->dev.offsets, T->dev.arcs, n, superfinal, keep.p, new_id.p, cnt.p);
  HIP_CHECK(hipGetLastError());
  scan_sync(ctx, cnt.p, off_out.p, (size_t)n_out + 1);
  const uint32_t e_out = read_u32(ctx, off_out.p + n_out);
  DBuf<wfst_tr> arcs_out(pool, e_out);
  DBuf<float> fin_out(pool, n_out);
  emit_kernel<<<grid16(ctx, n), TPB, 0, st>>>(T->dev.offsets, T->dev.arcs, T->dev.finals, n, superfinal, keep.p, new_id.p, B.c.cls,
                                              enc, off_out.p, arcs_out.p, fin_out.p);
  HIP_CHECK(hipGetLastError());
  return adopt_device(ctx, n_out, e_out, new_start, out_props & props::ALL, off_out.p, arcs_out.p, fin_out.p);
}

// the graph has a cycle (anywhere: the reference's DFS visits every state) — by peeling sinks, without refinement
bool has_cycle(wfst_ctx* ctx, const wfst_fst* f, Path path) {
  if (f->n_states == 0) return false;
  CoreBufs B;
  run_core(ctx, B, f->n_states, f->n_arcs, f->dev.offsets, f->dev.arcs, f->dev.finals, false, false, path);
  return B.peeled != f->n_states;
}

}  // namespace

// minimize_with_config (minimize.rs:92-176) for the acyclic deterministic acceptor branch: a NEW handle
wfst_fst* minimize_fst(wfst_ctx* ctx, const wfst_fst* f, float delta, bool allow_nondet) {
  using namespace props;
  const Path path = path_knob();
  hipStream_t st = ctx->stream;
  DevicePool& pool = *ctx->pool;
  ensure_device(const_cast<wfst_fst*>(f));
  const uint32_t n = f->n_states;
  uint64_t p = f->props & ALL;
  Facts fa;
  // compute_and_update_properties(ACCEPTOR | I_DETERMINISTIC | WEIGHTED | UNWEIGHTED) (:101-106): the stored word if it
  // knows all of them (compute_fst_properties.rs:22-28), else everything the arc scan finds
  if (!(knows(p, ACCEPTOR) && knows(p, I_DETERMINISTIC) && knows(p, WEIGHTED))) {
    content_facts(ctx, f, fa);
    content_idet(ctx, f, fa);
    p = merge_computed(p, content_props(fa.bits) | (fa.nondet ? NOT_I_DETERMINISTIC : I_DETERMINISTIC));
  }
  if (!(p & I_DETERMINISTIC) && !allow_nondet)
    throw Error("Refusing to minimize a non-deterministic FST with allow_nondet = false");
  if (!(p & ACCEPTOR))
    throw Error("minimize: transducers are not supported (the input is not an acceptor); use rustfst's minimize");
  if (!(p & I_DETERMINISTIC)) throw Error("minimize: non-deterministic inputs are not supported; use rustfst's minimize");

  // ACYCLIC, as acceptor_minimize's compute_and_update_properties finds it on the UNTRIMMED FST (:185-187, 198): stored, or
  // computed.  Any cycle is KO here, also one that connect would remove (the reference takes Hopcroft's branch then).
  bool computed_dfs = false;
  if (!knows(p, CYCLIC)) {
    if (has_cycle(ctx, f, path)) throw Error("minimize: cyclic inputs are not supported; use rustfst's minimize");
    computed_dfs = true;
  } else if (p & CYCLIC) {
    throw Error("minimize: cyclic inputs are not supported; use rustfst's minimize");
  }

  if (!(p & WEIGHTED)) {
    // ---- unweighted acceptor (:172-175): acceptor_minimize on the original labels
    if (computed_dfs) {  // the DFS pairs, the arc scan's pairs (no determinism: not in the mask) and UNWEIGHTED_CYCLES
      content_facts(ctx, f, fa);
      // ACCESSIBLE / COACCESSIBLE: connect overwrites both pairs (connect.rs:61-64), so their computed values never show
      p = merge_computed(p, content_props(fa.bits) | ACYCLIC | INITIAL_ACYCLIC | ACCESSIBLE | COACCESSIBLE | UNWEIGHTED_CYCLES);
    }
    // connect (:193): del_states' mask, then ACCESSIBLE | COACCESSIBLE
    const uint64_t pc = delete_states(p) | ACCESSIBLE | COACCESSIBLE;
    Handle T(connect_and_adopt(ctx, n, f->start, f->dev.offsets, f->dev.arcs, f->dev.finals, /*all_accessible=*/false, pc));
    if (T->n_states == 0) return T.release();  // (:195-197)
    tr_sort_device(ctx, T.get(), true);         // tr_sort(ILabelCompare) (:201)
    const uint64_t pd = tr_sort_props(pc, true);
    uint64_t out;
    if (T->n_arcs) {
      // merge_states: every class with arcs rewrites its representative's arcs through set_nextstate_unchecked, whose mask
      // (trs_iter_mut.rs:293-305) keeps the ACCEPTOR, epsilon and WEIGHTED pairs only; add_tr, set_start, connect and
      // tr_unique (mutate_properties.rs:43-100, 7-13; tr_unique.rs:45-50) add no positive bit of those pairs and connect's
      // mask drops every negative one
      out = pd & (ACCEPTOR | NO_EPSILONS | NO_I_EPSILONS | NO_O_EPSILONS | UNWEIGHTED);
    } else {  // one final state: no arc is touched; set_start, connect, tr_unique
      out = delete_states(set_start(pd)) | ACCESSIBLE | COACCESSIBLE;
      out &= ARCSORT_MASK & DELETE_ARCS_MASK;
    }
    return minimize_connected(ctx, T.get(), nullptr, out, path);
  }

  // ---- weighted acceptor (:162-171)
  if (f->start < 0) {
    // No start state: push_weights still reweights arcs and final weights (reweight.rs skips only the start-state step),
    // then every tr_map returns at once (tr_map.rs:86-88): no quantization, no encoding.  acceptor_minimize recomputes its
    // facts from the PUSHED content (reweight_properties left WEIGHTED unknown) and bails on a weight that is still
    // neither one nor zero; otherwise connect removes everything, decode's tr_map returns at once again and
    // rm_final_epsilon connects the empty FST once more.
    Handle V(new wfst_fst);  // f with the word of step 1 (the reference updated it in place): push's bookkeeping starts there
    V->owner_pool = f->owner_pool;
    V->device = f->device;
    V->ctx = f->ctx;
    V->n_states = f->n_states;
    V->n_arcs = f->n_arcs;
    V->start = -1;
    V->props = p;
    V->has_dev = true;
    V->mean_weight = f->mean_weight;
    V->has_negative = f->has_negative;
    V->dev = f->dev;
    Handle P(push_weights_fst(ctx, V.get(), /*ToInitial*/ 0u, /*remove_total_weight=*/false));
    ensure_device(P.get());
    Facts pf;
    content_facts(ctx, P.get(), pf);
    // compute_and_update_properties(ACCEPTOR | UNWEIGHTED | ACYCLIC) (:185-187): the DFS pairs (acyclic: checked above; no
    // start state, so nothing is accessible; COACCESSIBLE is overwritten by connect) and the arc scan's pairs
    const uint64_t comp = content_props(pf.bits) | ACYCLIC | INITIAL_ACYCLIC | NOT_ACCESSIBLE | COACCESSIBLE | UNWEIGHTED_CYCLES;
    if (comp & (NOT_ACCEPTOR | WEIGHTED)) throw Error("FST is not an unweighted acceptor");  // (:188-190)
    return empty_fst(ctx, delete_states(merge_computed(P->props & ALL, comp)) | ACCESSIBLE | COACCESSIBLE);
  }
  Handle P(push_weights_fst(ctx, f, /*ToInitial*/ 0u, /*remove_total_weight=*/false));
  ensure_device(P.get());
  const uint32_t np = P->n_states;
  const uint64_t ep = P->n_arcs;
  if (ep + np + 2 >= (1ull << 31)) throw Error("minimize: input too large");
  // encode(EncodeWeightsAndLabels) of the quantized FST, untrimmed
  DBuf<uint32_t> flag(pool, (size_t)np + 2), fcnt(pool, (size_t)np + 2), off2(pool, (size_t)np + 2);
  DBuf<float> fin2(pool, (size_t)np + 1);
  final_flags_kernel<<<(np + 2 + TPB - 1) / TPB, TPB, 0, st>>>(P->dev.finals, np, flag.p);
  HIP_CHECK(hipGetLastError());
  scan_sync(ctx, flag.p, fcnt.p, (size_t)np + 2);
  enc_offsets_kernel<<<(np + 1 + TPB - 1) / TPB, TPB, 0, st>>>(P->dev.offsets, fcnt.p, np, off2.p, fin2.p);
  HIP_CHECK(hipGetLastError());
  const uint32_t e2 = read_u32(ctx, off2.p + np);
  DBuf<wfst_tr> enc(pool, e2);
  {
    const uint32_t size = pow2_at_least(2 * (uint64_t)e2, "minimize");
    DBuf<unsigned long long> keys(pool, size);
    DBuf<uint32_t> minpos(pool, size);
    HIP_CHECK(hipMemsetAsync(keys.p, 0xFF, (size_t)size * sizeof(unsigned long long), st));
    HIP_CHECK(hipMemsetAsync(minpos.p, 0xFF, (size_t)size * sizeof(uint32_t), st));
    tuple_kernel<<<grid16(ctx, np), TPB, 0, st>>>(P->dev.offsets, P->dev.arcs, P->dev.finals, np, delta, off2.p, enc.p, keys.p,
                                                 size - 1, minpos.p);
    HIP_CHECK(hipGetLastError());
    if (e2) rank_kernel<<<(e2 + TPB - 1) / TPB, TPB, 0, st>>>(enc.p, e2, minpos.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(st));
  }
  // acceptor_minimize: connect (the word of the trimmed FST starts empty: every bit is fixed below)
  Handle T(connect_and_adopt(ctx, np + 1, P->start, off2.p, enc.p, fin2.p, /*all_accessible=*/false, 0));
  if (T->n_states == 0) {
    // nothing reaches a final state: the encoded FST's computed word (compute_fst_properties on its content: labels >= 1,
    // weights one, acyclic) through connect's mask; decode's tr_map returns at once, rm_final_epsilon connects again
    DBuf<uint32_t> out(pool, 1);
    HIP_CHECK(hipMemsetAsync(out.p, 0, sizeof(uint32_t), st));
    enc_facts_kernel<<<grid16(ctx, np + 1), TPB, 0, st>>>(off2.p, enc.p, np + 1, out.p);
    HIP_CHECK(hipGetLastError());
    const uint32_t bits = read_u32(ctx, out.p);
    uint64_t comp = ACCEPTOR | NO_EPSILONS | NO_I_EPSILONS | NO_O_EPSILONS | UNWEIGHTED | ACYCLIC | INITIAL_ACYCLIC | UNWEIGHTED_CYCLES;
    if (!(bits & FACT_NOT_I_SORTED)) comp |= I_LABEL_SORTED | O_LABEL_SORTED;
    if (!(bits & FACT_NOT_TOP_SORTED)) comp |= TOP_SORTED;
    return empty_fst(ctx, delete_states(comp) | ACCESSIBLE | COACCESSIBLE);
  }
  tr_sort_device(ctx, T.get(), false);  // tr_sort(ILabelCompare) on the encode labels (olabel carries their order)
  // decode's mapper keeps none of the bits tr_unique leaves (decode_static.rs:52-66); rm_final_epsilon's set_final /
  // del_trs pairs end in delete_trs_properties and connect (rm_final_epsilon.rs:62-75): ACCESSIBLE | COACCESSIBLE
  return minimize_connected(ctx, T.get(), enc.p, ACCESSIBLE | COACCESSIBLE, path);
}

}  // namespace wfst
