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
//                  next level; WFST_MINIMIZE_PATH=auto|narrow|wide pins one.  Which one ran: wfst_ctx_get_minimize_stats,
//                  tallied on the host from the control block (include/wfst.h; WFST_MINIMIZE_HASH_BITS for tests).
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

#include "batch_driver.h"
#include "common.h"
#include "fst_props.h"
#include "wg_ops.h"

namespace wfst {

uint64_t tr_sort_props(uint64_t in, bool ilabel_cmp);  // tr_sort.hip

namespace {

// the KO messages (wfst_minimize and, behind "item <i>: ", wfst_minimize_batch)
constexpr const char* MSG_REFUSE_NONDET = "Refusing to minimize a non-deterministic FST with allow_nondet = false";
constexpr const char* MSG_TRANSDUCER = "minimize: transducers are not supported (the input is not an acceptor); use rustfst's minimize";
constexpr const char* MSG_NONDET = "minimize: non-deterministic inputs are not supported; use rustfst's minimize";
constexpr const char* MSG_CYCLIC = "minimize: cyclic inputs are not supported; use rustfst's minimize";
constexpr const char* MSG_FAR_APART =
    "minimize: an unweighted input whose merged states carry arc weights further than 1/1024 apart is not "
    "supported (the reference keeps both arcs); use rustfst's minimize";
constexpr const char* MSG_NOT_UNWEIGHTED = "FST is not an unweighted acceptor";

constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint64_t EMPTY_KEY = ~0ull;
constexpr uint32_t TPB = 256;
constexpr uint32_t NARROW_TPB = 1024;   // the narrow regime is one such workgroup
constexpr uint32_t NARROW_MAX = 4096;   // levels of at most this many states stay in the one-workgroup kernel
constexpr uint32_t LANE_MAX_DEG = 64;   // beyond: a wave per state
constexpr uint64_t HI32 = 0xFFFFFFFF00000000ull;
// ctl words
// (C_WAVE: the C_NBIG of every level so far; C_UNEQ: full compares that found a difference — wfst_ctx_get_minimize_stats)
constexpr uint32_t C_LO = 0, C_HI = 1, C_TAIL = 2, C_LEVEL = 3, C_CURMAX = 4, C_NEXTMAX = 5, C_NBIG = 6, C_WAVE = 7, C_UNEQ = 8,
                   C_WORDS = 10;

__device__ inline uint32_t wkey(float f) { return f == 0.0f ? 0u : __float_as_uint(f); }  // -0.0 == +0.0
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
// (thread `tid` of `nth`: its share, to be OR-ed over the threads)
__device__ uint32_t facts_of_states(const uint32_t* __restrict__ off, const wfst_tr* __restrict__ arcs,
                                    const float* __restrict__ fin, uint32_t n, uint32_t tid, uint32_t nth) {
  const uint32_t lane = tid & 15u;
  uint32_t facts = 0;
  for (uint32_t s = tid >> 4; s < n; s += nth >> 4) {
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
  return facts;
}
__global__ void __launch_bounds__(TPB) facts_kernel(const uint32_t* __restrict__ off, const wfst_tr* __restrict__ arcs,
                                                    const float* __restrict__ fin, uint32_t n, uint32_t* __restrict__ out) {
  uint32_t facts = facts_of_states(off, arcs, fin, n, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
  for (int d = 32; d >= 1; d >>= 1) facts |= __shfl_xor(facts, d);
  if ((threadIdx.x & 63) == 0 && facts) atomicOr(out, facts);
}
// I_DETERMINISTIC: no state has two arcs with one ilabel (a set of (state, ilabel) pairs); *out = 1 when one has
__device__ bool idet_of_states(const uint32_t* __restrict__ off, const wfst_tr* __restrict__ arcs, uint32_t n,
                               unsigned long long* __restrict__ keys, uint32_t mask, uint32_t tid, uint32_t nth) {
  const uint32_t lane = tid & 15u;
  bool dup = false;
  for (uint32_t s = tid >> 4; s < n; s += nth >> 4)
    for (uint32_t i = off[s] + lane; i < off[s + 1]; i += 16) {
      bool existed;
      set_insert(keys, mask, ((uint64_t)s << 32) | arcs[i].ilabel, &existed);
      dup |= existed;
    }
  return dup;
}
__global__ void __launch_bounds__(TPB) idet_kernel(const uint32_t* __restrict__ off, const wfst_tr* __restrict__ arcs, uint32_t n,
                                                   unsigned long long* __restrict__ keys, uint32_t mask,
                                                   uint32_t* __restrict__ out) {
  if (idet_of_states(off, arcs, n, keys, mask, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x)) atomicOr(out, 1u);
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
__device__ void tuples_of_states(const uint32_t* __restrict__ off, const wfst_tr* __restrict__ arcs,
                                 const float* __restrict__ fin, uint32_t n, float delta, const uint32_t* __restrict__ off2,
                                 wfst_tr* __restrict__ enc, unsigned long long* __restrict__ keys, uint32_t mask,
                                 uint32_t* __restrict__ minpos, uint32_t tid, uint32_t nth) {
  const uint32_t lane = tid & 15u;
  for (uint32_t s = tid >> 4; s < n; s += nth >> 4) {
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
__global__ void __launch_bounds__(TPB) tuple_kernel(const uint32_t* __restrict__ off, const wfst_tr* __restrict__ arcs,
                                                    const float* __restrict__ fin, uint32_t n, float delta,
                                                    const uint32_t* __restrict__ off2, wfst_tr* __restrict__ enc,
                                                    unsigned long long* __restrict__ keys, uint32_t mask,
                                                    uint32_t* __restrict__ minpos) {
  tuples_of_states(off, arcs, fin, n, delta, off2, enc, keys, mask, minpos, blockIdx.x * blockDim.x + threadIdx.x,
                   gridDim.x * blockDim.x);
}
__global__ void rank_kernel(wfst_tr* __restrict__ enc, uint32_t e2, const uint32_t* __restrict__ minpos) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < e2) enc[i].olabel = minpos[enc[i].olabel];
}
// label order / topological order of the encoded FST (only asked for when connect leaves nothing): FACT_NOT_I_SORTED (its labels
// are equal pairs, carried in olabel) | FACT_NOT_TOP_SORTED
__device__ uint32_t enc_facts_of_states(const uint32_t* __restrict__ off2, const wfst_tr* __restrict__ enc, uint32_t n,
                                        uint32_t tid, uint32_t nth) {
  const uint32_t lane = tid & 15u;
  uint32_t facts = 0;
  for (uint32_t s = tid >> 4; s < n; s += nth >> 4)
    for (uint32_t i = off2[s] + lane; i < off2[s + 1]; i += 16) {
      if (i > off2[s] && enc[i].olabel < enc[i - 1].olabel) facts |= props::FACT_NOT_I_SORTED;
      if (enc[i].nextstate <= s) facts |= props::FACT_NOT_TOP_SORTED;
    }
  return facts;
}
__global__ void __launch_bounds__(TPB) enc_facts_kernel(const uint32_t* __restrict__ off2, const wfst_tr* __restrict__ enc,
                                                        uint32_t n, uint32_t* __restrict__ out) {
  uint32_t facts = enc_facts_of_states(off2, enc, n, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
  for (int d = 32; d >= 1; d >>= 1) facts |= __shfl_xor(facts, d);
  if ((threadIdx.x & 63) == 0 && facts) atomicOr(out, facts);
}

// ---------------------------------------------------------------- transpose
__global__ void __launch_bounds__(TPB) transpose_fill_kernel(const uint32_t* __restrict__ off, const wfst_tr* __restrict__ arcs,
                                                             uint32_t n, const uint32_t* __restrict__ roff,
                                                             uint32_t* __restrict__ cursor, uint32_t* __restrict__ rsrc) {
  transpose_fill(off, arcs, n, roff, cursor, rsrc, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
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
  uint64_t hmask;   // the bits of a signature's hash that are kept (WFST_MINIMIZE_HASH_BITS; all ones otherwise)
};

__device__ inline void core_init_state(const Core& c, uint32_t s) {
  const uint32_t deg = c.off[s + 1] - c.off[s];
  c.outdeg[s] = deg;
  if (deg == 0) {
    c.order[atomicAdd(&c.ctl[C_TAIL], 1u)] = s;
    atomicMax(&c.ctl[C_CURMAX], s);
  }
}
__global__ void core_init_kernel(Core c) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s < c.n) core_init_state(c, s);
}
__device__ inline void core_advance(const Core& c) {  // one thread
  stg(&c.ctl[C_LO], ld(&c.ctl[C_HI]));
  stg(&c.ctl[C_HI], ld(&c.ctl[C_TAIL]));
  const uint32_t level = ld(&c.ctl[C_LEVEL]) + 1u;
  stg(&c.ctl[C_LEVEL], level);
  if (level > 1) {  // (the first call only opens level 0, whose maximum core_init_state found)
    stg(&c.ctl[C_CURMAX], ld(&c.ctl[C_NEXTMAX]));
    stg(&c.ctl[C_NEXTMAX], 0u);
  }
  stg(&c.ctl[C_WAVE], ld(&c.ctl[C_WAVE]) + ld(&c.ctl[C_NBIG]));
  stg(&c.ctl[C_NBIG], 0u);
}
__global__ void core_advance_kernel(Core c) { core_advance(c); }

__device__ inline uint32_t label_key(const Core& c, const wfst_tr& a) { return c.by_olabel ? a.olabel : a.ilabel; }
__device__ inline uint64_t entry_hash(const Core& c, const wfst_tr& a, uint32_t j) {
  return mix64((((uint64_t)label_key(c, a) << 32) | ld(&c.cls[a.nextstate])) + (uint64_t)(j + 1) * GOLDEN64);
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
    h = mix64(h) & c.hmask;
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
        atomicAdd(&c.ctl[C_UNEQ], 1u);
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
    const uint64_t h = mix64(head_hash(fk, deg) + part) & c.hmask;
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
        if (lane == 0) atomicAdd(&c.ctl[C_UNEQ], 1u);
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
// NARROW: one workgroup (of nth threads), level after level while the level holds at most `narrow_max` states.  sh: three
// words of LDS.  per_level(lo, hi) runs on every thread before the level [lo, hi) of c.order leaves the graph.
template <class F>
__device__ void narrow_levels(const Core& c, uint32_t narrow_max, uint32_t nth, uint32_t* sh, F&& per_level) {
  uint32_t &s_lo = sh[0], &s_hi = sh[1], &s_nbig = sh[2];
  const uint32_t tid = threadIdx.x;
  if (tid == 0) {
    s_lo = ld(&c.ctl[C_LO]);
    s_hi = ld(&c.ctl[C_HI]);
  }
  __syncthreads();
  for (;;) {
    const uint32_t lo = s_lo, hi = s_hi;
    if (hi == lo || hi - lo > narrow_max) break;
    per_level(lo, hi);
    if (c.refine) {
      refine_small(c, lo, hi, tid, nth);
      __threadfence();
      __syncthreads();
      if (tid == 0) s_nbig = ld(&c.ctl[C_NBIG]);
      __syncthreads();
      if (s_nbig) refine_big(c, s_nbig, tid >> 6, nth >> 6, tid & 63u);
      __threadfence();
      __syncthreads();
    }
    assign_peel(c, lo, hi, tid, nth);
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
      stg(&c.ctl[C_WAVE], ld(&c.ctl[C_WAVE]) + ld(&c.ctl[C_NBIG]));
      stg(&c.ctl[C_NBIG], 0u);
    }
    __threadfence();
    __syncthreads();
  }
}
__global__ void __launch_bounds__(NARROW_TPB) narrow_kernel(Core c, uint32_t narrow_max) {
  __shared__ uint32_t sh[3];
  narrow_levels(c, narrow_max, NARROW_TPB, sh, [](uint32_t, uint32_t) {});
}

// ---------------------------------------------------------------- emit
// the unweighted branch compares no weights (minimize.rs:389-456), merge_states appends the members' arcs to the survivor
// and tr_unique drops those EQUAL to the survivor's (Tr's ==: approximate on the weight).  Flag a member arc that would stay.
__device__ inline bool weights_far(const Core& c, uint32_t s) {
  const uint32_t r = c.cls[s];
  if (r == s) return false;
  const uint32_t b = c.off[s], rb = c.off[r], deg = c.off[s + 1] - b;
  bool bad = false;
  for (uint32_t j = 0; j < deg; ++j) bad |= !weq(c.arcs[b + j].weight, c.arcs[rb + j].weight);
  return bad;
}
__global__ void weight_check_kernel(Core c, uint32_t* __restrict__ flag) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s < c.n && weights_far(c, s)) atomicOr(flag, 1u);
}
// keep[s]: s survives (the superfinal state of the weighted branch, the last state, goes); s <= n
__device__ inline uint32_t keeps(const uint32_t* __restrict__ cls, uint32_t n, uint32_t superfinal, uint32_t s) {
  return (s < n && cls[s] == s && s != superfinal) ? 1u : 0u;
}
__global__ void keep_kernel(const uint32_t* __restrict__ cls, uint32_t n, uint32_t superfinal, uint32_t* __restrict__ keep) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s <= n) keep[s] = keeps(cls, n, superfinal, s);
}
// arcs the survivor keeps: all but the one into the superfinal state
__device__ void emit_count(const uint32_t* __restrict__ off, const wfst_tr* __restrict__ arcs, uint32_t n, uint32_t superfinal,
                           const uint32_t* __restrict__ keep, const uint32_t* __restrict__ new_id, uint32_t* __restrict__ cnt,
                           uint32_t tid, uint32_t nth) {
  const uint32_t lane = tid & 15u;
  for (uint32_t s = tid >> 4; s < n; s += nth >> 4) {
    if (!keep[s]) continue;  // (uniform over the 16 lanes)
    uint32_t k = 0;
    for (uint32_t i = off[s] + lane; i < off[s + 1]; i += 16) k += arcs[i].nextstate != superfinal;
    for (int d = 8; d >= 1; d >>= 1) k += __shfl_xor(k, d, 16);
    if (lane == 0) cnt[new_id[s]] = k;
  }
}
__global__ void __launch_bounds__(TPB) emit_count_kernel(const uint32_t* __restrict__ off, const wfst_tr* __restrict__ arcs,
                                                         uint32_t n, uint32_t superfinal, const uint32_t* __restrict__ keep,
                                                         const uint32_t* __restrict__ new_id, uint32_t* __restrict__ cnt) {
  emit_count(off, arcs, n, superfinal, keep, new_id, cnt, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}
// the survivor's arcs in their sorted order, redirected to survivors' new ids; weighted branch (enc != null): label and
// weight decoded from the first occurrence of the tuple (its scan position sits in olabel), the arc into the superfinal state
// becomes the final weight: zero (+) (final(superfinal) = one (x) w) (rm_final_epsilon.rs:45-60)
__device__ void emit_states(const uint32_t* __restrict__ off, const wfst_tr* __restrict__ arcs, const float* __restrict__ fin,
                            uint32_t n, uint32_t superfinal, const uint32_t* __restrict__ keep,
                            const uint32_t* __restrict__ new_id, const uint32_t* __restrict__ cls,
                            const wfst_tr* __restrict__ enc, const uint32_t* __restrict__ off_out,
                            wfst_tr* __restrict__ arcs_out, float* __restrict__ fin_out, uint32_t tid, uint32_t nth) {
  const uint32_t lane = tid & 15u;
  for (uint32_t s = tid >> 4; s < n; s += nth >> 4) {
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
__global__ void __launch_bounds__(TPB) emit_kernel(const uint32_t* __restrict__ off, const wfst_tr* __restrict__ arcs,
                                                   const float* __restrict__ fin, uint32_t n, uint32_t superfinal,
                                                   const uint32_t* __restrict__ keep, const uint32_t* __restrict__ new_id,
                                                   const uint32_t* __restrict__ cls, const wfst_tr* __restrict__ enc,
                                                   const uint32_t* __restrict__ off_out, wfst_tr* __restrict__ arcs_out,
                                                   float* __restrict__ fin_out) {
  emit_states(off, arcs, fin, n, superfinal, keep, new_id, cls, enc, off_out, arcs_out, fin_out,
              blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}

// ---------------------------------------------------------------- host side
// WFST_MINIMIZE_HASH_BITS=n (0 <= n <= 64; tests): refine_small / refine_big keep the low n bits of a signature's hash, so
// that different signatures meet in one slot with one tag and the full compare decides.  The mask of the bits kept.
uint64_t hash_mask_knob() {
  const char* e = std::getenv("WFST_MINIMIZE_HASH_BITS");
  if (!e || !*e) return ~0ull;
  char* end = nullptr;
  const unsigned long v = std::strtoul(e, &end, 10);
  if (*e < '0' || *e > '9' || *end || std::strlen(e) > 2 || v > 64)
    throw Error(std::string("WFST_MINIMIZE_HASH_BITS: expected a number from 0 to 64, not '") + e + "'");
  return v == 64 ? ~0ull : (1ull << v) - 1ull;
}
struct Knobs {
  Path path;
  uint64_t hmask;
};

uint32_t grid16(wfst_ctx* ctx, uint32_t n) {  // 16 lanes per state
  return std::max<uint32_t>(1, std::min<uint32_t>((n + 15) / 16, (uint32_t)ctx->n_cus * 32));
}
// (the scratch goes back to the pool at once: synchronise first)
void scan_sync(wfst_ctx* ctx, const uint32_t* in, uint32_t* out, size_t count) {
  const DBuf<uint8_t> temp = exclusive_scan_u32(ctx, in, out, count);
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
}

// ---- the property word and the checks on it, step by step: minimize_fst and, for the batch call, minimize_batch_verdict
// compute_and_update_properties(ACCEPTOR | I_DETERMINISTIC | WEIGHTED | UNWEIGHTED) (:101-106) asks the content when the
// stored word does not know all of them (compute_fst_properties.rs:22-28)
bool word_needs_facts(uint64_t p) {
  using namespace props;
  return !(knows(p, ACCEPTOR) && knows(p, I_DETERMINISTIC) && knows(p, WEIGHTED));
}
uint64_t word_with_facts(uint64_t p, uint32_t bits, bool nondet) {
  return props::merge_computed(p, props::content_props(bits) | (nondet ? props::NOT_I_DETERMINISTIC : props::I_DETERMINISTIC));
}
// the KO the word decides (:107-118), or null
const char* refused_by_word(uint64_t p, bool allow_nondet) {
  using namespace props;
  if (!(p & I_DETERMINISTIC) && !allow_nondet) return MSG_REFUSE_NONDET;
  if (!(p & ACCEPTOR)) return MSG_TRANSDUCER;
  if (!(p & I_DETERMINISTIC)) return MSG_NONDET;
  return nullptr;
}
// unweighted branch: the word connect leaves (:193).  computed_dfs: the DFS pairs, the arc scan's pairs (no determinism: not
// in the mask) and UNWEIGHTED_CYCLES were computed; ACCESSIBLE / COACCESSIBLE: connect overwrites both pairs
// (connect.rs:61-64), so their computed values never show.  Then del_states' mask and ACCESSIBLE | COACCESSIBLE.
uint64_t unweighted_connect_word(uint64_t p, bool computed_dfs, uint32_t bits) {
  using namespace props;
  if (computed_dfs)
    p = merge_computed(p, content_props(bits) | ACYCLIC | INITIAL_ACYCLIC | ACCESSIBLE | COACCESSIBLE | UNWEIGHTED_CYCLES);
  return delete_states(p) | ACCESSIBLE | COACCESSIBLE;
}
// ... and the result's, from the connected machine's (pc) after tr_sort(ILabelCompare) (:201)
uint64_t unweighted_result_word(uint64_t pc, bool has_arcs) {
  using namespace props;
  const uint64_t pd = tr_sort_props(pc, true);
  // merge_states: every class with arcs rewrites its representative's arcs through set_nextstate_unchecked, whose mask
  // (trs_iter_mut.rs:293-305) keeps the ACCEPTOR, epsilon and WEIGHTED pairs only; add_tr, set_start, connect and
  // tr_unique (mutate_properties.rs:43-100, 7-13; tr_unique.rs:45-50) add no positive bit of those pairs and connect's
  // mask drops every negative one
  if (has_arcs) return pd & (ACCEPTOR | NO_EPSILONS | NO_I_EPSILONS | NO_O_EPSILONS | UNWEIGHTED);
  // one final state: no arc is touched; set_start, connect, tr_unique
  return (delete_states(set_start(pd)) | ACCESSIBLE | COACCESSIBLE) & ARCSORT_MASK & DELETE_ARCS_MASK;
}
// weighted input without a start state: compute_and_update_properties(ACCEPTOR | UNWEIGHTED | ACYCLIC) (:185-187) on the
// pushed content: the DFS pairs (acyclic: checked before; no start state, so nothing is accessible; COACCESSIBLE is
// overwritten by connect) and the arc scan's pairs.  NOT_ACCEPTOR or WEIGHTED in it: "FST is not an unweighted acceptor".
uint64_t startless_computed_word(uint32_t pushed_bits) {
  using namespace props;
  return content_props(pushed_bits) | ACYCLIC | INITIAL_ACYCLIC | NOT_ACCESSIBLE | COACCESSIBLE | UNWEIGHTED_CYCLES;
}
uint64_t startless_result_word(uint64_t pushed_word, uint64_t comp) {
  using namespace props;
  return delete_states(merge_computed(pushed_word & ALL, comp)) | ACCESSIBLE | COACCESSIBLE;
}
// weighted, nothing reaches a final state: the encoded FST's computed word (compute_fst_properties on its content: labels
// >= 1, weights one, acyclic) through connect's mask; decode's tr_map returns at once, rm_final_epsilon connects again
uint64_t empty_encoded_word(uint32_t enc_bits) {
  using namespace props;
  uint64_t comp = ACCEPTOR | NO_EPSILONS | NO_I_EPSILONS | NO_O_EPSILONS | UNWEIGHTED | ACYCLIC | INITIAL_ACYCLIC | UNWEIGHTED_CYCLES;
  if (!(enc_bits & FACT_NOT_I_SORTED)) comp |= I_LABEL_SORTED | O_LABEL_SORTED;
  if (!(enc_bits & FACT_NOT_TOP_SORTED)) comp |= TOP_SORTED;
  return delete_states(comp) | ACCESSIBLE | COACCESSIBLE;
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
// heights (and, with `refine`, the classes) of the graph (off, arcs, fin) with n states and E arcs.  The route is tallied
// from the control block every host step reads back anyway (wfst_ctx_get_minimize_stats): into the cycle check's counters
// without `refine`, else into the refinement's.
void run_core(wfst_ctx* ctx, CoreBufs& B, uint32_t n, uint64_t E, const uint32_t* off, const wfst_tr* arcs, const float* fin,
              bool refine, bool by_olabel, Knobs knobs) {
  const Path path = knobs.path;
  wfst_ctx::MinimizeStats& tally = ctx->min_stats;
  wfst_ctx::MinimizeStats::Pass& pass = refine ? tally.refine : tally.check;
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
  c.hmask = knobs.hmask;
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
  bool from_narrow = false;  // the block read next is what a narrow launch left
  for (;;) {
    HIP_CHECK(hipMemcpyAsync(h, B.ctl.p, sizeof(h), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    const uint32_t cnt = h[C_HI] - h[C_LO];
    pass.levels = h[C_LEVEL] - 1u;  // (C_LEVEL: 1 + the levels that left the graph; an empty one never does)
    if (refine) {
      tally.wave_states = h[C_WAVE];
      tally.unequal_compares = h[C_UNEQ];
    }
    if (from_narrow) ++(cnt == 0 ? pass.exit_done : pass.exit_wide);
    from_narrow = false;
    if (cnt == 0) break;
    if (path != Path::Wide && cnt <= narrow_max) {
      narrow_kernel<<<1, NARROW_TPB, 0, st>>>(c, narrow_max);
      ++pass.narrow_launches;
      from_narrow = true;
    } else {
      const uint32_t cap = (uint32_t)ctx->n_cus * 16;
      if (refine) {
        wide_small_kernel<<<std::max(1u, std::min((cnt + TPB - 1) / TPB, cap)), TPB, 0, st>>>(c);
        wide_big_kernel<<<std::max(1u, std::min((cnt + 3) / 4, cap)), TPB, 0, st>>>(c);
      }
      wide_peel_kernel<<<std::max(1u, std::min((cnt + 15) / 16, cap)), TPB, 0, st>>>(c);
      core_advance_kernel<<<1, 1, 0, st>>>(c);
      ++pass.wide_levels;
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
wfst_fst* minimize_connected(wfst_ctx* ctx, const wfst_fst* T, const wfst_tr* enc, uint64_t out_props, Knobs knobs) {
  hipStream_t st = ctx->stream;
  DevicePool& pool = *ctx->pool;
  const uint32_t n = T->n_states;
  const uint64_t E = T->n_arcs;
  const uint32_t superfinal = enc ? n - 1 : NONE;
  CoreBufs B;
  run_core(ctx, B, n, E, T->dev.offsets, T->dev.arcs, T->dev.finals, true, enc != nullptr, knobs);
  if (B.peeled != n) throw Error(MSG_CYCLIC);
  if (!enc && E) {
    DBuf<uint32_t> flag(pool, 1);
    HIP_CHECK(hipMemsetAsync(flag.p, 0, sizeof(uint32_t), st));
    weight_check_kernel<<<(n + TPB - 1) / TPB, TPB, 0, st>>>(B.c, flag.p);
    HIP_CHECK(hipGetLastError());
    if (read_u32(ctx, flag.p))
      throw Error(MSG_FAR_APART);
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
bool has_cycle(wfst_ctx* ctx, const wfst_fst* f, Knobs knobs) {
  if (f->n_states == 0) return false;
  CoreBufs B;
  run_core(ctx, B, f->n_states, f->n_arcs, f->dev.offsets, f->dev.arcs, f->dev.finals, false, false, knobs);
  return B.peeled != f->n_states;
}

}  // namespace

// minimize_with_config (minimize.rs:92-176) for the acyclic deterministic acceptor branch: a NEW handle
wfst_fst* minimize_fst(wfst_ctx* ctx, const wfst_fst* f, float delta, bool allow_nondet) {
  using namespace props;
  wfst_ctx::MinimizeStats& tally = ctx->min_stats;  // (wfst_ctx_get_minimize_stats: this call's, also when it ends KO)
  tally = wfst_ctx::MinimizeStats{};
  const Knobs knobs{path_knob("WFST_MINIMIZE_PATH"), hash_mask_knob()};
  hipStream_t st = ctx->stream;
  DevicePool& pool = *ctx->pool;
  ensure_device(const_cast<wfst_fst*>(f));
  const uint32_t n = f->n_states;
  uint64_t p = f->props & ALL;
  Facts fa;
  // compute_and_update_properties(ACCEPTOR | I_DETERMINISTIC | WEIGHTED | UNWEIGHTED) (:101-106): the stored word if it
  // knows all of them (compute_fst_properties.rs:22-28), else everything the arc scan finds
  if (word_needs_facts(p)) {
    content_facts(ctx, f, fa);
    content_idet(ctx, f, fa);
    p = word_with_facts(p, fa.bits, fa.nondet);
  }
  if (const char* msg = refused_by_word(p, allow_nondet)) throw Error(msg);

  // ACYCLIC, as acceptor_minimize's compute_and_update_properties finds it on the UNTRIMMED FST (:185-187, 198): stored, or
  // computed.  Any cycle is KO here, also one that connect would remove (the reference takes Hopcroft's branch then).
  bool computed_dfs = false;
  if (!knows(p, CYCLIC)) {
    if (has_cycle(ctx, f, knobs)) throw Error(MSG_CYCLIC);
    computed_dfs = true;
  } else if (p & CYCLIC) {
    throw Error(MSG_CYCLIC);
  }

  if (!(p & WEIGHTED)) {
    // ---- unweighted acceptor (:172-175): acceptor_minimize on the original labels
    if (n) tally.branch = 1;
    if (computed_dfs) content_facts(ctx, f, fa);
    const uint64_t pc = unweighted_connect_word(p, computed_dfs, fa.bits);  // connect (:193)
    Handle T(connect_and_adopt(ctx, n, f->start, f->dev.offsets, f->dev.arcs, f->dev.finals, /*all_accessible=*/false, pc));
    if (T->n_states == 0) {  // (:195-197)
      if (n) tally.branch = 4;
      return T.release();
    }
    tr_sort_device(ctx, T.get(), true);         // tr_sort(ILabelCompare) (:201)
    return minimize_connected(ctx, T.get(), nullptr, unweighted_result_word(pc, T->n_arcs != 0), knobs);
  }

  // ---- weighted acceptor (:162-171)
  if (n) tally.branch = 2;
  if (f->start < 0) {
    if (n) tally.branch = 3;
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
    const uint64_t comp = startless_computed_word(pf.bits);
    if (comp & (NOT_ACCEPTOR | WEIGHTED)) throw Error(MSG_NOT_UNWEIGHTED);  // (:188-190)
    return empty_fst(ctx, startless_result_word(P->props, comp));
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
    tally.branch = 4;
    DBuf<uint32_t> out(pool, 1);  // nothing reaches a final state
    HIP_CHECK(hipMemsetAsync(out.p, 0, sizeof(uint32_t), st));
    enc_facts_kernel<<<grid16(ctx, np + 1), TPB, 0, st>>>(off2.p, enc.p, np + 1, out.p);
    HIP_CHECK(hipGetLastError());
    return empty_fst(ctx, empty_encoded_word(read_u32(ctx, out.p)));
  }
  tr_sort_device(ctx, T.get(), false);  // tr_sort(ILabelCompare) on the encode labels (olabel carries their order)
  // decode's mapper keeps none of the bits tr_unique leaves (decode_static.rs:52-66); rm_final_epsilon's set_final /
  // del_trs pairs end in delete_trs_properties and connect (rm_final_epsilon.rs:62-75): ACCESSIBLE | COACCESSIBLE
  return minimize_connected(ctx, T.get(), enc.p, ACCESSIBLE | COACCESSIBLE, knobs);
}

// ================================================================ batch (wfst_minimize_batch)
// One workgroup per item, ONE launch for the whole list: the workgroup runs every stage of minimize_fst above on its item,
// inside the item's slice of one slab, as workgroup-local passes separated by barriers.  The stages are the device
// functions the single path's kernels are made of (facts_of_states, idet_of_states, transpose_fill, narrow_levels,
// tuples_of_states, weights_far, keeps, emit_count, emit_states); what the single path gets from other files is restated
// for one workgroup here: the reverse distances (on a DAG: one pass in peeling order), push.hip's reweight rules, connect
// (two frontier searches) and tr_sort's stable order (a rank sort fused with connect's compaction).
namespace {

constexpr uint32_t MB_MAX_STATES = 4096;    // the in_kernel rule (include/wfst.h)
constexpr uint32_t MB_MAX_ARCS = 16384;
constexpr size_t MB_MAX_SLAB = (size_t)8 << 30;  // all slices of a call together (include/wfst.h); beyond: KO before any launch
constexpr uint32_t MB_GROUP_MAX_DEG = 64;   // connect + sort: 16 lanes per state up to here, the whole workgroup beyond
// exit codes of an item (MbCtl::exit)
enum : uint32_t { MB_RUNNING = 0, MB_DONE = 1, MB_EMPTY = 2, MB_EMPTY_NO_START = 3, MB_KO_FACTS = 4, MB_KO_CYCLIC = 5, MB_KO_FAR_APART = 6 };
// what the host knows from the stored word (MbItem::known)
enum : uint32_t { MBK_FACTS = 1, MBK_ACCEPTOR = 2, MBK_IDET = 4, MBK_WEIGHTED = 8, MBK_CYCLIC_KNOWN = 16, MBK_CYCLIC = 32 };

struct MbCtl {  // one per item, at the head of the slab; read back once
  uint32_t exit;
  uint32_t bits;         // facts of the input's content (props::FACT_*)
  uint32_t nondet;       // some state has two arcs with one ilabel (only computed without MBK_FACTS)
  uint32_t weighted;     // the branch taken
  uint32_t push_facts;   // reweight: 1 = an arc went through set_weight, 2 = a final weight through set_final
  uint32_t pushed_bits;  // facts of the pushed content (weighted, no start state)
  uint32_t enc_bits;     // FACT_NOT_I_SORTED | FACT_NOT_TOP_SORTED of the encoded FST (weighted, nothing left after connect)
  uint32_t t_arcs;       // arcs of the connected machine
  uint32_t n_out, e_out, start_out;
  uint32_t pad;
};
struct MbItem {
  const uint32_t* off;
  const wfst_tr* arcs;
  const float* fin;
  uint32_t n, E, start /* NONE: no start state */, known;
  float delta;
  uint32_t tsize, ssize;  // slots of keys / of tab
  MbCtl* ctl;
  // the slice; N1 = n + 1 states and E2 = E + n arcs bound the encoded machine
  uint32_t* cctl;       // [C_WORDS] the Core's control words
  uint32_t *roff, *rcnt, *rsrc;  // [N1 + 1], [N1 + 1], [E2]: the transpose (of the input, then of the connected machine)
  uint32_t *outdeg, *order;      // [N1]
  float* d;                      // [n] reverse distances
  uint32_t *acc, *co;            // [N1 + 1] reached from the start / reaches a final state; then keep flags
  uint32_t *new_id, *off2;       // [N1 + 1], [N1 + 1]
  wfst_tr *enc, *tarcs;          // [E2] the encoded arcs; the pushed arcs, then the connected and sorted machine
  float* tfin;                   // [N1] the pushed final weights, then the connected machine's
  uint32_t* toff;                // [N1 + 1]
  unsigned long long* keys;      // [tsize] (state, ilabel) pairs, then the tuples
  uint32_t* minpos;              // [tsize]
  uint32_t *cls, *slot_of, *big; // [N1]
  unsigned long long* tab;       // [ssize]
  uint32_t *smin, *smax;         // [ssize]
  uint32_t *keep, *new_id2, *cnt;  // [N1 + 1]
  uint32_t* off_out;             // [N1 + 1] the result
  wfst_tr* arcs_out;             // [E2]
  float* fin_out;                // [N1]
};

__device__ inline float ldf(const float* p) { return __uint_as_float(ld((const uint32_t*)p)); }
__device__ inline void stf(float* p, float v) { stg((uint32_t*)p, __float_as_uint(v)); }
// the state's kept arcs (those into kept states) to their places in tr_sort's stable order: rank by (label key, position)
// among the kept ones.  Lane `lane` of `g` lanes.
__device__ void place_sorted(const wfst_tr* sarcs, uint32_t b, uint32_t deg, const uint32_t* keep, const uint32_t* new_id,
                             uint32_t by_olabel, wfst_tr* out, uint32_t lane, uint32_t g) {
  for (uint32_t i = lane; i < deg; i += g) {
    const wfst_tr a = sarcs[b + i];
    if (!keep[a.nextstate]) continue;
    const uint64_t k = ((uint64_t)(by_olabel ? a.olabel : a.ilabel) << 32) | i;
    uint32_t rank = 0;
    for (uint32_t j = 0; j < deg; ++j) {
      const wfst_tr o = sarcs[b + j];
      rank += (keep[o.nextstate] && ((((uint64_t)(by_olabel ? o.olabel : o.ilabel)) << 32) | j) < k) ? 1u : 0u;
    }
    out[rank] = wfst_tr{a.ilabel, a.olabel, a.weight, new_id[a.nextstate]};
  }
}

__global__ void __launch_bounds__(MB_TPB) minimize_batch_kernel(const MbItem* __restrict__ items) {
  __shared__ uint32_t part[MB_TPB + 1];
  __shared__ uint32_t sh[3];   // narrow_levels / wg_search
  __shared__ uint32_t s_bits, s_flag, s_nbig;
  const MbItem it = items[blockIdx.x];
  const uint32_t tid = threadIdx.x, lane = tid & 15u;
  const uint32_t n = it.n, E = it.E;
  MbCtl* ctl = it.ctl;
  auto leave = [&](uint32_t code) {
    if (tid == 0) ctl->exit = code;
  };
  // ---- 1. facts of the content
  if (tid == 0) s_bits = s_flag = s_nbig = 0;
  if (!(it.known & MBK_FACTS)) wg_fill64(it.keys, it.tsize, EMPTY_KEY);
  wg_bar();
  {
    uint32_t facts = facts_of_states(it.off, it.arcs, it.fin, n, tid, MB_TPB);
    for (int d = 32; d >= 1; d >>= 1) facts |= __shfl_xor(facts, d);
    if ((tid & 63) == 0 && facts) atomicOr(&s_bits, facts);
    if (!(it.known & MBK_FACTS) && idet_of_states(it.off, it.arcs, n, it.keys, it.tsize - 1, tid, MB_TPB)) atomicOr(&s_flag, 1u);
  }
  wg_bar();
  const uint32_t bits = s_bits, nondet = s_flag;
  bool acceptor, idet, weighted_in;
  if (it.known & MBK_FACTS) {
    acceptor = it.known & MBK_ACCEPTOR;
    idet = it.known & MBK_IDET;
    weighted_in = it.known & MBK_WEIGHTED;
  } else {
    acceptor = !(bits & props::FACT_NOT_ACCEPTOR);
    idet = !nondet;
    weighted_in = bits & (props::FACT_WEIGHTED | props::FACT_FINAL_WEIGHTED);
  }
  if (tid == 0) {
    ctl->bits = bits;
    ctl->nondet = nondet;
    ctl->weighted = weighted_in ? 1u : 0u;
  }
  if (!acceptor || !idet) return leave(MB_KO_FACTS);
  if ((it.known & MBK_CYCLIC_KNOWN) && (it.known & MBK_CYCLIC)) return leave(MB_KO_CYCLIC);
  __syncthreads();  // (s_flag is reused below)

  // ---- 2. the transpose of the input; acyclicity and reverse distances by peeling sinks
  wg_transpose(it.off, it.arcs, n, E, it.roff, it.rcnt, it.rsrc, part);
  if (weighted_in || !(it.known & MBK_CYCLIC_KNOWN)) {
    Core c{};
    c.off = it.off;
    c.arcs = it.arcs;
    c.fin = it.fin;
    c.n = n;
    c.roff = it.roff;
    c.rsrc = it.rsrc;
    c.outdeg = it.outdeg;
    c.order = it.order;
    c.ctl = it.cctl;
    c.hmask = ~0ull;
    wg_fill(it.cctl, C_WORDS, 0u);
    if (weighted_in) wg_fill((uint32_t*)it.d, n, __float_as_uint(INF));
    wg_bar();
    for (uint32_t s = tid; s < n; s += MB_TPB) core_init_state(c, s);
    wg_bar();
    if (tid == 0) core_advance(c);
    wg_bar();
    // d[s] = final[s] (+) (+)_arcs w (x) d[next]: the successors left the graph in earlier levels
    narrow_levels(c, NONE, MB_TPB, sh, [&](uint32_t lo, uint32_t hi) {
      if (!weighted_in) return;
      for (uint32_t k = lo + tid; k < hi; k += MB_TPB) {
        const uint32_t s = ld(&c.order[k]);
        float best = it.fin[s];
        for (uint32_t i = it.off[s]; i < it.off[s + 1]; ++i) best = wplus(best, wtimes(it.arcs[i].weight, ldf(&it.d[it.arcs[i].nextstate])));
        stf(&it.d[s], best);
      }
    });
    if (!(it.known & MBK_CYCLIC_KNOWN) && ld(&it.cctl[C_TAIL]) != n) return leave(MB_KO_CYCLIC);
  }

  const wfst_tr* sarcs = it.arcs;  // the machine connect works on
  const uint32_t* soff = it.off;
  uint32_t n1 = n;
  if (weighted_in) {
    // ---- 3. push_weights(ToInitial) (push.hip reweight_arcs_kernel / reweight_finals_kernel and the start-state step of
    // reweight_device: the input is acyclic, so the start state's own arcs and final weight take the factor)
    const float d_start = it.start != NONE ? ldf(&it.d[it.start]) : INF;
    const bool start_step = it.start != NONE && !is_one(d_start) && !is_zero(d_start);
    uint32_t pf = 0;
    for (uint32_t s = tid >> 4; s < n; s += MB_TPB >> 4) {
      const float d_s = ldf(&it.d[s]);
      const bool skip = is_zero(d_s);
      for (uint32_t i = it.off[s] + lane; i < it.off[s + 1]; i += 16) {
        wfst_tr a = it.arcs[i];
        if (!skip) {
          const float d_ns = ldf(&it.d[a.nextstate]);
          if (!is_zero(d_ns)) {
            a.weight = wdivide(wtimes(a.weight, d_ns), d_s);
            pf |= 1u;
          }
        }
        if (start_step && s == it.start) a.weight = wtimes(d_start, a.weight);
        it.tarcs[i] = a;
      }
      if (lane == 0) {
        float f = it.fin[s];
        if (f != INF && !skip) {
          f = wdivide(f, d_s);
          pf |= 2u;
        }
        if (start_step && s == it.start && f != INF) f = wtimes(d_start, f);
        it.tfin[s] = f;
      }
    }
    for (int d = 32; d >= 1; d >>= 1) pf |= __shfl_xor(pf, d);
    if ((tid & 63) == 0 && pf) atomicOr(&s_flag, pf);
    wg_fill64(it.keys, it.tsize, EMPTY_KEY);
    wg_fill(it.minpos, it.tsize, NONE);
    wg_bar();
    if (tid == 0) ctl->push_facts = s_flag;
    if (it.start == NONE) {  // no quantization, no encoding: the host decides from the pushed content
      uint32_t facts = facts_of_states(it.off, it.tarcs, it.tfin, n, tid, MB_TPB);
      if (facts) atomicOr(&ctl->pushed_bits, facts);
      return leave(MB_EMPTY_NO_START);
    }
    // ---- 4. quantize + encode: off2 = the offsets with one more arc per final state, state n = the superfinal state
    for (uint32_t s = tid; s < n + 2; s += MB_TPB) it.off2[s] = (s < n && it.tfin[s] != INF) ? 1u : 0u;
    wg_bar();
    wg_exclusive_scan(it.off2, it.off2, n + 2, part);
    for (uint32_t s = tid; s <= n; s += MB_TPB) {
      const uint32_t v = it.off[s] + it.off2[s];
      it.off2[s] = v;
      if (s == n) it.off2[n + 1] = v;
    }
    wg_bar();
    const uint32_t e2 = it.off2[n];
    tuples_of_states(it.off, it.tarcs, it.tfin, n, it.delta, it.off2, it.enc, it.keys, it.tsize - 1, it.minpos, tid, MB_TPB);
    wg_bar();
    for (uint32_t i = tid; i < e2; i += MB_TPB) it.enc[i].olabel = it.minpos[it.enc[i].olabel];
    wg_bar();
    sarcs = it.enc;
    soff = it.off2;
    n1 = n + 1;
  }

  // ---- 5. connect: reached from the start and reaching a final state, on the input's graph (the superfinal state stays
  // exactly when anything does)
  wg_fill(it.acc, n1 + 1, 0u);
  wg_fill(it.co, n1 + 1, 0u);
  if (tid == 0) sh[2] = 0;
  wg_bar();
  if (it.start != NONE) {
    if (tid == 0) {
      it.acc[it.start] = 1u;
      it.order[0] = it.start;
      sh[2] = 1;
    }
    wg_bar();
    wg_search(it.off, it.arcs, nullptr, it.acc, it.order, sh);
    if (tid == 0) sh[2] = 0;
    wg_bar();
    for (uint32_t s = tid; s < n; s += MB_TPB)
      if (it.fin[s] != INF) {
        it.co[s] = 1u;
        it.order[atomicAdd(&sh[2], 1u)] = s;
      }
    wg_bar();
    wg_search(it.roff, nullptr, it.rsrc, it.co, it.order, sh);
  }
  // keep flags (in co) and the new ids
  for (uint32_t s = tid; s <= n1; s += MB_TPB) {
    uint32_t k = 0;
    if (s < n) k = ld(&it.acc[s]) & ld(&it.co[s]);
    else if (s == n && weighted_in) k = (it.start != NONE) ? (ld(&it.acc[it.start]) & ld(&it.co[it.start])) : 0u;
    it.keep[s] = k;
  }
  wg_bar();
  const uint32_t tn = wg_exclusive_scan(it.keep, it.new_id, n1 + 1, part);
  if (tn == 0) {  // nothing reaches a final state
    if (weighted_in) {
      uint32_t facts = enc_facts_of_states(soff, sarcs, n1, tid, MB_TPB);
      if (facts) atomicOr(&ctl->enc_bits, facts);
    }
    return leave(MB_EMPTY);
  }
  // arcs a kept state keeps, the offsets, the final weights
  wg_fill(it.cnt, tn + 1, 0u);
  wg_bar();
  for (uint32_t s = tid >> 4; s < n1; s += MB_TPB >> 4) {
    if (!it.keep[s]) continue;
    uint32_t k = 0;
    for (uint32_t i = soff[s] + lane; i < soff[s + 1]; i += 16) k += it.keep[sarcs[i].nextstate];
    for (int d = 8; d >= 1; d >>= 1) k += __shfl_xor(k, d, 16);
    if (lane == 0) {
      const uint32_t ns = it.new_id[s];
      it.cnt[ns] = k;
      it.tfin[ns] = weighted_in ? (s == n ? 0.0f : INF) : it.fin[s];  // (ns <= s, and tfin[s] of the pushed FST is done with)
    }
  }
  wg_bar();
  const uint32_t te = wg_exclusive_scan(it.cnt, it.toff, tn + 1, part);
  // ---- 6. the kept arcs in tr_sort's order (on ilabel; weighted: on the encode rank in olabel)
  for (uint32_t s = tid >> 4; s < n1; s += MB_TPB >> 4) {
    if (!it.keep[s]) continue;
    const uint32_t b = soff[s], deg = soff[s + 1] - b;
    if (deg > MB_GROUP_MAX_DEG) {
      if (lane == 0) it.big[atomicAdd(&s_nbig, 1u)] = s;
      continue;
    }
    place_sorted(sarcs, b, deg, it.keep, it.new_id, weighted_in, it.tarcs + it.toff[it.new_id[s]], lane, 16);
  }
  wg_bar();
  for (uint32_t k = 0; k < s_nbig; ++k) {
    const uint32_t s = it.big[k];
    place_sorted(sarcs, soff[s], soff[s + 1] - soff[s], it.keep, it.new_id, weighted_in, it.tarcs + it.toff[it.new_id[s]], tid, MB_TPB);
  }
  wg_bar();
  const uint32_t t_start = it.new_id[it.start];

  // ---- 7. heights by peeling, fused with the refinement (the narrow regime of the single path)
  wg_transpose(it.toff, it.tarcs, tn, te, it.roff, it.rcnt, it.rsrc, part);
  uint32_t size = 64;
  while (size < 2 * tn) size *= 2;
  Core c{};
  c.off = it.toff;
  c.arcs = it.tarcs;
  c.fin = it.tfin;
  c.n = tn;
  c.roff = it.roff;
  c.rsrc = it.rsrc;
  c.outdeg = it.outdeg;
  c.order = it.order;
  c.ctl = it.cctl;
  c.cls = it.cls;
  c.slot_of = it.slot_of;
  c.tab = it.tab;
  c.smin = it.smin;
  c.smax = it.smax;
  c.tmask = size - 1;
  c.big = it.big;
  c.by_olabel = weighted_in ? 1u : 0u;
  c.refine = 1u;
  c.hmask = ~0ull;
  wg_fill(it.cctl, C_WORDS, 0u);
  wg_fill64(it.tab, size, 0ull);
  wg_fill(it.smin, size, NONE);
  wg_fill(it.smax, size, 0u);
  wg_bar();
  for (uint32_t s = tid; s < tn; s += MB_TPB) core_init_state(c, s);
  wg_bar();
  if (tid == 0) core_advance(c);
  wg_bar();
  narrow_levels(c, NONE, MB_TPB, sh, [](uint32_t, uint32_t) {});
  if (ld(&it.cctl[C_TAIL]) != tn) return leave(MB_KO_CYCLIC);

  // ---- 8. the far-apart-weights check, survivors, emit
  const uint32_t superfinal = weighted_in ? tn - 1 : NONE;
  if (tid == 0) s_flag = 0;
  __syncthreads();
  if (!weighted_in && te)
    for (uint32_t s = tid; s < tn; s += MB_TPB)
      if (weights_far(c, s)) atomicOr(&s_flag, 1u);
  for (uint32_t s = tid; s <= tn; s += MB_TPB) it.keep[s] = keeps(it.cls, tn, superfinal, s);
  wg_bar();
  if (s_flag) return leave(MB_KO_FAR_APART);
  const uint32_t n_out = wg_exclusive_scan(it.keep, it.new_id2, tn + 1, part);
  wg_fill(it.cnt, n_out + 1, 0u);
  wg_bar();
  emit_count(it.toff, it.tarcs, tn, superfinal, it.keep, it.new_id2, it.cnt, tid, MB_TPB);
  wg_bar();
  const uint32_t e_out = wg_exclusive_scan(it.cnt, it.off_out, n_out + 1, part);
  emit_states(it.toff, it.tarcs, it.tfin, tn, superfinal, it.keep, it.new_id2, it.cls, weighted_in ? it.enc : nullptr, it.off_out,
              it.arcs_out, it.fin_out, tid, MB_TPB);
  if (tid == 0) {
    ctl->t_arcs = te;
    ctl->n_out = n_out;
    ctl->e_out = e_out;
    ctl->start_out = it.new_id2[it.cls[t_start]];
    ctl->exit = MB_DONE;
  }
}

// carves one item's arrays out of the slab, every array 64-byte aligned; it == nullptr only measures
size_t carve_minimize_slice(Slab s, uint32_t n, uint32_t E, MbItem* it) {
  const size_t N1 = (size_t)n + 1, E2 = (size_t)E + n;
  const uint32_t tsize = pow2_at_least(2 * E2, "minimize_batch"), ssize = pow2_at_least(2 * N1, "minimize_batch");
  MbItem v{};
  v.cctl = s.take<uint32_t>(C_WORDS);
  v.roff = s.take<uint32_t>(N1 + 1);
  v.rcnt = s.take<uint32_t>(N1 + 1);
  v.rsrc = s.take<uint32_t>(E2);
  v.outdeg = s.take<uint32_t>(N1);
  v.order = s.take<uint32_t>(N1);
  v.d = s.take<float>(N1);
  v.acc = s.take<uint32_t>(N1 + 1);
  v.co = s.take<uint32_t>(N1 + 1);
  v.new_id = s.take<uint32_t>(N1 + 1);
  v.off2 = s.take<uint32_t>(N1 + 1);
  v.enc = s.take<wfst_tr>(E2);
  v.tarcs = s.take<wfst_tr>(E2);
  v.tfin = s.take<float>(N1);
  v.toff = s.take<uint32_t>(N1 + 1);
  v.keys = s.take<unsigned long long>(tsize);
  v.minpos = s.take<uint32_t>(tsize);
  v.cls = s.take<uint32_t>(N1);
  v.slot_of = s.take<uint32_t>(N1);
  v.big = s.take<uint32_t>(N1);
  v.tab = s.take<unsigned long long>(ssize);
  v.smin = s.take<uint32_t>(ssize);
  v.smax = s.take<uint32_t>(ssize);
  v.keep = s.take<uint32_t>(N1 + 1);
  v.new_id2 = s.take<uint32_t>(N1 + 1);
  v.cnt = s.take<uint32_t>(N1 + 1);
  v.off_out = s.take<uint32_t>(N1 + 1);
  v.arcs_out = s.take<wfst_tr>(E2);
  v.fin_out = s.take<float>(N1);
  v.tsize = tsize;
  v.ssize = ssize;
  if (it) *it = v;  // (the input's side is the caller's)
  return s.at();
}

// what minimize_fst decides on the host, from the stored word and what the kernel left in the item's MbCtl (for an item
// without states: from a zeroed one); in minimize_fst's order
struct MbVerdict {
  const char* error = nullptr;
  bool empty = false;
  uint64_t props = 0;
};
MbVerdict minimize_batch_verdict(const wfst_fst* f, const MbCtl& c, bool allow_nondet) {
  using namespace props;
  MbVerdict v;
  uint64_t p = f->props & ALL;
  if (word_needs_facts(p)) p = word_with_facts(p, c.bits, c.nondet != 0);
  if ((v.error = refused_by_word(p, allow_nondet))) return v;
  const bool computed_dfs = !knows(p, CYCLIC);
  if (c.exit == MB_KO_CYCLIC || (!computed_dfs && (p & CYCLIC))) return v.error = MSG_CYCLIC, v;
  if (c.exit == MB_KO_FACTS) throw Error("minimize_batch: the kernel and the host disagree about an item's facts");
  if (!(p & WEIGHTED)) {
    if (c.exit != MB_RUNNING && c.weighted) throw Error("minimize_batch: the kernel and the host disagree about an item's branch");
    const uint64_t pc = unweighted_connect_word(p, computed_dfs, c.bits);
    if (c.exit != MB_DONE && c.exit != MB_KO_FAR_APART) {
      v.empty = true;
      v.props = pc;
      return v;
    }
    if (c.exit == MB_KO_FAR_APART) return v.error = MSG_FAR_APART, v;
    v.props = unweighted_result_word(pc, c.t_arcs != 0);
    return v;
  }
  if (c.exit != MB_RUNNING && !c.weighted) throw Error("minimize_batch: the kernel and the host disagree about an item's branch");
  if (f->start < 0) {
    uint64_t pp = p;  // push_weights_fst's word (an FST without states comes back as it is)
    if (f->n_states) pp = reweight(reweight_marks(pp, c.push_facts));  // (reweight_device without its start-state step)
    const uint64_t comp = startless_computed_word(c.pushed_bits);
    if (comp & (NOT_ACCEPTOR | WEIGHTED)) return v.error = MSG_NOT_UNWEIGHTED, v;
    v.empty = true;
    v.props = startless_result_word(pp, comp);
    return v;
  }
  if (c.exit == MB_EMPTY) {
    v.empty = true;
    v.props = empty_encoded_word(c.enc_bits);
    return v;
  }
  if (c.exit != MB_DONE) throw Error("minimize_batch: unexpected exit code " + std::to_string(c.exit));
  v.props = ACCESSIBLE | COACCESSIBLE;
  return v;
}

}  // namespace

// the host loop is batch_driver.h's, with the ownership check, one pass (nothing grows) and a slab limit per call
void minimize_batch(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, float delta, bool allow_nondet, wfst_fst** outs,
                    uint8_t* in_kernel) {
  using namespace props;
  ctx->min_batch = {};
  check_items_owned(ctx, fsts, n, "minimize_batch");
  (void)path_knob("WFST_MINIMIZE_PATH");  // (a bad WFST_MINIMIZE_PATH is KO here as in the single call)
  hipStream_t st = ctx->stream;
  enum : uint8_t { KERNEL, TRIVIAL, SINGLE };
  struct Ran {  // what the kernel left of an item: its control block and its result arrays inside the slab
    MbCtl c{};  // (an item without states: nothing ran, nothing was found)
    const uint32_t* off = nullptr;
    const wfst_tr* arcs = nullptr;
    const float* fin = nullptr;
  };
  std::vector<uint8_t> kind(n);
  std::vector<Ran> ran(n);
  std::vector<size_t> run;  // the items that occupy a workgroup
  for (size_t i = 0; i < n; ++i) {
    const wfst_fst* f = fsts[i];
    // the rule is on (n_states, n_arcs) alone.  A word that says INITIAL_CYCLIC belongs to a cyclic input (KO) or
    // contradicts itself, and reweight's start-state step would add a state for it: the single call's business.
    const bool fits = f->n_states <= MB_MAX_STATES && f->n_arcs <= MB_MAX_ARCS;
    kind[i] = f->n_states == 0 ? TRIVIAL : (fits && !(f->props & INITIAL_CYCLIC)) ? KERNEL : SINGLE;
    if (kind[i] == KERNEL) {
      ensure_device(const_cast<wfst_fst*>(f));
      run.push_back(i);
    }
  }
  auto carve = [&](size_t i, Slab s, MbItem* it) {
    const wfst_fst* f = fsts[i];
    const size_t end = carve_minimize_slice(s, f->n_states, (uint32_t)f->n_arcs, it);
    if (!it) return end;
    const uint64_t p = f->props & ALL;
    it->off = f->dev.offsets;
    it->arcs = f->dev.arcs;
    it->fin = f->dev.finals;
    it->n = f->n_states;
    it->E = (uint32_t)f->n_arcs;
    it->start = f->start < 0 ? NONE : (uint32_t)f->start;
    it->known = 0;
    if (knows(p, ACCEPTOR) && knows(p, I_DETERMINISTIC) && knows(p, WEIGHTED))
      it->known |= MBK_FACTS | ((p & ACCEPTOR) ? MBK_ACCEPTOR : 0u) | ((p & I_DETERMINISTIC) ? MBK_IDET : 0u) |
                   ((p & WEIGHTED) ? MBK_WEIGHTED : 0u);
    if (knows(p, CYCLIC)) it->known |= MBK_CYCLIC_KNOWN | ((p & CYCLIC) ? MBK_CYCLIC : 0u);
    it->delta = delta;
    return end;
  };
  auto launch = [&](const MbItem* d_items, uint32_t m) { minimize_batch_kernel<<<m, MB_TPB, 0, st>>>(d_items); };
  auto classify = [&](size_t i, const MbCtl& c, const MbItem& it) {
    ran[i] = Ran{c, it.off_out, it.arcs_out, it.fin_out};
    return BatchExit::FINISHED;
  };
  const auto slabs = batch_launch_loop<MbItem, MbCtl>(ctx, ctx->min_batch, {"minimize_batch", 1, nullptr, MB_MAX_SLAB, "call"},
                                                      std::move(run), carve, nullptr, launch, classify);
  auto outcome = [&](size_t i) {
    if (kind[i] == SINGLE) return BatchOutcome::single();
    const MbCtl& c = ran[i].c;
    if (kind[i] == KERNEL && c.exit == MB_RUNNING) throw Error("minimize_batch: the kernel left item " + std::to_string(i) + " unfinished");
    const MbVerdict v = minimize_batch_verdict(fsts[i], c, allow_nondet);
    if (v.error) throw Error("item " + std::to_string(i) + ": " + v.error);
    if (v.empty) return BatchOutcome::handle(empty_fst(ctx, v.props));
    return BatchOutcome::adopt({c.n_out, c.e_out, (int64_t)c.start_out, v.props & ALL, ran[i].off, ran[i].arcs, ran[i].fin});
  };
  batch_finish(ctx, ctx->min_batch, n, outs, in_kernel, outcome, [&](size_t i) { return minimize_fst(ctx, fsts[i], delta, allow_nondet); });
}

}  // namespace wfst
