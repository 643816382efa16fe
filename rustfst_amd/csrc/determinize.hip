// determinize.hip — determinize / determinize_with_config of an acceptor on the device
// (rustfst/src/algorithms/determinize/{determinize_static.rs:149-190, determinize_fsa_op.rs:43-196, state_table.rs:79-96},
//  lazy/lazy_fst.rs:226-269): DeterminizeFsa with DefaultCommonDivisor, materialised in the reference's FIFO first-touch
// order.  Host restatement: nshortest.hip determinize_with_distance; oracle: oracle.cpp determinize_with_distance_impl.
//
// Level-synchronous subset construction.  The states of one BFS level are the ids [lo, hi); per level
//   count    raw candidates per level state (sum of its elements' out-degrees), exclusive scan -> slot ranges, K in all
//   check    capacities for K more candidates / states / elements / arcs; a shortfall stops BEFORE anything is written
//   expand   ONE LANE PER STATE: gathers (label, dest, w (x) arc w) in element then arc order, sorts them stably by
//            (label, dest) (insertion sort up to 16, else a bottom-up merge sort in its slice of a global scratch), then per
//            label: arc weight = plus over the label, duplicate destinations plus-merged, every element quantize(w - arc
//            weight, delta).  Candidate g of the state sits in slot coff[i] + g: slot order IS the emission order
//            (state position in the level, then arc position).  The state's final weight is computed here too.
//   lookup   every candidate in parallel against the states of EARLIER levels: the global table maps the hash of the
//            state-id sequence to a chain of states; the lowest-id chain member with the same states and pairwise
//            approx_eq weights (|a - b| <= KDELTA) wins.  These states do not change during the level, so this is exact.
//   rounds   the rest are resolved among themselves, per hash: the lowest unresolved slot of a hash (atomicMin) is a NEW
//            state (every earlier slot of that hash found an older state or joined an earlier leader); unresolved
//            candidates that approx-match it join it, the others wait for the next round's leader.  This is exactly the
//            sequential rule "join the lowest-id match, else create", approx_eq's missing transitivity included.
//   number   new states get hi + rank of their slot among the creators (first emission order = the reference's ids);
//            their subsets are appended, their ids pushed on the chains; every candidate becomes an output arc at
//            its rank among the valid slots, so the arcs come out in CSR order, per state in label order.
// Two regimes: NARROW = one workgroup runs every phase of level after level inside one launch (lattices: thousands of
// levels of a few states); WIDE = one device-wide launch per phase.  The host switches by the size of the next level
// (or WFST_DETERMINIZE_PATH=narrow|wide pins one).  Arrays grow by doubling between levels (hash table rehashed).
// TropicalWeight arithmetic exactly as the oracle's: plus = (b < a ? b : a), times with inf checks, divide = a - b,
// quantize = floor(v / delta + 0.5) * delta (semiring.rs:132-145); no contraction (pragma below).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#pragma clang fp contract(off)  // (before tropical.h comes in: its functions compile without contraction here too)

#include "batch_driver.h"
#include "common.h"
#include "fst_props.h"


namespace wfst {

namespace {

constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint64_t EMPTY_KEY = ~0ull;
constexpr uint32_t TPB = 256;  // threads of every block (the narrow regime is one such block)
// candidate status
constexpr uint32_t C_UNRES = 0, C_EXIST = 1, C_CREATE = 2, C_JOIN = 3, C_INVALID = 4;
// narrow regime: levels of at most NARROW_STATES states and NARROW_CANDS candidates stay in the one-workgroup kernel
constexpr uint32_t NARROW_STATES = 256, NARROW_CANDS = 8192;
constexpr uint32_t NARROW_LEVELS_PER_LAUNCH = 1u << 16;
// WFST_DETERMINIZE_BATCH_SCRATCH unset: where the batch kernel keeps the scratch of small levels (profiles/determinize_batch_timing.md)
#ifndef WFST_DETERMINIZE_BATCH_LDS_DEFAULT
#define WFST_DETERMINIZE_BATCH_LDS_DEFAULT false
#endif

struct Ctl {
  uint32_t lo, hi;   // the level to expand: states [lo, hi)
  uint32_t n_elts;   // subset elements stored (states [0, hi))
  uint32_t n_arcs;   // output arcs stored (states [0, lo))
  uint32_t K;        // raw candidates of the level (after the count scan)
  uint32_t T;        // size of the level's hash table (power of two)
  uint32_t need;     // 1: the level needs more room (nothing of it was written)
  uint32_t err;      // 1: state or element limit exceeded
  uint32_t rem;      // candidates left unresolved by the last round
  uint32_t levels;   // levels completed
  uint32_t exit;     // narrow kernel: 1 level too wide, 2 budget, 3 need, 4 done, 5 err
  uint32_t start;    // batch kernel: the input's start state (the block seeds state 0 itself)
};

struct Caps {
  uint32_t states;  // ids (so / aoff hold states + 1 entries)
  uint32_t elts;
  uint32_t arcs;
  uint32_t cands;   // slots of one level
  uint32_t slots;   // global hash table (power of two)
  uint32_t ltab;    // level hash table (power of two >= 2 * cands)
  uint32_t max_states;
  uint32_t max_elts;
};

struct Det {
  // input
  const uint32_t* off;
  const wfst_tr* arcs;
  const float* fin;
  float delta;
  // result
  uint32_t* so;     // [states + 1] subset start
  uint2* se;        // [elts] {state, weight bits}
  uint32_t* aoff;   // [states + 1] arc start
  float* ofin;      // [states]
  wfst_tr* oarc;    // [arcs]
  uint64_t* hkey;   // [slots] global table: hash of the state-id sequence
  uint32_t* hhead;  // [slots] chain head
  uint32_t* hnext;  // [states]
  // level scratch
  uint64_t* lsc;    // [states + 1] per level state: raw count, then its exclusive scan
  uint4* ca;        // [cands] raw candidates {label, dest, weight bits, -}, sorted in place
  uint4* cb;        // [cands] merge-sort scratch
  uint2* ce;        // [cands] merged candidate elements
  uint4* crec;      // [cands] {label, arc weight bits, element begin, element count}
  uint64_t* chash;  // [cands]
  uint32_t* cst;    // [cands] C_*
  uint32_t* cdest;  // [cands] existing id (C_EXIST) / leader slot (C_JOIN)
  uint32_t* cslot;  // [cands] level-table slot
  uint64_t* sc1;    // [cands + 1] (elements << 32 | 1) of creators, then scanned
  uint64_t* sc2;    // [cands + 1] 1 for valid slots, then scanned
  uint64_t* lkey;   // [ltab]
  uint32_t* lead;   // [2 * ltab] round leaders, two parities
  Ctl* ctl;
  Caps cap;
};

__device__ inline uint64_t hash_states(const uint2* e, uint32_t n) {  // FNV-1a over the state ids
  uint64_t h = 1469598103934665603ull;
  for (uint32_t k = 0; k < n; ++k) h = (h ^ e[k].x) * 1099511628211ull;
  return h == EMPTY_KEY ? h - 1 : h;
}
__device__ inline bool same_subset(const uint2* a, uint32_t na, const uint2* b, uint32_t nb) {
  if (na != nb) return false;
  for (uint32_t k = 0; k < na; ++k)
    if (a[k].x != b[k].x || !weq(__uint_as_float(a[k].y), __uint_as_float(b[k].y))) return false;
  return true;
}
// open addressing, linear probing; `insert`: claim an empty slot with a CAS (NONE when the table is full)
__device__ inline uint32_t probe(uint64_t* keys, uint32_t size, uint64_t h, bool insert) {
  const uint32_t mask = size - 1;
  uint32_t p = (uint32_t)(h ^ (h >> 32)) & mask;
  for (uint32_t i = 0; i < size; ++i, p = (p + 1) & mask) {
    uint64_t k = keys[p];
    if (k == h) return p;
    if (k == EMPTY_KEY) {
      if (!insert) return NONE;
      k = atomicCAS((unsigned long long*)&keys[p], (unsigned long long)EMPTY_KEY, (unsigned long long)h);
      if (k == EMPTY_KEY || k == h) return p;
    }
  }
  return NONE;
}

// ---------------------------------------------------------------- phases (lanes tid, tid + nt, ... of the level)
__device__ void ph_count(const Det& d, uint32_t lo, uint32_t L, uint32_t tid, uint32_t nt) {
  for (uint32_t i = tid; i < L; i += nt) {
    const uint32_t s = lo + i;
    uint64_t c = 0;
    for (uint32_t k = d.so[s]; k < d.so[s + 1]; ++k) {
      const uint32_t q = d.se[k].x;
      c += d.off[q + 1] - d.off[q];
    }
    d.lsc[i] = c;
  }
}

// the level fits (K candidates): capacities and the level table size; one lane
__device__ void ph_check(const Det& d, Ctl& c) {
  const uint64_t K = c.K;
  uint32_t T = 64;
  while ((uint64_t)T < 2 * K) T <<= 1;
  c.T = T;
  c.need = (K > d.cap.cands || (uint64_t)c.hi + K > d.cap.states || (uint64_t)c.n_elts + K > d.cap.elts ||
            (uint64_t)c.n_arcs + K > d.cap.arcs || 2 * ((uint64_t)c.hi + K) > d.cap.slots || T > d.cap.ltab)
               ? 1u
               : 0u;
}

__device__ void ph_clear(const Det& d, uint32_t T, uint32_t tid, uint32_t nt) {
  for (uint32_t i = tid; i < T; i += nt) {
    d.lkey[i] = EMPTY_KEY;
    d.lead[i] = NONE;
    d.lead[d.cap.ltab + i] = NONE;
  }
}

__device__ inline bool key_less(const uint4& a, const uint4& b) { return a.x != b.x ? a.x < b.x : a.y < b.y; }

__device__ void ph_expand(const Det& d, uint32_t lo, uint32_t L, uint32_t tid, uint32_t nt) {
  const float delta = d.delta;
  for (uint32_t i = tid; i < L; i += nt) {
    const uint32_t s = lo + i;
    const uint32_t b = (uint32_t)d.lsc[i], e = (uint32_t)d.lsc[i + 1], m = e - b;
    uint4* A = d.ca + b;
    float fw = INF;  // compute_final_weight (determinize_fsa_op.rs:101-118)
    uint32_t p = 0;
    for (uint32_t k = d.so[s]; k < d.so[s + 1]; ++k) {
      const uint2 el = d.se[k];
      const float w = __uint_as_float(el.y);
      fw = wplus(fw, wtimes(w, d.fin[el.x]));
      for (uint32_t a = d.off[el.x]; a < d.off[el.x + 1]; ++a) {
        const wfst_tr t = d.arcs[a];
        A[p++] = make_uint4(t.ilabel, t.nextstate, __float_as_uint(wtimes(w, t.weight)), 0u);
      }
    }
    d.ofin[s] = fw;
    // stable sort on (label, dest): the BTreeMap's ascending labels, norm_tr's stable sort by state
    const uint4* S = A;
    if (m <= 16) {
      for (uint32_t x = 1; x < m; ++x) {
        const uint4 v = A[x];
        uint32_t y = x;
        while (y > 0 && key_less(v, A[y - 1])) {
          A[y] = A[y - 1];
          --y;
        }
        A[y] = v;
      }
    } else {
      uint4* src = A;
      uint4* dst = d.cb + b;
      for (uint32_t w = 1; w < m; w <<= 1) {
        for (uint32_t l = 0; l < m; l += 2 * w) {
          const uint32_t mid = min(l + w, m), r = min(l + 2 * w, m);
          uint32_t x = l, y = mid, o = l;
          while (x < mid && y < r) dst[o++] = key_less(src[y], src[x]) ? src[y++] : src[x++];
          while (x < mid) dst[o++] = src[x++];
          while (y < r) dst[o++] = src[y++];
        }
        uint4* t = src;
        src = dst;
        dst = t;
      }
      S = src;
    }
    // norm_tr per label (determinize_fsa_op.rs:149-179)
    uint2* E = d.ce;
    uint32_t g = 0, ep = b;
    for (uint32_t x = 0; x < m;) {
      const uint32_t label = S[x].x;
      uint32_t y = x;
      float weight = INF;
      while (y < m && S[y].x == label) weight = wplus(weight, __uint_as_float(S[y++].z));
      const uint32_t eb = ep;
      for (uint32_t k = x; k < y; ++k) {
        const float w = __uint_as_float(S[k].z);
        if (ep > eb && E[ep - 1].x == S[k].y)
          E[ep - 1].y = __float_as_uint(wplus(__uint_as_float(E[ep - 1].y), w));
        else
          E[ep++] = make_uint2(S[k].y, __float_as_uint(w));
      }
      for (uint32_t k = eb; k < ep; ++k) E[k].y = __float_as_uint(quantize(__uint_as_float(E[k].y) - weight, delta));
      const uint32_t c = b + g++;
      d.crec[c] = make_uint4(label, __float_as_uint(weight), eb, ep - eb);
      d.chash[c] = hash_states(E + eb, ep - eb);
      d.cst[c] = C_UNRES;
      x = y;
    }
    for (uint32_t c = b + g; c < e; ++c) d.cst[c] = C_INVALID;
  }
}

// candidates against the states of earlier levels (lowest id wins); the others get their level-table slot
__device__ void ph_lookup(const Det& d, uint32_t K, uint32_t T, uint32_t hi, uint32_t tid, uint32_t nt) {
  for (uint32_t c = tid; c < K; c += nt) {
    if (d.cst[c] != C_UNRES) continue;
    const uint64_t h = d.chash[c];
    const uint4 r = d.crec[c];
    const uint32_t gs = probe(d.hkey, d.cap.slots, h, false);
    uint32_t best = NONE;
    if (gs != NONE) {
      uint32_t id = d.hhead[gs];
      for (uint32_t steps = 0; id != NONE && steps < hi; ++steps, id = d.hnext[id])
        if (id < best && same_subset(d.ce + r.z, r.w, d.se + d.so[id], d.so[id + 1] - d.so[id])) best = id;
    }
    if (best != NONE) {
      d.cst[c] = C_EXIST;
      d.cdest[c] = best;
    } else {
      d.cslot[c] = probe(d.lkey, T, h, true);  // (T >= 2 K: never full)
    }
  }
}

__device__ void ph_round_a(const Det& d, uint32_t K, uint32_t r, uint32_t tid, uint32_t nt) {
  const uint32_t cur = (r & 1) * d.cap.ltab, nxt = ((r + 1) & 1) * d.cap.ltab;
  for (uint32_t c = tid; c < K; c += nt) {
    if (d.cst[c] != C_UNRES) continue;
    atomicMin(&d.lead[cur + d.cslot[c]], c);
    d.lead[nxt + d.cslot[c]] = NONE;  // (round r - 1 has read it)
  }
}
// returns the number of candidates this lane left unresolved
__device__ uint32_t ph_round_b(const Det& d, uint32_t K, uint32_t r, uint32_t tid, uint32_t nt) {
  const uint32_t cur = (r & 1) * d.cap.ltab;
  uint32_t left = 0;
  for (uint32_t c = tid; c < K; c += nt) {
    if (d.cst[c] != C_UNRES) continue;
    const uint32_t l = d.lead[cur + d.cslot[c]];
    if (l == c) {
      d.cst[c] = C_CREATE;
      continue;
    }
    const uint4 a = d.crec[c], b = d.crec[l];
    if (d.chash[l] == d.chash[c] && same_subset(d.ce + a.z, a.w, d.ce + b.z, b.w)) {
      d.cst[c] = C_JOIN;
      d.cdest[c] = l;
    } else {
      ++left;
    }
  }
  return left;
}

__device__ void ph_flags(const Det& d, uint32_t K, uint32_t tid, uint32_t nt) {
  for (uint32_t c = tid; c < K; c += nt) {
    const uint32_t st = d.cst[c];
    d.sc1[c] = st == C_CREATE ? (((uint64_t)d.crec[c].w << 32) | 1ull) : 0ull;
    d.sc2[c] = st == C_INVALID ? 0ull : 1ull;
  }
}

__device__ void ph_number(const Det& d, const Ctl& c0, uint32_t tid, uint32_t nt) {
  const uint32_t lo = c0.lo, hi = c0.hi, K = c0.K, L = c0.hi - c0.lo;
  for (uint32_t c = tid; c < K; c += nt) {
    const uint32_t st = d.cst[c];
    if (st == C_INVALID) continue;
    uint32_t dest;
    if (st == C_CREATE) {
      dest = hi + (uint32_t)d.sc1[c];
      const uint32_t eb = c0.n_elts + (uint32_t)(d.sc1[c] >> 32);
      const uint4 r = d.crec[c];
      d.so[dest] = eb;
      for (uint32_t k = 0; k < r.w; ++k) d.se[eb + k] = d.ce[r.z + k];
      const uint32_t gs = probe(d.hkey, d.cap.slots, d.chash[c], true);  // (slots >= 2 (hi + K): never full)
      d.hnext[dest] = atomicExch(&d.hhead[gs], dest);
    } else if (st == C_JOIN) {
      dest = hi + (uint32_t)d.sc1[d.cdest[c]];
    } else {
      dest = d.cdest[c];
    }
    const uint4 r = d.crec[c];
    wfst_tr t;
    t.ilabel = r.x;
    t.olabel = r.x;
    t.weight = __uint_as_float(r.y);
    t.nextstate = dest;
    d.oarc[c0.n_arcs + (uint32_t)d.sc2[c]] = t;
  }
  for (uint32_t i = tid; i < L; i += nt) d.aoff[lo + i] = c0.n_arcs + (uint32_t)d.sc2[(uint32_t)d.lsc[i]];
}

// the next level; one lane
__device__ void ph_advance(const Det& d, Ctl& c) {
  const uint32_t ncre = (uint32_t)d.sc1[c.K], nel = (uint32_t)(d.sc1[c.K] >> 32), nv = (uint32_t)d.sc2[c.K];
  d.so[c.hi + ncre] = c.n_elts + nel;
  c.n_arcs += nv;
  c.n_elts += nel;
  c.lo = c.hi;
  c.hi += ncre;
  c.levels += 1;
  // (a cyclic weighted acceptor without the twins property has no finite determinization; the reference runs out of memory)
  if (c.hi > d.cap.max_states || c.n_elts > d.cap.max_elts) c.err = 1;
}

// ---------------------------------------------------------------- block-wide exclusive scan of v[b, e) (in place)
// v[e] receives the total (+ carry); every thread of the block calls it
__device__ uint64_t block_scan(uint64_t* v, uint32_t b, uint32_t e, uint64_t carry, uint64_t* lds) {
  const uint32_t t = threadIdx.x;
  for (uint32_t base = b; base < e; base += TPB) {
    const uint32_t i = base + t;
    const uint64_t x = i < e ? v[i] : 0ull;
    lds[t] = x;
    __syncthreads();
    for (uint32_t o = 1; o < TPB; o <<= 1) {
      const uint64_t y = t >= o ? lds[t - o] : 0ull;
      __syncthreads();
      lds[t] += y;
      __syncthreads();
    }
    if (i < e) v[i] = carry + lds[t] - x;
    carry += lds[TPB - 1];
    __syncthreads();
  }
  return carry;
}

// ---------------------------------------------------------------- narrow regime: one workgroup, many levels
// between phases: a device-scope fence (the atomics of one phase are read by plain loads of the next) and the barrier
__device__ inline void bar() {
  __threadfence();
  __syncthreads();
}
// one level of the narrow regime, every thread of the block: 0 = the level is complete, else the exit code (Ctl::exit).
// `d` holds the result arrays and the capacities the level is checked against; the phases after the check run on `dl`
// instead when it is given and the level has at most dl->cap.cands raw candidates (the batch kernel's level scratch in LDS).
__device__ __forceinline__ uint32_t narrow_level(const Det& d, const Det* dl, Ctl& c, uint32_t& left, uint64_t* lds,
                                                 uint32_t max_k) {
  const uint32_t t = threadIdx.x;
  const uint32_t L = c.hi - c.lo;
  ph_count(d, c.lo, L, t, TPB);
  bar();
  const uint64_t K = block_scan(d.lsc, 0, L, 0, lds);
  if (t == 0) {
    d.lsc[L] = K;
    c.K = (uint32_t)std::min<uint64_t>(K, 0xFFFFFFFFull);
    ph_check(d, c);
    if (K > 0xFFFFFFFFull) c.need = 1;
  }
  bar();
  if (c.need || c.K > max_k) return c.need ? 3 : 1;
  const Det& v = (dl && c.K <= dl->cap.cands) ? *dl : d;
  ph_clear(v, c.T, t, TPB);
  ph_expand(v, c.lo, L, t, TPB);
  bar();
  ph_lookup(v, c.K, c.T, c.hi, t, TPB);
  bar();
  for (uint32_t r = 0; r <= c.K; ++r) {  // (every round settles its leaders: at most K rounds)
    ph_round_a(v, c.K, r, t, TPB);
    if (t == 0) left = 0;
    bar();
    const uint32_t l = ph_round_b(v, c.K, r, t, TPB);
    if (l) atomicAdd(&left, l);
    bar();
    const bool done = left == 0;
    __syncthreads();
    if (done) break;
  }
  ph_flags(v, c.K, t, TPB);
  bar();
  const uint64_t t1 = block_scan(v.sc1, 0, c.K, 0, lds);
  const uint64_t t2 = block_scan(v.sc2, 0, c.K, 0, lds);
  if (t == 0) {
    v.sc1[c.K] = t1;
    v.sc2[c.K] = t2;
  }
  bar();
  ph_number(v, c, t, TPB);
  bar();
  if (t == 0) ph_advance(v, c);
  bar();
  return 0;
}
__global__ void __launch_bounds__(TPB) det_narrow_kernel(Det d, uint32_t max_l, uint32_t max_k, uint32_t budget) {
  __shared__ uint64_t lds[TPB];
  __shared__ Ctl c;
  __shared__ uint32_t left;
  const uint32_t t = threadIdx.x;
  if (t == 0) c = *d.ctl;
  __syncthreads();
  for (uint32_t it = 0;; ++it) {
    const uint32_t L = c.hi - c.lo;
    if (c.err || L == 0 || L > max_l || it >= budget) {
      if (t == 0) c.exit = c.err ? 5 : (L == 0 ? 4 : (L > max_l ? 1 : 2));
      break;
    }
    const uint32_t x = narrow_level(d, nullptr, c, left, lds, max_k);
    if (x) {
      if (t == 0) c.exit = x;
      break;
    }
  }
  __syncthreads();
  if (t == 0) *d.ctl = c;
}

// ---------------------------------------------------------------- batch: one workgroup per item, one launch for all
// Block b runs the narrow level loop on items[b] from the seed to the end.  Exits as above, without the level budget:
// 1 = a level of more than NARROW_STATES states or NARROW_CANDS raw candidates (the host finishes the item with the
// single-FST path), 3 = the item's slice is too small (the host grows it and runs the item again), 4 done, 5 err.
// lds_bytes > 0: the level scratch of levels with at most BATCH_LDS_CANDS candidates lives in LDS.
constexpr uint32_t BATCH_LDS_CANDS = 496, BATCH_LDS_LTAB = 1024;
constexpr size_t BATCH_LDS_BYTES = (size_t)BATCH_LDS_CANDS * (3 * 16 + 8 + 8 + 3 * 4) + 2 * 8 * (BATCH_LDS_CANDS + 1) +
                                   (size_t)BATCH_LDS_LTAB * (8 + 2 * 4);
__global__ void __launch_bounds__(TPB) det_batch_kernel(const Det* __restrict__ items, uint32_t lds_bytes) {
  extern __shared__ __align__(16) unsigned char arena[];
  __shared__ uint64_t lds[TPB];
  __shared__ Ctl c;
  __shared__ uint32_t left;
  const uint32_t t = threadIdx.x;
  const Det d = items[blockIdx.x];
  Det dl = d;
  if (lds_bytes) {  // 16-byte arrays first, then the 8-byte, then the 4-byte ones
    unsigned char* p = arena;
    auto take = [&](size_t bytes) {
      unsigned char* q = p;
      p += bytes;
      return q;
    };
    dl.ca = (uint4*)take(16 * BATCH_LDS_CANDS);
    dl.cb = (uint4*)take(16 * BATCH_LDS_CANDS);
    dl.crec = (uint4*)take(16 * BATCH_LDS_CANDS);
    dl.ce = (uint2*)take(8 * BATCH_LDS_CANDS);
    dl.chash = (uint64_t*)take(8 * BATCH_LDS_CANDS);
    dl.sc1 = (uint64_t*)take(8 * (BATCH_LDS_CANDS + 1));
    dl.sc2 = (uint64_t*)take(8 * (BATCH_LDS_CANDS + 1));
    dl.lkey = (uint64_t*)take(8 * BATCH_LDS_LTAB);
    dl.cst = (uint32_t*)take(4 * BATCH_LDS_CANDS);
    dl.cdest = (uint32_t*)take(4 * BATCH_LDS_CANDS);
    dl.cslot = (uint32_t*)take(4 * BATCH_LDS_CANDS);
    dl.lead = (uint32_t*)take(4 * 2 * BATCH_LDS_LTAB);
    dl.cap.cands = BATCH_LDS_CANDS;
    dl.cap.ltab = BATCH_LDS_LTAB;  // (>= 2 * BATCH_LDS_CANDS: ph_check's T fits)
  }
  if (t == 0) c = *d.ctl;
  for (uint32_t i = t; i < d.cap.slots; i += TPB) {
    d.hkey[i] = EMPTY_KEY;
    d.hhead[i] = NONE;
  }
  bar();
  if (t == 0) {  // state 0 = {(start, 0.0)} (det_seed_kernel)
    d.so[0] = 0;
    d.so[1] = 1;
    d.se[0] = make_uint2(c.start, __float_as_uint(0.0f));
    const uint32_t gs = probe(d.hkey, d.cap.slots, hash_states(d.se, 1), true);
    d.hhead[gs] = 0;
    d.hnext[0] = NONE;
  }
  bar();
  for (;;) {
    const uint32_t L = c.hi - c.lo;
    if (c.err || L == 0 || L > NARROW_STATES) {
      if (t == 0) c.exit = c.err ? 5 : (L == 0 ? 4 : 1);
      break;
    }
    const uint32_t x = narrow_level(d, lds_bytes ? &dl : nullptr, c, left, lds, NARROW_CANDS);
    if (x) {
      if (t == 0) c.exit = x;
      break;
    }
  }
  __syncthreads();
  if (t == 0) {
    if (c.exit == 4) d.aoff[c.hi] = c.n_arcs;  // CSR: aoff[N] = number of arcs
    *d.ctl = c;
  }
}

// out_dist[s] = plus over the elements (q, w) of subset s, in stored order, of w (x) in_dist[q]; q >= n_in counts as +inf
// (determinize_static.rs:24-39, state_table.rs:25-39,79-96).  One lane per result state, all jobs of a batch in one launch:
// job j owns out[off[j], off[j + 1]).
struct DistJob {
  const uint32_t* so;
  const uint2* se;
  const float* in;
  uint32_t n_in;
};
__global__ void __launch_bounds__(TPB) det_dist_kernel(const DistJob* __restrict__ jobs, const uint32_t* __restrict__ off,
                                                       uint32_t n_jobs, float* __restrict__ out) {
  const uint32_t total = off[n_jobs];
  for (uint32_t g = blockIdx.x * TPB + threadIdx.x; g < total; g += gridDim.x * TPB) {
    uint32_t lo = 0, hi = n_jobs;  // the job with off[j] <= g < off[j + 1] (empty jobs are skipped by the search)
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) / 2;
      if (off[mid] <= g) lo = mid; else hi = mid;
    }
    const DistJob j = jobs[lo];
    const uint32_t s = g - off[lo];
    float acc = INF;
    for (uint32_t k = j.so[s]; k < j.so[s + 1]; ++k) {
      const uint2 e = j.se[k];
      acc = wplus(acc, wtimes(__uint_as_float(e.y), e.x < j.n_in ? j.in[e.x] : INF));
    }
    out[g] = acc;
  }
}

// ---------------------------------------------------------------- wide regime: one launch per phase
__global__ void __launch_bounds__(TPB) det_count_kernel(Det d) {
  const Ctl c = *d.ctl;
  if (c.err || c.need) return;
  ph_count(d, c.lo, c.hi - c.lo, blockIdx.x * TPB + threadIdx.x, gridDim.x * TPB);
}
// grid-wide exclusive scan of v[0, n) in place, n read from the device (*n_lo32 or the level size): three launches
//   part: block k sums its chunk into part[k]; top: one block scans part[]; apply: block k scans its chunk with carry part[k]
__device__ inline uint32_t scan_len(const Ctl& c, int which) { return which == 0 ? c.hi - c.lo : c.K; }
__global__ void __launch_bounds__(TPB) det_scan_part_kernel(Det d, uint64_t* v, uint64_t* part, int which) {
  __shared__ uint64_t lds[TPB];
  const Ctl c = *d.ctl;
  if (c.err || (c.need && which)) return;
  const uint32_t n = scan_len(c, which), G = gridDim.x, ch = (n + G - 1) / G;
  const uint32_t b = min(n, blockIdx.x * ch), e = min(n, b + ch);
  uint64_t s = 0;
  for (uint32_t i = b + threadIdx.x; i < e; i += TPB) s += v[i];
  lds[threadIdx.x] = s;
  __syncthreads();
  for (uint32_t o = TPB / 2; o; o >>= 1) {
    if (threadIdx.x < o) lds[threadIdx.x] += lds[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = lds[0];
}
__global__ void __launch_bounds__(TPB) det_scan_top_kernel(Det d, uint64_t* part, uint32_t G, int which) {
  __shared__ uint64_t lds[TPB];
  const Ctl c = *d.ctl;
  if (c.err || (c.need && which)) return;
  block_scan(part, 0, G, 0, lds);
}
// which == 0 (the count scan): also the capacity check
__global__ void __launch_bounds__(TPB) det_scan_apply_kernel(Det d, uint64_t* v, const uint64_t* part, uint32_t G, int which) {
  __shared__ uint64_t lds[TPB];
  const Ctl c = *d.ctl;
  if (c.err || (c.need && which)) return;
  const uint32_t n = scan_len(c, which), ch = (n + G - 1) / G;
  const uint32_t b = min(n, blockIdx.x * ch), e = min(n, b + ch);
  const uint64_t tot = block_scan(v, b, e, part[blockIdx.x], lds);
  if (blockIdx.x == G - 1 && threadIdx.x == 0) v[n] = tot;
}
__global__ void det_check_kernel(Det d) {
  Ctl c = *d.ctl;
  if (c.err) return;
  const uint64_t K = d.lsc[c.hi - c.lo];
  c.K = (uint32_t)std::min<uint64_t>(K, 0xFFFFFFFFull);
  ph_check(d, c);
  if (K > 0xFFFFFFFFull) c.need = 1;
  *d.ctl = c;
}
__global__ void __launch_bounds__(TPB) det_clear_kernel(Det d) {
  const Ctl c = *d.ctl;
  if (c.err || c.need) return;
  ph_clear(d, c.T, blockIdx.x * TPB + threadIdx.x, gridDim.x * TPB);
}
__global__ void __launch_bounds__(TPB) det_expand_kernel(Det d) {
  const Ctl c = *d.ctl;
  if (c.err || c.need) return;
  ph_expand(d, c.lo, c.hi - c.lo, blockIdx.x * TPB + threadIdx.x, gridDim.x * TPB);
}
__global__ void __launch_bounds__(TPB) det_lookup_kernel(Det d) {
  const Ctl c = *d.ctl;
  if (c.err || c.need) return;
  ph_lookup(d, c.K, c.T, c.hi, blockIdx.x * TPB + threadIdx.x, gridDim.x * TPB);
}
__global__ void __launch_bounds__(TPB) det_round_a_kernel(Det d, uint32_t r) {
  const Ctl c = *d.ctl;
  if (c.err || c.need) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) d.ctl->rem = 0;
  ph_round_a(d, c.K, r, blockIdx.x * TPB + threadIdx.x, gridDim.x * TPB);
}
__global__ void __launch_bounds__(TPB) det_round_b_kernel(Det d, uint32_t r) {
  const Ctl c = *d.ctl;
  if (c.err || c.need) return;
  uint32_t left = ph_round_b(d, c.K, r, blockIdx.x * TPB + threadIdx.x, gridDim.x * TPB);
  for (int o = 32; o >= 1; o >>= 1) left += __shfl_xor(left, o);
  if ((threadIdx.x & 63) == 0 && left) atomicAdd(&d.ctl->rem, left);
}
__global__ void __launch_bounds__(TPB) det_flags_kernel(Det d) {
  const Ctl c = *d.ctl;
  if (c.err || c.need) return;
  ph_flags(d, c.K, blockIdx.x * TPB + threadIdx.x, gridDim.x * TPB);
}
__global__ void __launch_bounds__(TPB) det_number_kernel(Det d) {
  const Ctl c = *d.ctl;
  if (c.err || c.need) return;
  ph_number(d, c, blockIdx.x * TPB + threadIdx.x, gridDim.x * TPB);
}
__global__ void det_advance_kernel(Det d) {
  Ctl c = *d.ctl;
  if (c.err || c.need) return;
  ph_advance(d, c);
  *d.ctl = c;
}

// ---------------------------------------------------------------- set-up, growth, end
__global__ void det_seed_kernel(Det d, uint32_t start) {  // state 0 = {(start, 0.0)}, not quantized (determinize_fsa_op.rs:45-55)
  d.so[0] = 0;
  d.so[1] = 1;
  d.se[0] = make_uint2(start, __float_as_uint(0.0f));
  const uint32_t gs = probe(d.hkey, d.cap.slots, hash_states(d.se, 1), true);
  d.hhead[gs] = 0;
  d.hnext[0] = NONE;
}
__global__ void __launch_bounds__(TPB) det_rehash_kernel(const uint64_t* okey, const uint32_t* ohead, uint32_t oslots,
                                                         uint64_t* nkey, uint32_t* nhead, uint32_t nslots) {
  for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < oslots; i += gridDim.x * TPB) {
    if (okey[i] == EMPTY_KEY) continue;
    const uint32_t p = probe(nkey, nslots, okey[i], true);
    nhead[p] = ohead[i];  // (the chains in hnext stay as they are)
  }
}

template <class T>
void grow(DevicePool& pool, DBuf<T>& b, size_t n, size_t keep, hipStream_t st) {
  if (b.p && b.n >= n) return;
  DBuf<T> nb(pool, n);
  if (b.p && keep) HIP_CHECK(hipMemcpyAsync(nb.p, b.p, keep * sizeof(T), hipMemcpyDeviceToDevice, st));
  b = std::move(nb);
}

struct Run {
  DevicePool& pool;
  hipStream_t st;
  Caps cap{};
  DBuf<uint32_t> so, aoff, hhead, hnext, cst, cdest, cslot, lead;
  DBuf<uint2> se, ce;
  DBuf<float> ofin;
  DBuf<wfst_tr> oarc;
  DBuf<uint64_t> hkey, lsc, chash, sc1, sc2, lkey, part;
  DBuf<uint4> ca, cb, crec;
  DBuf<Ctl> ctl;
  wfst_ctx::DeterminizeStats* tally = nullptr;  // grow_* / rehashes: reserve calls after the first that enlarged an array
  explicit Run(DevicePool& p, hipStream_t s) : pool(p), st(s) {}

  // room for at least `states` ids, `elts` elements, `arcs` arcs and a level of `cands` slots; the first `kept_*` entries
  // of the result arrays are copied
  void reserve(uint64_t states, uint64_t elts, uint64_t arcs, uint64_t cands, const Ctl& c) {
    auto up = [](uint64_t have, uint64_t want) {
      uint64_t n = std::max<uint64_t>(have, 1024);
      while (n < want) n <<= 1;
      if (n > 0x7FFFFFFFull) throw Error("determinize: more than 2^31 states, elements, arcs or level candidates");
      return n;
    };
    const uint64_t ns = up(cap.states, states), ne = up(cap.elts, elts), na = up(cap.arcs, arcs), nc = up(cap.cands, cands);
    if (tally && so.p && ns > cap.states) tally->grow_states += 1;
    if (tally && se.p && ne > cap.elts) tally->grow_elts += 1;
    if (tally && oarc.p && na > cap.arcs) tally->grow_arcs += 1;
    if (tally && ca.p && nc > cap.cands) tally->grow_cands += 1;
    if (ns > cap.states || !so.p) {
      grow(pool, so, ns + 1, c.hi + 1, st);
      grow(pool, aoff, ns + 1, c.lo, st);
      grow(pool, ofin, ns, c.lo, st);
      grow(pool, hnext, ns, c.hi, st);
      grow(pool, lsc, ns + 1, 0, st);
      cap.states = (uint32_t)ns;
    }
    if (ne > cap.elts || !se.p) {
      grow(pool, se, ne, c.n_elts, st);
      cap.elts = (uint32_t)ne;
    }
    if (na > cap.arcs || !oarc.p) {
      grow(pool, oarc, na, c.n_arcs, st);
      cap.arcs = (uint32_t)na;
    }
    if (nc > cap.cands || !ca.p) {
      for (DBuf<uint4>* b : {&ca, &cb, &crec}) grow(pool, *b, nc, 0, st);
      grow(pool, ce, nc, 0, st);
      for (DBuf<uint32_t>* b : {&cst, &cdest, &cslot}) grow(pool, *b, nc, 0, st);
      for (DBuf<uint64_t>* b : {&chash, &sc1, &sc2}) grow(pool, *b, nc + 1, 0, st);
      cap.cands = (uint32_t)nc;
      cap.ltab = pow2_at_least(2 * nc, "determinize");
      grow(pool, lkey, cap.ltab, 0, st);
      grow(pool, lead, 2 * (size_t)cap.ltab, 0, st);
    }
    const uint32_t slots = pow2_at_least(2 * (uint64_t)cap.states, "determinize");
    if (slots > cap.slots) {
      DBuf<uint64_t> nk(pool, slots);
      DBuf<uint32_t> nh(pool, slots);
      HIP_CHECK(hipMemsetAsync(nk.p, 0xFF, (size_t)slots * sizeof(uint64_t), st));
      HIP_CHECK(hipMemsetAsync(nh.p, 0xFF, (size_t)slots * sizeof(uint32_t), st));
      if (cap.slots) {
        det_rehash_kernel<<<std::min<uint32_t>((cap.slots + TPB - 1) / TPB, 1024), TPB, 0, st>>>(hkey.p, hhead.p, cap.slots, nk.p,
                                                                                                  nh.p, slots);
        HIP_CHECK(hipGetLastError());
        if (tally) tally->rehashes += 1;
      }
      hkey = std::move(nk);
      hhead = std::move(nh);
      cap.slots = slots;
    }
  }
  Det view(const wfst_fst* f, float delta) {
    return Det{f->dev.offsets, f->dev.arcs, f->dev.finals, delta, so.p, se.p, aoff.p, ofin.p, oarc.p, hkey.p, hhead.p,
               hnext.p, lsc.p, ca.p, cb.p, ce.p, crec.p, chash.p, cst.p, cdest.p, cslot.p, sc1.p, sc2.p, lkey.p,
               lead.p, ctl.p, cap};
  }
};

}  // namespace

// out_dist of determinize_with_distance for ONE result: in_dist on the device, the answer on the host
struct DistReq {
  const float* d_in;
  uint32_t n_in;
  std::vector<float>* out;  // resized to the result's state count
};
// determinize_with_config for an acceptor (determinize_static.rs:176-190, the DeterminizeFsa branch): a NEW handle
static wfst_fst* determinize_acceptor(wfst_ctx* ctx, const wfst_fst* f, float delta, uint32_t det_type,
                                      const DistReq* dq = nullptr);
static const char* const NOT_ACCEPTOR_MSG =
    "determinize: transducers are not supported (the property word does not contain ACCEPTOR); use rustfst's determinize";
static const char* const LIMIT_MSG = "determinize: more than 16 M states (the input does not determinize?)";
static uint32_t max_states_knob() {
  uint32_t max_states = 1u << 24;  // the host restatement's limits (nshortest.hip): 16 M states, 256 M elements
  if (const char* e = std::getenv("WFST_DETERMINIZE_MAX_STATES")) {  // tests: reach the guard in seconds
    const long v = std::atol(e);
    if (v > 0 && (uint64_t)v < max_states) max_states = (uint32_t)v;
  }
  return max_states;
}
static uint32_t level_budget_knob() {  // levels of one det_narrow_kernel launch
  uint32_t budget = NARROW_LEVELS_PER_LAUNCH;
  if (const char* e = std::getenv("WFST_DETERMINIZE_LEVEL_BUDGET")) {  // tests: reach the budget exit with a short input
    const long v = std::atol(e);
    if (v > 0 && (uint64_t)v < budget) budget = (uint32_t)v;
  }
  return budget;
}

wfst_fst* determinize_fst(wfst_ctx* ctx, const wfst_fst* f, float delta, uint32_t det_type) {
  // the reference branches on the STORED word (determinize_static.rs:181-185): anything else takes the gallic path
  if (!(f->props & props::ACCEPTOR)) throw Error(NOT_ACCEPTOR_MSG);
  return determinize_acceptor(ctx, f, delta, det_type);
}

// optimize.hip: a machine whose every arc carries ilabel == olabel >= 1 (encode(EncodeLabels)) and whose word has lost
// ACCEPTOR.  The reference's gallic branch yields what the acceptor construction yields on such a machine;
// the word is the gallic call's: determinize_properties on the word as it is, without ACCEPTOR.
wfst_fst* determinize_encoded_fst(wfst_ctx* ctx, const wfst_fst* f, float delta, uint32_t det_type) {
  return determinize_acceptor(ctx, f, delta, det_type);
}

static wfst_fst* determinize_acceptor(wfst_ctx* ctx, const wfst_fst* f, float delta, uint32_t det_type, const DistReq* dq) {
  const uint64_t out_props = props::determinize(f->props, det_type != 1);
  wfst_ctx::DeterminizeStats& tally = ctx->det_stats;  // (wfst_ctx_get_determinize_stats: this call's, also when it ends KO)
  tally = wfst_ctx::DeterminizeStats{};
  if (f->start < 0 || f->n_states == 0) {  // compute_start -> None: the empty FST (lazy_fst.rs:229-232)
    HostCsr h;
    h.offsets.push_back(0);
    if (dq) dq->out->clear();
    return make_host_fst(ctx, 0, -1, out_props, std::move(h));
  }
  ensure_device(const_cast<wfst_fst*>(f));
  const Path path = path_knob("WFST_DETERMINIZE_PATH");
  const uint32_t max_states = max_states_knob(), budget = level_budget_knob();
  hipStream_t st = ctx->stream;
  Run run(*ctx->pool, st);
  run.tally = &tally;
  run.cap.max_states = max_states;
  run.cap.max_elts = 1u << 28;
  run.ctl = DBuf<Ctl>(*ctx->pool, 1);
  Ctl c{};
  c.lo = 0;
  c.hi = 1;
  c.n_elts = 1;
  run.reserve(1024, 4096, 4096, 4096, c);
  HIP_CHECK(hipMemcpyAsync(run.ctl.p, &c, sizeof(Ctl), hipMemcpyHostToDevice, st));
  det_seed_kernel<<<1, 1, 0, st>>>(run.view(f, delta), (uint32_t)f->start);
  HIP_CHECK(hipGetLastError());
  const uint32_t G = std::max<uint32_t>(1, std::min<uint32_t>(1024, (uint32_t)ctx->n_cus * 4));
  run.part = DBuf<uint64_t>(*ctx->pool, G + 1);
  auto read_ctl = [&] {
    HIP_CHECK(hipMemcpyAsync(&c, run.ctl.p, sizeof(Ctl), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
  };
  // every pass of this loop completes at least one level or grows the arrays (bounded by the state limit)
  for (;;) {
    if (c.err) throw Error(LIMIT_MSG);
    const uint32_t L = c.hi - c.lo;
    if (L == 0) break;
    if (c.need) {  // room for the level that could not start (K slots; every state of it may add K more)
      const uint64_t K = std::max<uint64_t>(c.K, 1);
      run.reserve((uint64_t)c.hi + K + 1, (uint64_t)c.n_elts + K, (uint64_t)c.n_arcs + K, K, c);
      c.need = 0;
      HIP_CHECK(hipMemcpyAsync(run.ctl.p, &c, sizeof(Ctl), hipMemcpyHostToDevice, st));
    }
    const Det d = run.view(f, delta);
    const bool narrow = path == Path::Narrow || (path == Path::Auto && L <= NARROW_STATES);
    if (narrow) {
      const uint32_t ml = path == Path::Narrow ? 0xFFFFFFFFu : NARROW_STATES;
      const uint32_t mk = path == Path::Narrow ? 0xFFFFFFFFu : NARROW_CANDS;
      det_narrow_kernel<<<1, TPB, 0, st>>>(d, ml, mk, budget);
      HIP_CHECK(hipGetLastError());
      read_ctl();
      tally.narrow_launches += 1;
      if (c.exit == 1) (c.hi - c.lo > NARROW_STATES ? tally.exit_wide_states : tally.exit_wide_cands) += 1;
      tally.exit_budget += c.exit == 2;
      tally.exit_need += c.exit == 3;
      tally.exit_done += c.exit == 4;
      if (!(c.exit == 1 && path == Path::Auto)) continue;  // else a level too wide for one workgroup: it runs wide
    }
    // one wide level (after a narrow launch `L`, hence `grid`, is still the size of the level that launch began with, not of
    // the level it stopped at: every phase strides by its grid, so `grid` only has to be >= 1)
    const uint32_t grid = std::max<uint32_t>(1, std::min<uint32_t>((L + TPB - 1) / TPB, (uint32_t)ctx->n_cus * 4));
    det_count_kernel<<<grid, TPB, 0, st>>>(d);
    det_scan_part_kernel<<<G, TPB, 0, st>>>(d, d.lsc, run.part.p, 0);
    det_scan_top_kernel<<<1, TPB, 0, st>>>(d, run.part.p, G, 0);
    det_scan_apply_kernel<<<G, TPB, 0, st>>>(d, d.lsc, run.part.p, G, 0);
    det_check_kernel<<<1, 1, 0, st>>>(d);
    HIP_CHECK(hipGetLastError());
    read_ctl();
    if (!c.err && c.need) tally.wide_need += 1;
    if (c.err || c.need) continue;
    const uint32_t gk = std::max<uint32_t>(1, std::min<uint32_t>((c.K + TPB - 1) / TPB, (uint32_t)ctx->n_cus * 8));
    const uint32_t gt = std::max<uint32_t>(1, std::min<uint32_t>((c.T + TPB - 1) / TPB, (uint32_t)ctx->n_cus * 8));
    det_clear_kernel<<<gt, TPB, 0, st>>>(d);
    det_expand_kernel<<<grid, TPB, 0, st>>>(d);
    det_lookup_kernel<<<gk, TPB, 0, st>>>(d);
    HIP_CHECK(hipGetLastError());
    // rounds: two per look at the control block (most levels need one: exact duplicates and older states)
    uint32_t r = 0;
    for (;;) {
      for (int k = 0; k < 2; ++k, ++r) {
        det_round_a_kernel<<<gk, TPB, 0, st>>>(d, r);
        det_round_b_kernel<<<gk, TPB, 0, st>>>(d, r);
      }
      HIP_CHECK(hipGetLastError());
      read_ctl();
      if (c.rem == 0) break;
      if (r > c.K + 2) throw Error("determinize: resolve rounds did not converge");
    }
    det_flags_kernel<<<gk, TPB, 0, st>>>(d);
    for (uint64_t* v : {d.sc1, d.sc2}) {
      det_scan_part_kernel<<<G, TPB, 0, st>>>(d, v, run.part.p, 1);
      det_scan_top_kernel<<<1, TPB, 0, st>>>(d, run.part.p, G, 1);
      det_scan_apply_kernel<<<G, TPB, 0, st>>>(d, v, run.part.p, G, 1);
    }
    det_number_kernel<<<std::max(gk, grid), TPB, 0, st>>>(d);
    det_advance_kernel<<<1, 1, 0, st>>>(d);
    HIP_CHECK(hipGetLastError());
    read_ctl();
    tally.wide_levels += 1;
    tally.rounds_max = std::max<uint64_t>(tally.rounds_max, r);
  }
  tally.levels = c.levels;
  tally.cap_states = run.cap.states;
  tally.cap_elts = run.cap.elts;
  tally.cap_arcs = run.cap.arcs;
  tally.cap_cands = run.cap.cands;
  // CSR: aoff[N] = number of arcs
  const uint32_t N = c.hi;
  HIP_CHECK(hipMemcpyAsync(run.aoff.p + N, &c.n_arcs, sizeof(uint32_t), hipMemcpyHostToDevice, st));
  if (dq) {  // one job: every state of the result
    const DistJob job{run.so.p, run.se.p, dq->d_in, dq->n_in};
    const uint32_t off[2] = {0, N};
    DBuf<DistJob> d_job(*ctx->pool, 1);
    DBuf<uint32_t> d_off(*ctx->pool, 2);
    DBuf<float> d_out(*ctx->pool, N);
    HIP_CHECK(hipMemcpyAsync(d_job.p, &job, sizeof(job), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(d_off.p, off, sizeof(off), hipMemcpyHostToDevice, st));
    det_dist_kernel<<<std::max<uint32_t>(1, std::min<uint32_t>((N + TPB - 1) / TPB, 1024)), TPB, 0, st>>>(d_job.p, d_off.p, 1, d_out.p);
    HIP_CHECK(hipGetLastError());
    dq->out->resize(N);
    HIP_CHECK(hipMemcpyAsync(dq->out->data(), d_out.p, (size_t)N * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
  }
  HIP_CHECK(hipStreamSynchronize(st));
  return adopt_device(ctx, N, c.n_arcs, 0, out_props, run.aoff.p, run.oarc.p, run.ofin.p);
}

// ---------------------------------------------------------------- batch (wfst_determinize_batch)
namespace {
struct Slice {  // capacities of one item's slice of the launch's slab
  uint64_t states, elts, arcs, cands;
};
struct Done {  // a finished item: its result arrays inside the slab of the launch that finished it
  uint32_t N = 0, n_arcs = 0;
  const uint32_t *aoff = nullptr, *so = nullptr;
  const wfst_tr* oarc = nullptr;
  const float* ofin = nullptr;
  const uint2* se = nullptr;
};
// carves one item's arrays out of the slab: every array 64-byte aligned; d == nullptr only measures
size_t carve_slice(Slab s, const Slice& sl, const wfst_fst* f, float delta, uint32_t max_states, Det* d) {
  const uint32_t slots = pow2_at_least(2 * sl.states, "determinize"), ltab = pow2_at_least(2 * sl.cands, "determinize");
  Det v{};
  v.so = s.take<uint32_t>(sl.states + 1);
  v.aoff = s.take<uint32_t>(sl.states + 1);
  v.ofin = s.take<float>(sl.states);
  v.hnext = s.take<uint32_t>(sl.states);
  v.lsc = s.take<uint64_t>(sl.states + 1);
  v.se = s.take<uint2>(sl.elts);
  v.oarc = s.take<wfst_tr>(sl.arcs);
  v.hkey = s.take<uint64_t>(slots);
  v.hhead = s.take<uint32_t>(slots);
  v.ca = s.take<uint4>(sl.cands);
  v.cb = s.take<uint4>(sl.cands);
  v.crec = s.take<uint4>(sl.cands);
  v.ce = s.take<uint2>(sl.cands);
  v.chash = s.take<uint64_t>(sl.cands);
  v.sc1 = s.take<uint64_t>(sl.cands + 1);
  v.sc2 = s.take<uint64_t>(sl.cands + 1);
  v.lkey = s.take<uint64_t>(ltab);
  v.cst = s.take<uint32_t>(sl.cands);
  v.cdest = s.take<uint32_t>(sl.cands);
  v.cslot = s.take<uint32_t>(sl.cands);
  v.lead = s.take<uint32_t>(2 * (size_t)ltab);
  if (d) {
    v.off = f->dev.offsets;
    v.arcs = f->dev.arcs;
    v.fin = f->dev.finals;
    v.delta = delta;
    v.cap = Caps{(uint32_t)sl.states, (uint32_t)sl.elts, (uint32_t)sl.arcs, (uint32_t)sl.cands, slots, ltab, max_states, 1u << 28};
    *d = v;
  }
  return s.at();
}
bool lds_scratch_knob() {
  const char* e = std::getenv("WFST_DETERMINIZE_BATCH_SCRATCH");
  if (!e || !*e) return WFST_DETERMINIZE_BATCH_LDS_DEFAULT;
  if (!std::strcmp(e, "lds")) return true;
  if (!std::strcmp(e, "global")) return false;
  throw Error(std::string("WFST_DETERMINIZE_BATCH_SCRATCH: expected lds or global, not '") + e + "'");
}
}  // namespace

// the host loop is batch_driver.h's, with the grow loop and without a slab limit
void determinize_batch(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, float delta, uint32_t det_type, wfst_fst** outs,
                       uint8_t* in_kernel, const float* const* in_dist, const uint64_t* n_in_dist, std::vector<float>* out_dist,
                       std::vector<uint64_t>* out_off) {
  ctx->det_batch = {};
  // (no check_items_owned: this call has never refused an item of another device or context)
  // every stored word before anything is launched
  for (size_t i = 0; i < n; ++i)
    if (!(fsts[i]->props & props::ACCEPTOR)) throw Error("item " + std::to_string(i) + ": " + NOT_ACCEPTOR_MSG);
  const bool use_lds = lds_scratch_knob(), min_arena = arena_min_knob("WFST_DETERMINIZE_BATCH_ARENA");
  const uint32_t max_states = max_states_knob();
  hipStream_t st = ctx->stream;
  enum : uint8_t { OPEN, DONE, SINGLE, TRIVIAL };
  std::vector<uint8_t> state(n, OPEN);
  std::vector<Slice> slice(n);
  std::vector<Done> done(n);
  std::vector<size_t> open;
  for (size_t i = 0; i < n; ++i) {
    const wfst_fst* f = fsts[i];
    if (f->start < 0 || f->n_states == 0) {  // the empty FST: never occupies a workgroup
      state[i] = TRIVIAL;
      continue;
    }
    ensure_device(const_cast<wfst_fst*>(f));
    // from the input's sizes alone (no device read): a level of up to `cands` raw candidates on top of as many states as
    // the input has; whatever needs more reports it and runs again
    const uint64_t cands = std::min<uint64_t>(std::max<uint64_t>(f->n_arcs, 64), NARROW_CANDS);
    slice[i] = min_arena ? Slice{1, 1, 1, 1} : Slice{f->n_states + cands + 1, 2ull * f->n_states + cands, f->n_arcs + cands, cands};
    open.push_back(i);
  }
  // in_dist of every item in one upload
  DBuf<float> d_in;
  std::vector<size_t> in_at(n, 0);
  if (out_dist) {
    std::vector<float> cat;
    for (size_t i = 0; i < n; ++i) {
      in_at[i] = cat.size();
      if (n_in_dist[i]) cat.insert(cat.end(), in_dist[i], in_dist[i] + n_in_dist[i]);
    }
    d_in = DBuf<float>(*ctx->pool, cat.size());
    if (!cat.empty()) HIP_CHECK(hipMemcpyAsync(d_in.p, cat.data(), cat.size() * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));
  }
  auto n_in = [&](size_t i) { return (uint32_t)std::min<uint64_t>(n_in_dist[i], 0xFFFFFFFFull); };
  size_t first_err = n;  // the in-flight KO: the lowest index wins, thrown after the loop
  auto carve = [&](size_t i, Slab s, Det* d) { return carve_slice(s, slice[i], fsts[i], delta, max_states, d); };
  auto init = [&](size_t i) {
    Ctl c{};
    c.hi = 1;
    c.n_elts = 1;
    c.start = (uint32_t)fsts[i]->start;
    return c;
  };
  const uint32_t lds_bytes = use_lds ? (uint32_t)BATCH_LDS_BYTES : 0u;
  auto launch = [&](const Det* d_dets, uint32_t m) { det_batch_kernel<<<m, TPB, lds_bytes, st>>>(d_dets, lds_bytes); };
  auto classify = [&](size_t i, const Ctl& c, const Det& d) {
    if (c.exit == 4) {
      state[i] = DONE;
      done[i] = Done{c.hi, c.n_arcs, d.aoff, d.so, d.oarc, d.ofin, d.se};
      return BatchExit::FINISHED;
    }
    if (c.exit == 1 || c.exit == 5) {
      if (c.exit == 5) first_err = std::min(first_err, i);  // (its single path never runs: the call is KO)
      state[i] = SINGLE;
      return BatchExit::SINGLE;
    }
    if (c.exit != 3) throw Error("determinize_batch: unexpected exit code " + std::to_string(c.exit));
    Slice& sl = slice[i];
    const uint64_t K = std::max<uint64_t>(c.K, 1);
    auto up = [](uint64_t& have, uint64_t want) {
      if (want > have) have = std::max<uint64_t>(2 * have, want);
    };
    const Slice before = sl;
    up(sl.cands, K);
    up(sl.states, (uint64_t)c.hi + K + 1);
    up(sl.elts, (uint64_t)c.n_elts + K);
    up(sl.arcs, (uint64_t)c.n_arcs + K);
    if (sl.cands == before.cands && sl.states == before.states && sl.elts == before.elts && sl.arcs == before.arcs)
      return BatchExit::STUCK;
    if (sl.states > 0x7FFFFFFFull || sl.elts > 0x7FFFFFFFull || sl.arcs > 0x7FFFFFFFull)
      throw Error("determinize: more than 2^31 states, elements, arcs or level candidates");
    return BatchExit::GREW;
  };
  // every launch finishes an item, hands it to the single path, or at least doubles what its slice was short of, and the
  // limits cap the slices: a bounded number of launches
  const auto slabs = batch_launch_loop<Det, Ctl>(ctx, ctx->det_batch, {"determinize_batch", BATCH_MAX_LAUNCHES, "a slice"}, std::move(open),
                                                 carve, init, launch, classify);
  if (first_err < n) throw Error("item " + std::to_string(first_err) + ": " + LIMIT_MSG);
  std::vector<std::vector<float>> single_dist(n);
  auto outcome = [&](size_t i) {
    const uint64_t out_props = props::determinize(fsts[i]->props, det_type != 1);
    if (state[i] == SINGLE) return BatchOutcome::single();  // a level too wide for one workgroup
    if (state[i] == DONE) return BatchOutcome::adopt({done[i].N, done[i].n_arcs, 0, out_props, done[i].aoff, done[i].oarc, done[i].ofin});
    HostCsr h;
    h.offsets.push_back(0);
    return BatchOutcome::handle(make_host_fst(ctx, 0, -1, out_props, std::move(h)));
  };
  auto single = [&](size_t i) {
    if (!out_dist) return determinize_acceptor(ctx, fsts[i], delta, det_type);
    const DistReq dq{d_in.p + in_at[i], n_in(i), &single_dist[i]};
    return determinize_acceptor(ctx, fsts[i], delta, det_type, &dq);
  };
  // out_dist: one distance launch for the items the kernel finished (idx), the single path's own for the others
  auto distances = [&](const std::vector<size_t>& idx) {
    if (!out_dist) return;
    std::vector<float> kd;  // out_dist of the kernel's items, in idx order
    std::vector<uint32_t> koff(idx.size() + 1, 0);
    if (!idx.empty()) {
      std::vector<DistJob> jobs(idx.size());
      uint64_t tot = 0;
      for (size_t k = 0; k < idx.size(); ++k) {
        const size_t i = idx[k];
        jobs[k] = DistJob{done[i].so, done[i].se, d_in.p + in_at[i], n_in(i)};
        tot += done[i].N;
        if (tot > 0x7FFFFFFFull) throw Error("determinize_batch: more than 2^31 result states in one batch");
        koff[k + 1] = (uint32_t)tot;
      }
      DBuf<DistJob> d_jobs(*ctx->pool, jobs.size());
      DBuf<uint32_t> d_off(*ctx->pool, koff.size());
      DBuf<float> d_out(*ctx->pool, tot);
      HIP_CHECK(hipMemcpyAsync(d_jobs.p, jobs.data(), jobs.size() * sizeof(DistJob), hipMemcpyHostToDevice, st));
      HIP_CHECK(hipMemcpyAsync(d_off.p, koff.data(), koff.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
      det_dist_kernel<<<(uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((tot + TPB - 1) / TPB, 1024)), TPB, 0, st>>>(
          d_jobs.p, d_off.p, (uint32_t)jobs.size(), d_out.p);
      HIP_CHECK(hipGetLastError());
      kd.resize(tot);
      HIP_CHECK(hipMemcpyAsync(kd.data(), d_out.p, tot * sizeof(float), hipMemcpyDeviceToHost, st));
      HIP_CHECK(hipStreamSynchronize(st));
    }
    out_off->assign(n + 1, 0);
    for (size_t i = 0; i < n; ++i) (*out_off)[i + 1] = (*out_off)[i] + (state[i] == SINGLE ? outs[i]->n_states : done[i].N);
    out_dist->assign((*out_off)[n], 0.0f);
    for (size_t k = 0; k < idx.size(); ++k)
      std::copy(kd.begin() + koff[k], kd.begin() + koff[k + 1], out_dist->begin() + (*out_off)[idx[k]]);
    for (size_t i = 0; i < n; ++i)
      if (state[i] == SINGLE) std::copy(single_dist[i].begin(), single_dist[i].end(), out_dist->begin() + (*out_off)[i]);
  };
  batch_finish(ctx, ctx->det_batch, n, outs, in_kernel, outcome, single, distances);
}

// determinize_with_distance (determinize_static.rs:24-39): the Functional construction and out_dist, for one acceptor
wfst_fst* determinize_with_distance_fst(wfst_ctx* ctx, const wfst_fst* f, const float* in_dist, uint64_t n_in_dist, float delta,
                                        std::vector<float>& out_dist) {
  if (!(f->props & props::ACCEPTOR)) throw Error(NOT_ACCEPTOR_MSG);
  DBuf<float> d_in(*ctx->pool, n_in_dist);
  if (n_in_dist) {
    HIP_CHECK(hipMemcpyAsync(d_in.p, in_dist, n_in_dist * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
  }
  const DistReq dq{d_in.p, (uint32_t)std::min<uint64_t>(n_in_dist, 0xFFFFFFFFull), &out_dist};
  return determinize_acceptor(ctx, f, delta, 0, &dq);
}

}  // namespace wfst
