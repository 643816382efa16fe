// compose.hip — composition (+ trim, + fused n=1 shortest path) of HBM-resident CSR FSTs.
//
// Replaces, for SortedMatcher x2 + SequenceComposeFilter (the AutoFilter default):
//   compose / compose_with_config      rustfst/src/algorithms/compose/compose_static.rs:166-306
//   ComposeFstOp::{compute_start,compute_trs,compute_final_weight,match_input,ordered_expand,
//                  match_tr,match_tr_selected,add_tr}   compose/compose_fst_op.rs:199-449
//   SortedMatcher / IteratorSortedMatcher / eps_loop   compose/matchers/sorted_matcher.rs:44-184, matchers/mod.rs:98-105
//   SequenceComposeFilter::{set_state,filter_tr}       compose/compose_filters/sequence_compose_filter.rs:134-171
//   StateTable::find_id                                 lazy/state_table.rs:49-59,102-119
//   LazyFst::compute (FIFO BFS = the state numbering)   lazy/lazy_fst.rs:226-269
//   connect + del_states                                connect.rs:51-66, vector_fst/mutable_fst.rs:132-189
//
// Execution model ("one wavefront = one composition problem"): the reference is a sequential BFS whose
// state ids are first-touch order.  A 64-lane wave walks that BFS level by level for ONE (fst1,fst2)
// pair; a launch runs one wave per problem, so a batch of acceptors against a shared transducer fills
// the chip with independent waves (8 XCDs x 32 CUs x up to 32 waves) and needs no inter-workgroup
// synchronisation at all.  Inside a level the 64 lanes share the work of one composed state:
//   - the searched side's arc block (<= 64 arcs) is read with ONE coalesced 16-B-per-lane load and kept
//     in registers; label matching is a wave ballot, matched arcs are fetched with lane shuffles
//     (no second trip to HBM); larger blocks fall back to a per-lane binary search;
//   - emitted arcs get their slot by a wave prefix sum, destination tuples go through an
//     open-addressing table (u64 key CAS) whose value word holds atomicMin(first emission index);
//   - after the level, first occurrences are ranked with ballots: new ids = reference BFS ids.
// Everything stays in HBM/L2 between phases: the fused pipeline (compose -> relax -> backtrace) never
// returns to the host.
#include <chrono>
#include <cstdlib>
#include <cstring>

#include "batch_driver.h"
#include "common.h"
#include "compose_match.h"
#include "fst_props.h"
#include "host_parallel.h"
#include "string_placement.h"

namespace wfst {

namespace {

// bits of the 4th word of a state record (fst_store.hip derive_noeps_kernel; common.h SREC_*)
using wfst::SREC_ALL_IEPS;
using wfst::SREC_ALL_OEPS;
using wfst::SREC_NO_IEPS;
using wfst::SREC_NO_OEPS;
constexpr uint64_t HT_EMPTY = ~0ull;
constexpr uint32_t HV_INIT = 0xFFFFFFFFu;
constexpr uint32_t HV_PEND = 0x80000000u;
constexpr uint64_t KEY_INF = ~0ull;

enum : uint32_t {
  ST_OK = 0, ST_OVERFLOW_STATES = 1, ST_OVERFLOW_ARCS = 2, ST_OVERFLOW_HASH = 3, ST_OVERFLOW_PATH = 4,
  ST_NOT_A_STRING_CASE = 5,  // the string o T kernel met a case it does not cover: redo on the general kernel
  ST_SWITCH_WIDE = 6,        // a frontier too wide for one wave: compose() redoes the pair on the wide driver
  ST_TIE_ORDER = 7           // fused shortest path: a state of the path has no predecessor tight in the hop count (inexact
                             // f32 sums, sssp.hip parent_class): the host redoes the problem as compose + shortest_path
};
enum : uint32_t { FLAG_TRIM = 1, FLAG_SP = 2 };

struct FstView {
  const uint32_t* offsets;
  const wfst_tr* arcs;
  const float* finals;
  const uint32_t* noeps;
  const uint4* srec;   // {arc begin, arc count, final bits, SREC_* epsilon facts}
  const uint2* anext;  // per arc {arc begin, arc count} of its destination state (string o T kernel only), or null
  uint32_t n_states;
  int32_t start;  // -1 = None
  uint64_t n_arcs;
};

struct ProblemDesc {
  FstView f1;
  uint32_t mode;
  uint32_t filter;  // ComposeFilterEnum value (compose_static.rs:19-33); 0 (Auto) == 3 (Sequence)
  // string_compose_sp_kernel: where this problem's path arcs go in the packed path buffer.  Handed out by the host
  // (launch_begin: a path has n_states - 1 arcs at most, known before the launch); compose_wave_kernel draws from a cursor.
  uint32_t path_off;
};

struct Caps {
  uint32_t S;  // composed states
  uint32_t A;  // composed arcs
  uint32_t H;  // hash slots (power of two)
  uint32_t W;  // give up (ST_SWITCH_WIDE) when a BFS level adds more states than this; 0 = never
};

struct Result {
  uint32_t status;
  uint32_t n_states, n_arcs;  // pre-trim
  uint32_t t_states, t_arcs;  // after trim (== pre-trim when not trimming)
  int32_t t_start;
  uint32_t has_path, hops;
  float final_weight, total;
  uint32_t path_off;  // offset of the path arcs in the packed path buffer
  uint32_t n_levels;
  uint32_t facts;     // string_compose_sp_kernel: OR of the path arcs' property facts (fst_props.h: path_arc_facts), or
                      // PATH_FACTS_NONE: the host knows the path FST's properties without reading its arcs back
  uint32_t run_levels, runs;  // string_compose_sp_kernel: levels taken inside chase runs, and the number of runs (0 elsewhere)
  uint32_t pair_levels, pair_splits;  // ... levels the run's loop carried that are not run levels (a frontier of two states, or one
                                      // state that matches two arcs), and those of them with two matches (0 elsewhere)
  uint32_t done;     // string_compose_sp_kernel, results in pinned memory: the run's ticket, written after everything else of
                      // the problem (system-scope fence in between): the host waits for these words instead of the stream
#ifdef WFST_PHASE_TIMING
  unsigned long long dbg[8];
  uint32_t hw_id, xcc_id;  // where the wave ran: HW_REG_HW_ID (wave 3:0, SIMD 5:4, CU 11:8, SH 12, SE 15:13) and HW_REG_XCC_ID (3:0)
#endif
};

struct Arena {
  uint64_t* tuples;   // [S]   packed (fs<<63 | s1<<32 | s2)
  uint64_t* hkeys;    // [H]
  uint64_t* skey;     // [S]   shortest-path key (enc(d)<<32 | hops)
  uint64_t* parent;   // [S]
  wfst_tr* arcs;      // [A]   composed arcs (pre-trim), nextstate patched level by level
  wfst_tr* t_arcs;    // [A]   trimmed arcs
  uint32_t* hvals;    // [H]
  uint32_t* off;      // [S+1]
  uint32_t* t_off;    // [S+1]
  float* fin;         // [S]
  float* t_fin;       // [S]
  uint32_t* aux;      // [S]   coaccessible flag / mark
  uint32_t* aux2;     // [S]   new id / jump pointer
  uint32_t* lvl;      // [S+1] first id of each BFS level
};

__host__ __device__ inline size_t al16(size_t x) { return (x + 15) & ~(size_t)15; }
// one problem's arena (a batch = arena_bytes(caps) apart); *bytes_out, when asked for, is its size
__host__ __device__ inline Arena carve_arena(char* base, const Caps& c, size_t* bytes_out = nullptr) {
  Arena a;
  char* p = base;
  a.tuples = (uint64_t*)p; p += al16((size_t)c.S * 8);
  a.hkeys = (uint64_t*)p; p += al16((size_t)c.H * 8);
  a.skey = (uint64_t*)p; p += al16((size_t)c.S * 8);
  a.parent = (uint64_t*)p; p += al16((size_t)c.S * 8);
  a.arcs = (wfst_tr*)p; p += al16((size_t)c.A * 16);
  a.t_arcs = (wfst_tr*)p; p += al16((size_t)c.A * 16);
  a.hvals = (uint32_t*)p; p += al16((size_t)c.H * 4);
  a.off = (uint32_t*)p; p += al16((size_t)(c.S + 1) * 4);
  a.t_off = (uint32_t*)p; p += al16((size_t)(c.S + 1) * 4);
  a.fin = (float*)p; p += al16((size_t)c.S * 4);
  a.t_fin = (float*)p; p += al16((size_t)c.S * 4);
  a.aux = (uint32_t*)p; p += al16((size_t)c.S * 4);
  a.aux2 = (uint32_t*)p; p += al16((size_t)c.S * 4);
  a.lvl = (uint32_t*)p; p += al16((size_t)(c.S + 1) * 4);
  if (bytes_out) *bytes_out = ((size_t)(p - base) + 255) & ~(size_t)255;
  return a;
}
inline size_t arena_bytes(const Caps& c) {
  size_t b = 0;
  carve_arena(nullptr, c, &b);
  return b;
}

// ComposeStateTuple {fs, s1, s2} in one u64: fs (0..2) : 2 | s1 : 30 | s2 : 32
constexpr uint32_t TUPLE_S1_MASK = 0x3FFFFFFFu;
__device__ __forceinline__ uint64_t pack_tuple(uint32_t fs, uint32_t s1, uint32_t s2) {
  return ((uint64_t)fs << 62) | ((uint64_t)s1 << 32) | s2;
}
__device__ __forceinline__ uint32_t tuple_s1(uint64_t tk) { return (uint32_t)(tk >> 32) & TUPLE_S1_MASK; }

// StateTable::find_id (lazy/state_table.rs:49-59) as an open-addressing table.  The value word is
// atomicMin(first emission index of this level) while the tuple is new, then its final id.
__device__ __forceinline__ uint32_t ht_insert(uint64_t* hkeys, uint32_t* hvals, uint32_t hmask, uint64_t key,
                                              uint32_t pend) {
  uint32_t slot = (uint32_t)mix64(key) & hmask;
  for (uint32_t probes = 0; probes <= hmask; ++probes) {
    const uint64_t k = hkeys[slot];  // may be a stale EMPTY: the CAS below is the arbiter
    if (k == key) break;
    if (k == HT_EMPTY) {
      const uint64_t prev = atomicCAS((unsigned long long*)&hkeys[slot], (unsigned long long)HT_EMPTY,
                                      (unsigned long long)key);
      if (prev == HT_EMPTY || prev == key) break;
    }
    slot = (slot + 1) & hmask;
  }
  atomicMin(&hvals[slot], pend);
  return slot;
}

// Optional per-phase cycle accounting (build with -DWFST_PHASE_TIMING; results land in Result::dbg).
#ifdef WFST_PHASE_TIMING
#define PT_DECL unsigned long long pt_t = clock64(), pt_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#define PT_MARK(k)                              \
  {                                             \
    const unsigned long long pt_n = clock64();  \
    pt_acc[k] += pt_n - pt_t;                   \
    pt_t = pt_n;                                \
  }
// (s_getreg's operand: register id | first bit << 6 | (bits - 1) << 11; HW_REG_HW_ID is 4, HW_REG_XCC_ID 20)
#define PT_STORE(res)                                                          \
  for (int pt_i = 0; pt_i < 8; ++pt_i) (res).dbg[pt_i] = pt_acc[pt_i];        \
  (res).hw_id = __builtin_amdgcn_s_getreg(4 | (0 << 6) | (31 << 11));          \
  (res).xcc_id = __builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11));
// (string_compose_sp_kernel: the rows asked for so far have arrived.  The wait is part of the timing build only: it ends the
// overlap the real kernel has, so such a build gives the SHARES of a level, not its length)
#define PT_ROWS_IN() asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#else
#define PT_DECL
#define PT_MARK(k)
#define PT_STORE(res)
#define PT_ROWS_IN()
#endif

struct Level {
  uint32_t arc_begin;  // first emitted arc of the level
  uint32_t hi;         // number of ids assigned before this level's new states
};

// LDS staging of ONE BFS level when it emits <= 64 arcs (the common case for acceptor o transducer
// lattices): the level's arcs, destination tuples and shortest-path candidates stay on-chip, duplicates
// are resolved with lane shuffles, and only first occurrences touch the hash table.
struct FastStage {
  uint32_t il[64], ol[64];
  float w[64];
  uint64_t key[64];   // destination tuple
  uint64_t cand[64];  // shortest-path candidate key of the destination through this arc
  uint64_t nkey[64];  // compacted new states (next frontier): tuple
  uint64_t nsk[64];   //                                        shortest-path key
  uint4 nr1[64];      //                                        state record in fst1 (prefetched)
  uint4 nr2[64];      //                                        state record in fst2 (prefetched)
};

enum : int { EXP_OK = 0, EXP_ARENA_OVERFLOW = 1, EXP_FAST_OVERFLOW = 2 };

// ComposeFstOp::compute_trs + compute_final_weight for composed state q = tuple `tk`
// (compose_fst_op.rs:406-449).
//  FAST = false: appends q's arcs at arcs[*n_arcs ...]; destination = hash slot (patched to the id after
//                the level is ranked).
//  FAST = true : stages the arcs in LDS at stg[*level_cnt ...]; nothing touches the hash table here.
template <bool FAST>
__device__ int expand_state(const FstView& f1, const FstView& f2, uint32_t mode, uint32_t filter, const Arena& ar,
                            const Caps& caps,
                            uint32_t q, uint64_t tk, uint4 r1, uint4 r2, uint64_t src_sk, const Level& lv,
                            uint32_t* n_arcs_io, FastStage* stg, uint32_t* level_cnt_io, uint32_t* status) {
  const uint32_t lane = lane_id();
  const uint32_t hmask = caps.H - 1;
  const uint32_t fs = (uint32_t)(tk >> 62);
  const uint32_t s1 = tuple_s1(tk);
  const uint32_t s2 = (uint32_t)tk;
  // r1 / r2 = the 16-byte state records {arc begin, arc count, final bits, noeps} of s1 in fst1 / s2 in fst2
  const uint32_t b1 = r1.x, b2 = r2.x;
  const uint32_t n1 = r1.y, n2 = r2.y;
  const float fin1 = __uint_as_float(r1.z), fin2 = __uint_as_float(r2.z);
  // compute_final_weight :420-449 (final1 (x) final2; None when either is None / the product is zero)
  if (lane == 0) ar.fin[q] = (fin1 != INF && fin2 != INF) ? wtimes(fin1, fin2) : INF;
  // set_state of the filters (sequence_compose_filter.rs:134-148, alt_sequence_compose_filter.rs:143-158,
  // match_compose_filter.rs:126-147): fst1 looks at its OUTPUT epsilons, fst2 at its INPUT epsilons; the state
  // record carries the four facts as bits (SREC_*)
  const bool alleps1 = (r1.w & SREC_ALL_OEPS) && !(fin1 != INF);
  const bool noeps1 = (r1.w & SREC_NO_OEPS) != 0;
  const bool alleps2 = (r2.w & SREC_ALL_IEPS) && !(fin2 != INF);
  const bool noeps2 = (r2.w & SREC_NO_IEPS) != 0;
  // match_input :199-219 (SortedMatcher::priority = num_trs)
  const bool mi = mode == MODE_BOTH ? (n1 <= n2) : (mode == MODE_INPUT);
  const wfst_tr* it_arcs = mi ? f1.arcs + b1 : f2.arcs + b2;
  const wfst_tr* se_arcs = mi ? f2.arcs + b2 : f1.arcs + b1;
  const uint32_t n_it = mi ? n1 : n2;
  const uint32_t n_se = mi ? n2 : n1;
  const uint32_t sa = mi ? s2 : s1;
  const uint32_t sb = mi ? s1 : s2;
  // filter_tr outcomes, constant per composed state; the four classes of (arc1, arc2) pairs a matcher can produce:
  //   X: arc1.olabel == NO_LABEL (fst1 stands still, fst2 takes an input-epsilon arc)
  //   Y: arc2.ilabel == NO_LABEL (fst2 stands still, fst1 takes an output-epsilon arc)
  //   Z: both real, arc1.olabel == 0 == arc2.ilabel                 M: both real, matching non-epsilon label
  const FilterOutcomes fo = filter_outcomes(filter, fs, alleps1, noeps1, alleps2, noeps2);  // compose_filters.h
  const uint32_t fsX = fo.fsX, fsY = fo.fsY, fsZ = fo.fsZ, fsM = 0u;
  const uint32_t fs_nolabel = mi ? fsX : fsY;  // iterated arc labelled NO_LABEL (the loop pseudo-arc)
  const uint32_t fs_eps = mi ? fsY : fsX;      // iterated arc labelled 0 paired with the matcher's EpsLoop

  const bool small = n_se <= 64;
  ArcReg se{0, 0, 0.0f, 0};
  uint32_t se_key = 0xFFFFFFFEu;
  if (small && lane < n_se) {
    se = load_arc<GlobalLoad>(se_arcs + lane);
    se_key = mi ? se.il : se.ol;
  }
  const float src_d = key_f32((uint32_t)(src_sk >> 32));
  const uint32_t src_h1 = (uint32_t)src_sk + 1u;

  uint32_t n_arcs = *n_arcs_io;
  uint32_t level_cnt = FAST ? *level_cnt_io : 0u;
  const uint32_t n_items = n_it + 1;  // item 0 = the loop pseudo-arc (ordered_expand :229-233)
  for (uint32_t base = 0; base < n_items; base += 64) {
    const uint32_t j = base + lane;
    const bool have = j < n_items;
    ArcReg ab{0, 0, 0.0f, 0};
    if (have) {
      if (j == 0)
        ab = mi ? ArcReg{0u, NO_LABEL, 0.0f, sb} : ArcReg{NO_LABEL, 0u, 0.0f, sb};
      else
        ab = load_arc<GlobalLoad>(it_arcs + (j - 1));
    }
    const uint32_t label = mi ? ab.ol : ab.il;                    // match_tr :333
    const uint32_t skey = label == NO_LABEL ? 0u : label;          // IteratorSortedMatcher::new :131-135
    uint32_t lo = 0, cnt = 0;
    if (small) {
      const uint32_t in_chunk = min(64u, n_items - base);
      for (uint32_t jj = 0; jj < in_chunk; ++jj) {
        const uint32_t k = rl(skey, jj);
        const uint64_t m = __ballot(lane < n_se && se_key == k);
        if (lane == jj) {
          cnt = (uint32_t)__popcll(m);
          lo = m ? (uint32_t)__ffsll((unsigned long long)m) - 1u : 0u;
        }
      }
    } else if (have) {
      equal_range<GlobalLoad>(se_arcs, n_se, mi, skey, &lo, &cnt);
    }
    uint32_t fsn;  // filter state of the emitted arcs of this item (of its real pairs when eps_item)
    bool eps_item = false;
    uint32_t loop1 = 0;  // 1: the first pair of an eps_item is the matcher's EpsLoop (accepted by the filter)
    if (!have) {
      cnt = 0;
      fsn = FILTER_REJECT;
    } else if (label == NO_LABEL) {
      fsn = fs_nolabel;  // real arcs with key 0, no EpsLoop (sorted_matcher.rs:127-139)
    } else if (label == 0u) {
      // the matcher yields EpsLoop first, then the real epsilon arcs (:124-184); the filter sees the loop as class
      // X/Y and the real ones as class Z (rejected by the sequence filters, accepted by Null/Trivial/Match)
      eps_item = true;
      loop1 = fs_eps != FILTER_REJECT ? 1u : 0u;
      fsn = fsZ;
      cnt = loop1 + (fsZ != FILTER_REJECT ? cnt : 0u);
    } else {
      fsn = fsM;
    }
    if (!eps_item && fsn == FILTER_REJECT) cnt = 0;
    uint32_t total, pos, maxcnt;
    if (__ballot(cnt > 1u) == 0) {  // every item emits 0 or 1 arc (the usual case): two ballots replace the scans
      const uint64_t em = __ballot(cnt == 1u);
      pos = lanes_below(em);
      total = (uint32_t)__popcll(em);
      maxcnt = total ? 1u : 0u;
    } else {
      pos = wave_excl_scan(cnt, lane, &total);
      maxcnt = wave_max(cnt);
    }
    if (total == 0) continue;
    if (FAST && level_cnt + total > 64u) return EXP_FAST_OVERFLOW;
    if ((FAST ? n_arcs + level_cnt : n_arcs) + total > caps.A) {
      *status = ST_OVERFLOW_ARCS;
      return EXP_ARENA_OVERFLOW;
    }
    if ((uint64_t)lv.hi + (FAST ? level_cnt : n_arcs - lv.arc_begin) + total + 64 > (uint64_t)caps.H) {
      *status = ST_OVERFLOW_HASH;
      return EXP_ARENA_OVERFLOW;
    }
    for (uint32_t m = 0; m < maxcnt; ++m) {
      ArcReg aa;
      const bool is_loop = loop1 != 0u && m == 0u;  // (loop1 is only ever set on eps items)
      if (small) {
        aa = shfl_arc(se, (lo + m - loop1) & 63u);
      } else {
        aa = ArcReg{0, 0, 0.0f, 0};
        if (m < cnt && !is_loop) aa = load_arc<GlobalLoad>(se_arcs + lo + m - loop1);
      }
      if (m < cnt) {
        const uint32_t fsn_m = is_loop ? fs_eps : fsn;
        if (is_loop) aa = mi ? ArcReg{NO_LABEL, 0u, 0.0f, sa} : ArcReg{0u, NO_LABEL, 0.0f, sa};  // eps_loop, mod.rs:98-105
        // arc1 from fst1, arc2 from fst2 (match_tr_selected :301-319); selected field by field so that the
        // structs stay in registers (a reference select would push them to scratch)
        const ArcReg a1{mi ? ab.il : aa.il, mi ? ab.ol : aa.ol, mi ? ab.w : aa.w, mi ? ab.ns : aa.ns};
        const ArcReg a2{mi ? aa.il : ab.il, mi ? aa.ol : ab.ol, mi ? aa.w : ab.w, mi ? aa.ns : ab.ns};
        const uint64_t key = pack_tuple(fsn_m, a1.ns, a2.ns);
        const float wsum = wtimes(a1.w, a2.w);  // add_tr :267-285
        if (FAST) {
          const uint32_t e = level_cnt + pos + m;
          stg->il[e] = a1.il;
          stg->ol[e] = a2.ol;
          stg->w[e] = wsum;
          stg->key[e] = key;
          uint64_t cand = KEY_INF;
          if (src_sk != KEY_INF) {
            const float c = (src_d + wsum) + 0.0f;
            if (c < INF) cand = ((uint64_t)f32_key(c) << 32) | src_h1;
          }
          stg->cand[e] = cand;
        } else {
          const uint32_t e = n_arcs + pos + m;
          const uint32_t slot = ht_insert(ar.hkeys, ar.hvals, hmask, key, HV_PEND | (e - lv.arc_begin));
          store_arc(ar.arcs + e, a1.il, a2.ol, wsum, slot);
        }
      }
    }
    if (FAST)
      level_cnt += total;
    else
      n_arcs += total;
  }
  if (FAST)
    *level_cnt_io = level_cnt;
  else
    *n_arcs_io = n_arcs;
  return EXP_OK;
}

// StateTable::find_id for a tuple seen for the first time in this level (fast path): CAS first, so a
// new tuple costs one L2 round trip.  Returns the slot; *existed tells whether an earlier level owns it.
__device__ __forceinline__ uint32_t ht_find_or_insert(uint64_t* hkeys, uint32_t hmask, uint64_t key, bool* existed) {
  uint32_t slot = (uint32_t)mix64(key) & hmask;
  for (uint32_t probes = 0; probes <= hmask; ++probes) {
    const uint64_t prev = atomicCAS((unsigned long long*)&hkeys[slot], (unsigned long long)HT_EMPTY,
                                    (unsigned long long)key);
    if (prev == HT_EMPTY) {
      *existed = false;
      return slot;
    }
    if (prev == key) {
      *existed = true;
      return slot;
    }
    slot = (slot + 1) & hmask;
  }
  *existed = false;
  return slot;
}

// One relaxation pass over states [lo, hi): lanes over states.  Returns (wave-uniform) whether any key improved.
__device__ bool relax_states(const Arena& ar, uint32_t lo, uint32_t hi, uint32_t n_arcs_total) {
  const uint32_t lane = lane_id();
  bool changed = false;
  for (uint32_t base = lo; base < hi; base += 64) {
    const uint32_t q = base + lane;
    if (q < hi) {
      const uint64_t kq = ld_l2(&ar.skey[q]);
      if (kq != KEY_INF) {
        const float d = key_f32((uint32_t)(kq >> 32));
        const uint32_t h1 = (uint32_t)kq + 1u;
        const uint32_t b = ar.off[q], e = ar.off[q + 1];
        for (uint32_t i = b; i < e && i < n_arcs_total; ++i) {
          const ArcReg a = load_arc<GlobalLoad>(ar.arcs + i);
          const float c = (d + a.w) + 0.0f;
          if (!(c < INF)) continue;
          const uint64_t ck = ((uint64_t)f32_key(c) << 32) | h1;
          const uint64_t old = atomicMin((unsigned long long*)&ar.skey[a.ns], (unsigned long long)ck);
          if (ck < old) changed = true;
        }
      }
    }
  }
  return __any(changed);
}

// One composition problem on the calling wavefront: the body of compose_wave_kernel (second operand and capacities are the
// launch's) and of compose_batch_kernel (both are the item's).  Always inlined: where an argument comes from is the
// entry's business and costs the body nothing.  `res` is filled; the entry stores it.
template <uint32_t FLAGS>
__device__ __forceinline__ void compose_wave_problem(const FstView& f1, const FstView& f2, const uint32_t mode,
                                                     const uint32_t filter, const Caps& caps, const Arena& ar, Result& res,
                                                     wfst_tr* __restrict__ path_buf, const uint32_t path_cap,
                                                     uint32_t* __restrict__ path_cursor) {
  const uint32_t lane = lane_id();
  res.status = ST_OK;
  res.n_states = res.n_arcs = res.t_states = res.t_arcs = 0;
  res.t_start = -1;
  res.has_path = res.hops = 0;
  res.final_weight = res.total = INF;
  res.path_off = 0;
  res.n_levels = 0;
  res.facts = props::PATH_FACTS_NONE;
  res.run_levels = res.runs = res.pair_levels = res.pair_splits = 0;

  __shared__ FastStage stg;
  PT_DECL
  uint32_t n_states = 0, n_arcs = 0, n_levels = 0;
  bool ok = true;
  bool needs_fixup = false;

  // compute_start :389-404
  if (f1.start >= 0 && f2.start >= 0) {
    // clear this problem's table
    for (uint32_t i = lane; i < caps.H; i += 64) {
      ar.hkeys[i] = HT_EMPTY;
      ar.hvals[i] = HV_INIT;
    }
    if (FLAGS & FLAG_SP)
      for (uint32_t i = lane; i < caps.S; i += 64) ar.skey[i] = KEY_INF;
    wave_sync();
    if (lane == 0) {
      const uint64_t key0 = pack_tuple(0u, (uint32_t)f1.start, (uint32_t)f2.start);
      const uint32_t slot = ht_insert(ar.hkeys, ar.hvals, caps.H - 1, key0, 0u);
      st_l2(&ar.hvals[slot], 0u);
      ar.tuples[0] = key0;
      if (FLAGS & FLAG_SP) ar.skey[0] = (uint64_t)f32_key(0.0f) << 32;
    }
    wave_sync();
    n_states = 1;
    uint32_t lo = 0, hi = 1;
    PT_MARK(0)  // table clear + start tuple
    // frontier in registers while it is <= 64 states wide: lane i holds state lo + i
    bool fast = true;
    uint64_t f_key = lane == 0 ? pack_tuple(0u, (uint32_t)f1.start, (uint32_t)f2.start) : 0ull;
    uint64_t f_sk = lane == 0 ? ((uint64_t)f32_key(0.0f) << 32) : KEY_INF;
    uint4 f_r1 = make_uint4(0, 0, 0, 0), f_r2 = make_uint4(0, 0, 0, 0);
    if (lane == 0) {
      f_r1 = ld_global16(f1.srec + f1.start);
      f_r2 = ld_global16(f2.srec + f2.start);
    }
    // LazyFst::compute :235-259 — FIFO BFS; level k = ids [lo, hi)
    while (lo < hi && ok) {
      if (lane == 0) ar.lvl[n_levels] = lo;
      n_levels++;
      Level lv{n_arcs, hi};
      bool did_fast = false;
      if (fast) {
        // ---------------- small-level fast path: the whole level lives in LDS / registers
        uint32_t level_cnt = 0;
        int rc = EXP_OK;
        for (uint32_t q = lo; q < hi; ++q) {
          const uint64_t tk = rl64(f_key, q - lo);
          const uint64_t ssk = rl64(f_sk, q - lo);
          if (lane == 0) ar.off[q] = n_arcs + level_cnt;
          rc = expand_state<true>(f1, f2, mode, filter, ar, caps, q, tk, rl128(f_r1, q - lo), rl128(f_r2, q - lo), ssk, lv,
                                  &n_arcs, &stg, &level_cnt, &res.status);
          if (rc != EXP_OK) break;
        }
        if (rc == EXP_ARENA_OVERFLOW) {
          ok = false;
          break;
        }
        PT_MARK(1)  // fast: expansions (state records -> arc blocks -> matches -> LDS stage)
        if (rc == EXP_OK) {
          did_fast = true;
          lds_handoff();
          const bool have = lane < level_cnt;
          uint32_t il = 0, ol = 0;
          float w = 0.0f;
          uint64_t key = HT_EMPTY, cand = KEY_INF;
          if (have) {
            il = stg.il[lane];
            ol = stg.ol[lane];
            w = stg.w[lane];
            key = stg.key[lane];
            cand = stg.cand[lane];
          }
          // speculative fetch of the destination's state records: overlaps the hash-table round trip below and
          // removes one dependent trip to HBM from the next level
          uint4 pr1 = make_uint4(0, 0, 0, 0), pr2 = make_uint4(0, 0, 0, 0);
          if (have) {
            pr1 = ld_global16(f1.srec + tuple_s1(key));
            pr2 = ld_global16(f2.srec + (uint32_t)key);
          }
          // first occurrence of each destination tuple inside the level + min candidate of its group
          uint64_t mymin = cand;
          uint32_t first = 64;
          for (uint32_t i = 0; i < level_cnt; ++i) {
            const uint64_t ki = rl64(key, i);
            const uint64_t ci = rl64(cand, i);
            if (have && ki == key) {
              mymin = ci < mymin ? ci : mymin;
              if (first == 64) first = i;
            }
          }
          const bool is_first = have && first == lane;
          PT_MARK(2)  // fast: stage read + record prefetch issue + in-register dedupe
          uint32_t slot = 0, id = 0;
          bool existed = false;
          if (is_first) {
            slot = ht_find_or_insert(ar.hkeys, caps.H - 1, key, &existed);
            if (existed) id = ld_l2(&ar.hvals[slot]);
          }
          const bool newf = is_first && !existed;
          const uint64_t nm = __ballot(newf);
          const uint32_t n_new = (uint32_t)__popcll(nm);
          if (hi + n_new > caps.S) {
            res.status = ST_OVERFLOW_STATES;
            ok = false;
            break;
          }
          if (newf) {  // new id = hi + (number of earlier first occurrences)  [state_table.rs:49-59]
            const uint32_t rank = lanes_below(nm);
            id = hi + rank;
            ar.hvals[slot] = id;  // plain store: later readers are this wave (same CU / L2); an sc1 store's ack is slow
            ar.tuples[id] = key;
            if (FLAGS & FLAG_SP) ar.skey[id] = mymin;
            stg.nkey[rank] = key;
            stg.nsk[rank] = mymin;
            stg.nr1[rank] = pr1;
            stg.nr2[rank] = pr2;
          } else if ((FLAGS & FLAG_SP) && is_first && mymin != KEY_INF) {
            atomicMin((unsigned long long*)&ar.skey[id], (unsigned long long)mymin);  // older state: fix-up will iterate
          }
          PT_MARK(3)  // fast: hash CAS + id assignment + stores issue
          const uint32_t id_all = __shfl(id, first & 63u);
          if (have) {
            store_arc(ar.arcs + n_arcs + lane, il, ol, w, id_all);
            if (id_all < hi) needs_fixup = true;  // arc into this or an earlier level
          }
          n_arcs += level_cnt;
          if (lane == 0) ar.off[hi] = n_arcs;
          lds_handoff();
          if (lane < n_new) {
            f_key = stg.nkey[lane];
            f_sk = stg.nsk[lane];
            f_r1 = stg.nr1[lane];
            f_r2 = stg.nr2[lane];
          } else {
            f_key = 0ull;
            f_sk = KEY_INF;
          }
          lds_handoff();
          lo = hi;
          hi += n_new;
          n_states = hi;
          PT_MARK(4)  // fast: arc stores + frontier compaction
        }
        // rc == EXP_FAST_OVERFLOW: more than 64 arcs in this level -> redo it on the general path
      }
      if (did_fast) continue;
      // ---------------- general path: level staged through the arena in HBM/L2
      for (uint32_t q = lo; q < hi; ++q) {
        if (lane == 0) ar.off[q] = n_arcs;
        const uint64_t tk = ar.tuples[q];
        if (expand_state<false>(f1, f2, mode, filter, ar, caps, q, tk, ld_global16(f1.srec + tuple_s1(tk)),
                                ld_global16(f2.srec + (uint32_t)tk), KEY_INF, lv, &n_arcs, nullptr, nullptr, &res.status) != EXP_OK) {
          ok = false;
          break;
        }
      }
      if (!ok) break;
      if (lane == 0) ar.off[hi] = n_arcs;
      wave_sync();
      // rank first occurrences: new id = hi + (number of earlier first occurrences)  [state_table.rs:49-59]
      uint32_t n_new = 0;
      for (uint32_t base = lv.arc_begin; base < n_arcs; base += 64) {
        const uint32_t e = base + lane;
        bool first = false;
        uint32_t slot = 0;
        if (e < n_arcs) {
          slot = ar.arcs[e].nextstate;
          first = ld_l2(&ar.hvals[slot]) == (HV_PEND | (e - lv.arc_begin));
        }
        const uint64_t m = __ballot(first);
        const uint32_t cntm = (uint32_t)__popcll(m);
        if (hi + n_new + cntm > caps.S) {
          res.status = ST_OVERFLOW_STATES;
          ok = false;
          break;
        }
        if (first) {
          const uint32_t id = hi + n_new + lanes_below(m);
          st_l2(&ar.hvals[slot], id);
          ar.tuples[id] = ld_l2(&ar.hkeys[slot]);
        }
        n_new += cntm;
      }
      if (!ok) break;
      wave_sync();
      // patch destinations: slot -> id
      for (uint32_t base = lv.arc_begin; base < n_arcs; base += 64) {
        const uint32_t e = base + lane;
        if (e < n_arcs) {
          const uint32_t id = ld_l2(&ar.hvals[ar.arcs[e].nextstate]);
          ar.arcs[e].nextstate = id;
          if (id < hi) needs_fixup = true;  // arc into this or an earlier level: one forward pass is not enough
        }
      }
      wave_sync();
      if (FLAGS & FLAG_SP) {
        // relax this level's arcs now: on a lattice every predecessor of these states is already final
        relax_states(ar, lo, hi, n_arcs);
        wave_sync();
      }
      if (caps.W && n_new > caps.W) {
        res.status = ST_SWITCH_WIDE;
        ok = false;
        break;
      }
      lo = hi;
      hi += n_new;
      n_states = hi;
      fast = n_new <= 64;
      if (fast) {  // pull the new frontier back into registers
        f_key = lane < n_new ? ar.tuples[lo + lane] : 0ull;
        f_sk = ((FLAGS & FLAG_SP) && lane < n_new) ? ld_l2(&ar.skey[lo + lane]) : KEY_INF;
        if (lane < n_new) {
          f_r1 = ld_global16(f1.srec + tuple_s1(f_key));
          f_r2 = ld_global16(f2.srec + (uint32_t)f_key);
        }
      }
    }
    if (lane == 0) ar.lvl[n_levels] = n_states;
    PT_MARK(5)  // general-path levels
  }
  needs_fixup = __any(needs_fixup);
  res.n_states = n_states;
  res.n_arcs = n_arcs;
  res.n_levels = n_levels;
  res.t_states = n_states;
  res.t_arcs = n_arcs;
  res.t_start = n_states ? 0 : -1;

  // ------------------------------------------------------------ trim: connect() + del_states (stable)
  if ((FLAGS & FLAG_TRIM) && ok && n_states) {
    // every BFS-discovered state is accessible; coaccess = can reach a final state (connect.rs:54-60)
    for (uint32_t i = lane; i < n_states; i += 64) ar.aux[i] = ar.fin[i] != INF ? 1u : 0u;
    wave_sync();
    bool changed = true;
    while (changed) {
      changed = false;
      for (int32_t k = (int32_t)n_levels - 1; k >= 0; --k) {  // reverse level order: one pass on lattices
        const uint32_t llo = ar.lvl[k], lhi = ar.lvl[k + 1];
        for (uint32_t base = llo; base < lhi; base += 64) {
          const uint32_t q = base + lane;
          if (q < lhi && ld_l2(&ar.aux[q]) == 0u) {
            const uint32_t b = ar.off[q], e = ar.off[q + 1];
            for (uint32_t i = b; i < e; ++i) {
              if (ld_l2(&ar.aux[ar.arcs[i].nextstate])) {
                st_l2(&ar.aux[q], 1u);
                changed = true;
                break;
              }
            }
          }
        }
        wave_sync();
      }
      changed = __any(changed);
    }
    // new ids = rank among survivors (mutable_fst.rs:139-149)
    uint32_t kept = 0;
    for (uint32_t base = 0; base < n_states; base += 64) {
      const uint32_t q = base + lane;
      const bool keep = q < n_states && ld_l2(&ar.aux[q]) != 0u;
      const uint64_t m = __ballot(keep);
      if (q < n_states) ar.aux2[q] = keep ? kept + lanes_below(m) : FILTER_REJECT;
      kept += (uint32_t)__popcll(m);
    }
    wave_sync();
    // surviving arcs, order preserved, retargeted (mutable_fst.rs:153-176)
    uint32_t t_arcs = 0;
    for (uint32_t base = 0; base < n_states; base += 64) {
      const uint32_t q = base + lane;
      const bool keep = q < n_states && ar.aux2[q] != FILTER_REJECT;
      uint32_t b = 0, e = 0, cnt = 0;
      if (keep) {
        b = ar.off[q];
        e = ar.off[q + 1];
        for (uint32_t i = b; i < e; ++i) cnt += ar.aux2[ar.arcs[i].nextstate] != FILTER_REJECT;
      }
      uint32_t total;
      const uint32_t pos = wave_excl_scan(cnt, lane, &total);
      if (keep) {
        const uint32_t nq = ar.aux2[q];
        uint32_t w = t_arcs + pos;
        ar.t_off[nq] = w;
        ar.t_fin[nq] = ar.fin[q];
        for (uint32_t i = b; i < e; ++i) {
          const ArcReg a = load_arc<GlobalLoad>(ar.arcs + i);
          const uint32_t nn = ar.aux2[a.ns];
          if (nn != FILTER_REJECT) store_arc(ar.t_arcs + (w++), a.il, a.ol, a.w, nn);
        }
      }
      t_arcs += total;
    }
    if (lane == 0) ar.t_off[kept] = t_arcs;
    res.t_states = kept;
    res.t_arcs = t_arcs;
    res.t_start = (kept && ar.aux2[0] != FILTER_REJECT) ? (int32_t)ar.aux2[0] : -1;
    wave_sync();
  }

  // ------------------------------------------------------------ fused n=1 shortest path on the composed FST
  // (run on the untrimmed composition: dead states cannot lie on a successful path, and the canonical tie
  //  rule is invariant under the stable renumbering of trim, so the result equals shortest_path(connect(C)))
  if ((FLAGS & FLAG_SP) && ok && n_states) {
    if (needs_fixup) {  // cyclic / non-layered composition: iterate to the fixed point
      for (uint32_t it = 0; it <= n_states; ++it) {
        wave_sync();
        if (!relax_states(ar, 0, n_states, n_arcs)) break;
      }
    }
    wave_sync();
    // f_parent = argmin (d (x) rho, id)      shortest_path.rs:214-220
    unsigned long long best = KEY_INF;
    for (uint32_t base = 0; base < n_states; base += 64) {
      const uint32_t q = base + lane;
      if (q < n_states) {
        const uint64_t kq = ld_l2(&ar.skey[q]);
        const float f = ar.fin[q];
        if (kq != KEY_INF && f < INF) {
          const float tot = (key_f32((uint32_t)(kq >> 32)) + f) + 0.0f;
          if (tot < INF) {
            const unsigned long long c = ((unsigned long long)f32_key(tot) << 32) | q;
            best = c < best ? c : best;
          }
        }
      }
    }
    best = wave_min_u64(best);
    if (best != KEY_INF) {
      const uint32_t fp = (uint32_t)best;
      const uint32_t hops = (uint32_t)ld_l2(&ar.skey[fp]);
      res.has_path = 1;
      res.hops = hops;
      res.final_weight = ar.fin[fp];
      res.total = key_f32((uint32_t)(best >> 32));
      // parent[t] = min (s,pos) among layered tight arcs
      for (uint32_t i = lane; i < n_states; i += 64) ar.parent[i] = KEY_INF;
      wave_sync();
      for (uint32_t base = 0; base < n_states; base += 64) {
        const uint32_t q = base + lane;
        if (q < n_states) {
          const uint64_t kq = ld_l2(&ar.skey[q]);
          if (kq != KEY_INF) {
            const float d = key_f32((uint32_t)(kq >> 32));
            const uint32_t h1 = (uint32_t)kq + 1u;
            const uint32_t b = ar.off[q], e = ar.off[q + 1];
            for (uint32_t i = b; i < e; ++i) {
              const ArcReg a = load_arc<GlobalLoad>(ar.arcs + i);
              const float c = (d + a.w) + 0.0f;
              if (!(c < INF)) continue;
              const uint64_t ck = ((uint64_t)f32_key(c) << 32) | h1, kt = ld_l2(&ar.skey[a.ns]);
              // class 0: tight in distance and hop count; class 1 (top bit): tight in the distance only, from a state
              // with a smaller key (sssp.hip parent_class)
              if (ck == kt)
                atomicMin((unsigned long long*)&ar.parent[a.ns], ((unsigned long long)q << 32) | (i - b));
              else if ((ck >> 32) == (kt >> 32) && kq < kt)
                atomicMin((unsigned long long*)&ar.parent[a.ns], (1ull << 63) | ((unsigned long long)q << 32) | (i - b));
            }
          }
        }
      }
      wave_sync();
      // mark the ancestors of f_parent by pointer doubling: aux = mark, jump pointers ping-pong
      // between aux2 and lvl (dead after trim)
      uint32_t* ja = ar.aux2;
      uint32_t* jb = ar.lvl;
      for (uint32_t i = lane; i < n_states; i += 64) {
        const uint64_t pr = ld_l2(&ar.parent[i]);
        ja[i] = pr == KEY_INF ? i : ((uint32_t)(pr >> 32) & 0x7FFFFFFFu);
        ar.aux[i] = i == fp ? 1u : 0u;
      }
      wave_sync();
      for (uint32_t span = 1; span <= hops; span <<= 1) {
        // mark[jump[t]] |= mark[t]; jump'[t] = jump[jump[t]]
        for (uint32_t i = lane; i < n_states; i += 64) {
          const uint32_t j = ja[i];
          if (ld_l2(&ar.aux[i])) st_l2(&ar.aux[j], 1u);
          jb[i] = ja[j];
        }
        wave_sync();
        uint32_t* tmp = ja;
        ja = jb;
        jb = tmp;
      }
      // reserve the slice of the packed path buffer and write the arcs (shortest_path.rs:257-272)
      uint32_t poff = 0;
      if (lane == 0) poff = atomicAdd(path_cursor, hops);
      poff = __shfl(poff, 0);
      // a marked state without a class-0 predecessor: positions cannot be read off the hop counts
      bool tie = false;
      for (uint32_t i = lane; i < n_states; i += 64)
        if (ld_l2(&ar.aux[i]) && (uint32_t)ld_l2(&ar.skey[i]) >= 1u && (ld_l2(&ar.parent[i]) >> 63)) tie = true;
      if (__any(tie)) {
        res.status = ST_TIE_ORDER;
      } else if ((uint64_t)poff + hops > path_cap) {
        res.status = ST_OVERFLOW_PATH;
      } else {
        res.path_off = poff;
        for (uint32_t i = lane; i < n_states; i += 64) {
          if (ld_l2(&ar.aux[i])) {
            const uint64_t ki = ld_l2(&ar.skey[i]);
            const uint32_t hi_ = (uint32_t)ki;
            if (hi_ >= 1u) {
              const uint64_t pr = ld_l2(&ar.parent[i]);
              const uint32_t s = (uint32_t)(pr >> 32), pos = (uint32_t)pr;
              const ArcReg a = load_arc<GlobalLoad>(ar.arcs + ar.off[s] + pos);
              const uint32_t k = hops - hi_;  // i is the k-th state created by the backtrace
              store_arc(path_buf + poff + k, a.il, a.ol, a.w, k);
            }
          }
        }
      }
    }
  }
  PT_MARK(6)  // trim / shortest-path epilogue
  PT_STORE(res)
}

template <uint32_t FLAGS>
__global__ void __launch_bounds__(64) compose_wave_kernel(const ProblemDesc* __restrict__ descs, FstView f2, Caps caps,
                                                          char* __restrict__ arena_base, size_t arena_stride,
                                                          Result* __restrict__ results, wfst_tr* __restrict__ path_buf,
                                                          uint32_t path_cap, uint32_t* __restrict__ path_cursor) {
  const uint32_t p = blockIdx.x;
  const ProblemDesc desc = descs[p];
  const Arena ar = carve_arena(arena_base + (size_t)p * arena_stride, caps);
  Result res;
  compose_wave_problem<FLAGS>(desc.f1, f2, desc.mode, desc.filter, caps, ar, res, path_buf, path_cap, path_cursor);
  if (lane_id() == 0) results[p] = res;
}

// wfst_compose_batch: one wavefront per item, every item with its own second operand, capacities and arena (carved on
// the host from the launch's slab: a 20-state item beside a 4 000-state item pays for 20 states; skey and parent, which
// only the fused shortest path uses, are not part of it).  The width hand-over is off (caps.W == 0): include/wfst.h.
struct ComposeBatchCtl {  // one per item, at the head of the slab; read back once
  uint32_t status;            // ST_*
  uint32_t n_states, n_arcs;  // pre-trim
  uint32_t t_states, t_arcs;  // after trim (== pre-trim when not trimming)
  int32_t t_start;
  uint32_t done;  // 1: the wave wrote this block (the host zeroes the blocks before the launch)
  uint32_t pad;
};
struct ComposeBatchItem {
  FstView f1, f2;
  uint32_t mode, filter;
  Caps caps;
  Arena ar;
  ComposeBatchCtl* ctl;
};

template <uint32_t FLAGS>
__global__ void __launch_bounds__(64) compose_batch_kernel(const ComposeBatchItem* __restrict__ items) {
  static_assert((FLAGS & FLAG_SP) == 0, "the arenas of a list have no shortest-path arrays");
  const ComposeBatchItem it = items[blockIdx.x];
  Result res;
  compose_wave_problem<FLAGS>(it.f1, it.f2, it.mode, it.filter, it.caps, it.ar, res, nullptr, 0u, nullptr);
  if (lane_id() == 0) {
    ComposeBatchCtl c;
    c.status = res.status;
    c.n_states = res.n_states;
    c.n_arcs = res.n_arcs;
    c.t_states = res.t_states;
    c.t_arcs = res.t_arcs;
    c.t_start = res.t_start;
    c.done = 1u;
    c.pad = 0u;
    *it.ctl = c;
  }
}


// ------------------------------------------------------------------------------------------------------------------
// string o T  ->  shortest path, one wave per problem: the decoding case of the fused batch, where fst1 is a linear,
// epsilon-free, single-final acceptor (utils::acceptor, labels_to_fst.rs:111-132) and fst2 has no input-epsilon arcs.
// The composition is then a layered lattice — BFS level i = the composed states (i, q) — so the general machinery above
// collapses:
//   * a tuple first seen in level i + 1 cannot have been seen before: first-occurrence ranking inside the level (ballots over
//     the new states, which live in lane registers) IS StateTable::find_id; no hash table, no CAS round trip;
//   * ids are handed out level by level in emission order, arcs of a state in fst2's arc order (the label-equal run of a
//     sorted block): the numbering LazyFst::compute produces (lazy/lazy_fst.rs:226-269), hence the same canonical parent
//     (smallest (source id, arc position) among the tight arcs == the first strict improvement in emission order);
//   * every arc goes from level i to level i + 1: one forward pass is the exact (min,+) fixed point, hops == level;
//   * the arc block of a destination is named by the matched arc itself (FstView::anext), so a level costs ONE dependent
//     trip to memory (the arc blocks of the frontier) instead of three (state record -> arc block -> hash).
// Composed states / arcs are only counted (the fused batch returns paths); parents live in LDS.  Anything outside the
// covered case (more than 64 states in a level, more than STR_MAXS states in all) reports ST_NOT_A_STRING_CASE and the
// host re-runs that problem on compose_wave_kernel.  Results are bit-identical to the general kernel's by construction and
// by test (tests/test_gpu_parity.py: both kernels against the oracle).
constexpr uint64_t WIDE_COMPOSE_STATES = 16384;  // compose(): results beyond this go to compose_wide.hip
constexpr uint32_t WIDE_COMPOSE_WIDTH = 64;      // ... and so do results with a BFS level wider than this (one wave's worth)
constexpr uint32_t STR_MAXS = 2048;
constexpr uint32_t STR_NONE = 0xFFFFFFFFu;

// One wave = one problem; a workgroup holds blockDim.x / 64 of them, each with its own `maxs`-state slice of the dynamic
// LDS (the waves never meet: no workgroup barrier anywhere).  How many waves share a workgroup is the host's choice
// (string_placement.h) and changes nothing but where they sit.  Spread — a workgroup per compute unit, a wave per SIMD, for as
// long as the context has them — a level's dependent load and its ~26-instruction chain wait for nobody (profiles/
// string_placement_ab.md).  Packed — what 64 KB of LDS hold, eight waves at the 512-state slice — while a resident
// relaxation grid is at work on the device: a resident wave of this kernel blocks its whole CU for that grid's 1024-thread,
// 128-VGPR workgroups (they need every register of all four SIMDs), the grid needs ~245 whole CUs at once, and 8 workgroups of 8
// waves land on one CU per XCD and leave it 31 of 32.
__global__ void __launch_bounds__(512) string_compose_sp_kernel(const ProblemDesc* __restrict__ descs, FstView f2,
                                                                Result* __restrict__ results, wfst_tr* __restrict__ path_buf,
                                                                uint32_t path_cap, uint32_t n_problems, uint32_t maxs, uint64_t f2_n_arcs,
                                                                uint32_t scalar_rows, uint32_t run_on, uint32_t pair_on,
                                                                uint32_t done_ticket) {
  extern __shared__ uint32_t s_dyn[];
  const uint32_t p = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (p >= n_problems) return;
  uint32_t* const s_par = s_dyn + (size_t)(threadIdx.x >> 6) * 4u * maxs;  // predecessor state on the best path into this state (STR_NONE: unreached)
  uint32_t* const s_ol = s_par + maxs;                                      // olabel of the arc taken from it
  float* const s_w = reinterpret_cast<float*>(s_ol + maxs);                 // weight of that arc (w1 (x) w2)
  uint32_t* const s_pth = s_ol + 2u * maxs;                                 // states of the best path, from the final one backwards
  const uint32_t lane = lane_id();
  // the problem's result, then (everything this wave wrote is in host memory) its ticket
#define STR_RESULT() do {                                                                                  \
    PT_STORE(res)                                                                                          \
    res.done = 0u;                                                                                         \
    if (lane == 0) results[p] = res;                                                                       \
    if (done_ticket != 0u) { /* (0: a large batch — the host waits for the stream, see launch_begin) */     \
      __threadfence_system(); /* (the stores' acknowledgements alone are not enough: measured) */             \
      if (lane == 0) __hip_atomic_store(&results[p].done, done_ticket, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); \
    }                                                                                                      \
  } while (0)
  const FstView f1 = descs[p].f1;
  const uint32_t poff = descs[p].path_off;  // this problem's slice of the path buffer (launch_begin); read with the descriptor:
                                            // it may live in host memory
  Result res;
  res.status = ST_OK;
  res.n_states = res.n_arcs = res.t_states = res.t_arcs = 0;
  res.t_start = -1;
  res.has_path = res.hops = 0;
  res.final_weight = res.total = INF;
  res.path_off = 0;
  res.n_levels = 0;
  res.facts = props::PATH_FACTS_NONE;
  res.run_levels = res.runs = res.pair_levels = res.pair_splits = 0;
  PT_DECL
  if (f1.start < 0 || f2.start < 0) {  // compute_start -> None
    STR_RESULT();
    return;
  }
  const uint32_t L = f1.n_states - 1u;  // number of arcs of the string
  // frontier of the current level in registers: lane k < F holds composed state lo + k = (pos, q)
  uint32_t q = 0, nb = 0, nc = 0;
  float d = INF;
  if (lane == 0) {
    q = (uint32_t)f2.start;
    d = 0.0f;  // Weight::one()
    const uint4 r = ld_global16(f2.srec + q);
    nb = r.x;
    nc = r.y;
  }
  uint32_t lo = 0, hi = 1, F = 1, n_arcs = 0, level = 0;  // level = position of the current frontier in the string
  if (lane == 0) s_par[0] = STR_NONE;
  // the string's arcs, 64 at a time, one per lane (a linear acceptor: arc i leaves state i), the next 64 already on their
  // way: a label is a v_readlane away.  (One broadcast load per level, asked for one level ahead, made every level wait
  // for a vector load — ~0.6 us for a lone wave — however fast the arc block of fst2 came in.)
  uint4 ch_cur = make_uint4(0, 0, 0, 0), ch_nxt = make_uint4(0, 0, 0, 0);
  if (lane < L) ch_cur = ld_global16(f1.arcs + lane);
  if (64u + lane < L) ch_nxt = ld_global16(f1.arcs + 64u + lane);
  bool ok = true;
  // Early issue (vector path): a level of ONE state whose block fits one chunk and matches ONE arc knows the next level's
  // block — the matched arc's destination range — two instructions after the ballot.  Its rows are asked for there, into
  // (pf_a, pf_nx), and the level's bookkeeping (on_match, the loop tail, the next label) runs under that load instead of
  // in front of it; the next level takes the pair when pf is set.  The rows are immutable: a pair that goes unused
  // (ok = false, the end of the string) is dropped.
  bool pf = false;
  const uint32_t L_u = rl(L, 0);  // (L in a scalar register: the early-issue decision stays a scalar branch)
  uint4 pf_a = make_uint4(0, 0, 0, 0);
  uint2 pf_nx = make_uint2(0, 0);
  // The chase run (vector path, run_on): while the frontier is ONE state whose block fits one chunk and ONE arc of it carries
  // the label, the only dependence from level to level is rows -> the matched lane -> that arc's anext pair -> the next rows.
  // A run level puts that and nothing else between the rows' arrival and the next rows' issue: the matched arc's fields are
  // read off its lane first, so the next rows land in the registers the level reads them from (no copy behind a wait; lanes
  // that do not load keep what they held: every reader masks with lane < fc).  The level's one new state (consecutive ids,
  // one per level) is settled under that load, by on_match's own arithmetic in level order.  The string's 64-label chunks
  // are rotated between the segments of a run, not inside the level.  A level that is not such a one (no match, several
  // matches, a longer block, the string's last level, the last state of the slice) ends the run with `pos` on it and is
  // done by the general level below, from the rows the run already holds (pf) where it has them.
  // Pair levels (pair_on, vector rows): the run's loop also carries a frontier of TWO states.  A level whose frontier has one
  // or two states (each block within one chunk) and whose matches, taken in (frontier state, arc position) order, are one or
  // two with distinct destinations makes exactly those states, in that order: no destination is met twice, so there is no
  // find_id hit and no second way in, and on_match would give match j the id hi + j, the parent lo + f and the value
  // (d_f + ws) + 0 — which is what the pair level writes, asking for the rows of both new states first and settling under
  // that load.  Everything else (no match, three matches or more, two matches into one state — dedup and the strict tie
  // rule stay on_match's —, a longer block, the last level, hi + t reaching the slice) ends the run as before; a frontier of
  // two goes to the general level without rows (it asks for both blocks at once), a frontier of one with its rows.
  PT_MARK(6)  // prologue
  for (uint32_t pos = 0; pos < L && F && ok; ++pos) {
    if (pos && (pos & 63u) == 0u) {
      ch_cur = ch_nxt;
      ch_nxt = make_uint4(0, 0, 0, 0);
      if (pos + 64u + lane < L) ch_nxt = ld_global16(f1.arcs + pos + 64u + lane);
    }
    if (run_on && F == 1u && (!scalar_rows || run_on == 2u)) {
      uint32_t fb = rl(nb, 0), fc = rl(nc, 0);
      if (fc <= 64u && pos + 1u < L_u && hi + 1u < maxs) {
        const uint32_t p0 = pos;
        // the rows of the level in (a, nx): lanes < fc hold them, the other lanes hold whatever they held (every reader masks)
        uint4 a = pf_a;
        uint2 nx = pf_nx;
        if (!pf && lane < fc) {
          a = ld_global16(f2.arcs + fb + lane);
          nx = *reinterpret_cast<const uint2*>(reinterpret_cast<const char*>(f2.anext) + 8ull * (fb + lane));
        }
        pf = false;
        float dd = __uint_as_float(rl(__float_as_uint(d), 0));  // the distance of the run's last state (uniform)
        // `lane < fc` as a scalar mask, made under the load: the compare's own mask is then the ballot (the predicate as a lane
        // value costs the chain two dependent vector instructions more)
        uint64_t fcm = fc >= 64u ? ~0ull : (1ull << fc) - 1ull;
        // the second state of a carried frontier (`two`): its rows in (b, bx), its block and its distance; state 0's are
        // (a, nx), fb / fc and dd
        uint4 b = make_uint4(0, 0, 0, 0);
        uint2 bx = make_uint2(0, 0);
        uint32_t fb1 = 0, fc1 = 0;
        float dd1 = INF;
        bool two = false;
        const bool pairs = pair_on != 0u && !scalar_rows;
        uint32_t n_run = 0, n_runs = 0, n_pair = 0, n_split = 0;
        bool in_run = false;  // the last level taken was a run level: the counter's runs are maximal sequences of those
        PT_MARK(5)
        for (bool go = true; go;) {  // one pass = the run's levels inside one 64-label chunk of the string
          bool on_boundary = false;  // the last level taken moved pos onto the next chunk
          bool split = false;        // the run levels stopped on a level of two matches: the pair level below looks at it
          const uint32_t s0 = pos;
          if (!two) for (;;) {
            const uint32_t label = rl(ch_cur.x, pos & 63u);
            const float w1 = __uint_as_float(rl(ch_cur.z, pos & 63u));
            PT_MARK(3)  // run: the last level's settle and counters, under the load
            PT_ROWS_IN()
            PT_MARK(4)  // run: waiting for the rows
            // ---- on the chain: rows -> ballot -> the matched lane's fields -> the next rows
            const uint64_t m = __ballot(a.x == label) & fcm;
            if (m == 0ull || (m & (m - 1ull)) != 0ull) {  // the general level's: lanes < fc hold its rows
              pf = true;
              go = false;
              break;
            }
            const uint32_t l = (uint32_t)__ffsll((unsigned long long)m) - 1u;
            const uint32_t xb = rl(nx.x, l), xc = rl(nx.y, l);
            const uint32_t ol = rl(a.y, l), w2u = rl(a.z, l);  // (a.w, the destination, is the general level's to name: it
                                                               // ends every run and sets q from its own matches)
            if (lane < xc && xc <= 64u) {  // (everything of the old rows is read off: the new ones land in their place)
              a = ld_global16(f2.arcs + xb + lane);
              nx = *reinterpret_cast<const uint2*>(reinterpret_cast<const char*>(f2.anext) + 8ull * (xb + lane));
            }
            PT_MARK(5)  // run: from the rows' arrival to the next rows' issue
            // ---- under the load: state hi = (pos + 1, a.w) is settled as on_match settles the one new state of a level (F == 1:
            // its only way in is from state hi - 1)
            const float ws = wtimes(w1, __uint_as_float(w2u));  // add_tr, compose_fst_op.rs:267-285
            float c = INF;
            if (dd < INF) c = (dd + ws) + 0.0f;
            const bool reached = c < INF;
            if (lane == 0) {
              s_ol[hi] = ol;
              s_w[hi] = ws;
              s_par[hi] = reached ? hi - 1u : STR_NONE;
            }
            dd = reached ? c : INF;
            fb = xb;
            fc = xc;
            fcm = fc >= 64u ? ~0ull : (1ull << fc) - 1ull;
            n_arcs += 1;
            hi += 1;
            pos += 1;
            on_boundary = (pos & 63u) == 0u;
            if (fc > 64u) {  // a longer block: the general level loads it chunk by chunk
              go = false;
              break;
            }
            if (!(pos + 1u < L_u && hi + 1u < maxs)) {  // the general level's, with these rows
              pf = true;
              go = false;
              break;
            }
            if (on_boundary) break;
          }
          if (pos != s0) {
            n_run += pos - s0;
            n_runs += in_run ? 0u : 1u;
            in_run = true;
          }
          // (the run level's loop is left as it was: whether the level it stopped on, rows in hand, has two matches is asked here)
          if (pairs && !two && pf && pos + 1u < L_u && hi + 2u < maxs &&
              __popcll(__ballot(a.x == rl(ch_cur.x, pos & 63u)) & fcm) == 2) {
            split = true;
            pf = false;
            go = true;
          }
          // ---- pair levels: a frontier of two states, or the level of two matches the run levels stopped on.  One trip to
          // memory per level like a run level, off the run level's chain
          if (go && (two || split)) for (;;) {
            const uint32_t label = rl(ch_cur.x, pos & 63u);
            const float w1 = __uint_as_float(rl(ch_cur.z, pos & 63u));
            PT_MARK(3)
            PT_ROWS_IN()
            PT_MARK(4)
            const uint64_t m0 = __ballot(a.x == label) & fcm;
            const uint64_t m1 = two ? __ballot(b.x == label) & (fc1 >= 64u ? ~0ull : (1ull << fc1) - 1ull) : 0ull;
            const uint32_t c0 = (uint32_t)__popcll(m0), t = c0 + (uint32_t)__popcll(m1);
            if (t == 0u || t > 2u || hi + t >= maxs) {  // the general level's (one state: with its rows)
              pf = !two;
              go = false;
              break;
            }
            // match j, in (frontier state, arc position) order, sits in lane lj of state 0's rows, or (from_b) of state 1's
            const bool from_b0 = c0 == 0u, from_b1 = c0 < 2u;
            const uint32_t l0 = (uint32_t)__ffsll((unsigned long long)(from_b0 ? m1 : m0)) - 1u;
            const uint64_t rest = c0 == 1u ? m1 : (from_b1 ? m1 & (m1 - 1ull) : m0 & (m0 - 1ull));
            const uint32_t l1 = t == 2u ? (uint32_t)__ffsll((unsigned long long)rest) - 1u : 0u;
            auto field = [&](bool from_b, uint32_t va, uint32_t vb, uint32_t l) -> uint32_t { return from_b ? rl(vb, l) : rl(va, l); };
            const uint32_t xb0 = field(from_b0, nx.x, bx.x, l0), xc0 = field(from_b0, nx.y, bx.y, l0);
            const uint32_t ol0 = field(from_b0, a.y, b.y, l0), w2u0 = field(from_b0, a.z, b.z, l0);
            uint32_t xb1 = 0, xc1 = 0, ol1 = 0, w2u1 = 0;
            if (t == 2u) {
              if (field(from_b0, a.w, b.w, l0) == field(from_b1, a.w, b.w, l1)) {  // one destination by two ways: on_match's
                pf = !two;
                go = false;
                break;
              }
              xb1 = field(from_b1, nx.x, bx.x, l1);
              xc1 = field(from_b1, nx.y, bx.y, l1);
              ol1 = field(from_b1, a.y, b.y, l1);
              w2u1 = field(from_b1, a.z, b.z, l1);
            }
            if (lane < xc0 && xc0 <= 64u) {  // (everything of the old rows is read off)
              a = ld_global16(f2.arcs + xb0 + lane);
              nx = *reinterpret_cast<const uint2*>(reinterpret_cast<const char*>(f2.anext) + 8ull * (xb0 + lane));
            }
            if (t == 2u && lane < xc1 && xc1 <= 64u) {
              b = ld_global16(f2.arcs + xb1 + lane);
              bx = *reinterpret_cast<const uint2*>(reinterpret_cast<const char*>(f2.anext) + 8ull * (xb1 + lane));
            }
            PT_MARK(5)
            // ---- under the load: states hi and (t == 2) hi + 1, each with one way in
            const uint32_t lo_r = hi - (two ? 2u : 1u);
            const float d0 = from_b0 ? dd1 : dd, d1 = from_b1 ? dd1 : dd;
            const float ws0 = wtimes(w1, __uint_as_float(w2u0));  // add_tr, compose_fst_op.rs:267-285
            float cand0 = INF, cand1 = INF, ws1 = 0.0f;
            if (d0 < INF) cand0 = (d0 + ws0) + 0.0f;
            const bool reached0 = cand0 < INF;
            bool reached1 = false;
            if (t == 2u) {
              ws1 = wtimes(w1, __uint_as_float(w2u1));
              if (d1 < INF) cand1 = (d1 + ws1) + 0.0f;
              reached1 = cand1 < INF;
            }
            if (lane == 0) {
              s_ol[hi] = ol0;
              s_w[hi] = ws0;
              s_par[hi] = reached0 ? lo_r + (from_b0 ? 1u : 0u) : STR_NONE;
              if (t == 2u) {
                s_ol[hi + 1u] = ol1;
                s_w[hi + 1u] = ws1;
                s_par[hi + 1u] = reached1 ? lo_r + (from_b1 ? 1u : 0u) : STR_NONE;
              }
            }
            dd = reached0 ? cand0 : INF;
            dd1 = reached1 ? cand1 : INF;
            fb = xb0;
            fc = xc0;
            fcm = fc >= 64u ? ~0ull : (1ull << fc) - 1ull;
            fb1 = xb1;
            fc1 = xc1;
            two = t == 2u;
            n_arcs += t;
            hi += t;
            pos += 1;
            n_pair += 1u;
            n_split += two ? 1u : 0u;
            in_run = false;
            on_boundary = (pos & 63u) == 0u;
            if (fc > 64u || fc1 > 64u) {  // a longer block: the general level loads it chunk by chunk
              go = false;
              break;
            }
            if (!(pos + 1u < L_u && hi + 1u < maxs)) {  // the general level's
              pf = !two;
              go = false;
              break;
            }
            if (on_boundary || !two) break;
          }
          if (on_boundary) {  // the next 64 labels of the string (the loop's head does this only where no run moved pos there)
            ch_cur = ch_nxt;
            ch_nxt = make_uint4(0, 0, 0, 0);
            if (pos + 64u + lane < L) ch_nxt = ld_global16(f1.arcs + pos + 64u + lane);
          }
        }
        if (pf) {
          pf_a = a;
          pf_nx = nx;
        }
        if (pos != p0) {
          if (lane == 0) {
            nb = fb;
            nc = fc;
            d = dd;
          }
          if (two && lane == 1) {
            nb = fb1;
            nc = fc1;
            d = dd1;
          }
          F = two ? 2u : 1u;
          lo = hi - F;
          level = pos;
          res.run_levels += n_run;
          res.runs += n_runs;
          res.pair_levels += n_pair;
          res.pair_splits += n_split;
        }
        PT_MARK(3)
      }
    }
    const bool use_pf = pf;  // set by the last level: this level is one state, and lanes < min(its arc count, 64) hold its rows
    pf = false;
    const uint32_t pl = pos & 63u;
    const uint32_t label = rl(ch_cur.x, pl);
    const float w1 = __uint_as_float(rl(ch_cur.z, pl));
    uint32_t nq = 0, nnb = 0, nnc = 0, n_new = 0;  // new states of the next level: lane k holds state hi + k
    float nd = INF;
    // one matched arc (f -> qd, output label ol, weight w2, the destination's arc block [xb, xb + xc)): the destination
    // becomes a state of the next level unless the level has it already, and keeps the better way in
    auto on_match = [&](uint32_t f, float fd, uint32_t qd, uint32_t ol, uint32_t xb, uint32_t xc, float w2) -> bool {
      const float wsum = wtimes(w1, w2);  // add_tr, compose_fst_op.rs:267-285
      float c = INF;
      if (fd < INF) c = (fd + wsum) + 0.0f;  // candidate distance; +inf never relaxes (shortest_path.rs:226)
      const uint64_t ex = __ballot(lane < n_new && nq == qd);  // StateTable::find_id inside the level
      uint32_t idx;
      if (ex == 0) {
        idx = n_new;
        if (idx >= 64u || hi + idx >= maxs) return false;
        if (lane == idx) {
          nq = qd;
          nnb = xb;
          nnc = xc;
          nd = INF;
        }
        if (lane == 0) s_par[hi + idx] = STR_NONE;
        n_new += 1;
      } else {
        idx = (uint32_t)__ffsll((unsigned long long)ex) - 1u;
      }
      const float cur = __uint_as_float(rl(__float_as_uint(nd), idx));
      if (c < cur) {  // strict: on ties the earlier (source id, arc position) stays
        if (lane == idx) nd = c;
        if (lane == 0) {
          s_par[hi + idx] = lo + f;
          s_ol[hi + idx] = ol;
          s_w[hi + idx] = wsum;
        }
      }
      return true;
    };
    // The common level: ONE frontier state with a short arc block.  A lone wave's vector load takes ~0.6 us from issue to
    // use on this chip, a scalar load of the same (immutable) rows ~0.1 us (tools/ubench_chase.hip): the labels of a block
    // of up to 12 arcs come through the scalar cache (the loads also bring every line of the block and of its
    // destination ranges in), they are compared on the scalar unit, the matched arc is a scalar-cache hit, and the next
    // level's block address never leaves SGPRs.
    bool took_scalar = false;
    if (scalar_rows && F == 1u) {
      const uint32_t fb = rl(nb, 0), fc = rl(nc, 0);
      if (fc <= 12u && (uint64_t)fb + 12u <= f2_n_arcs) {
        took_scalar = true;
        const float fd = __uint_as_float(rl(__float_as_uint(d), 0));
        // step 1: the twelve labels (one dword per arc: every 64-byte line of the block is touched) and one word of every line
        // of the destination-range block, all issued together: one miss latency
        uint32_t l0, l1, l2, l3, l4, l5, l6, l7, l8, l9, l10, l11, t0, t1, t2;
        const wfst_tr* ap = f2.arcs + fb;
        const uint2* np = f2.anext + fb;
        asm volatile(
            "s_load_dword %0, %15, 0x0\n\ts_load_dword %1, %15, 0x10\n\ts_load_dword %2, %15, 0x20\n\ts_load_dword %3, %15, 0x30\n\t"
            "s_load_dword %4, %15, 0x40\n\ts_load_dword %5, %15, 0x50\n\ts_load_dword %6, %15, 0x60\n\ts_load_dword %7, %15, 0x70\n\t"
            "s_load_dword %8, %15, 0x80\n\ts_load_dword %9, %15, 0x90\n\ts_load_dword %10, %15, 0xa0\n\ts_load_dword %11, %15, 0xb0\n\t"
            "s_load_dword %12, %16, 0x0\n\ts_load_dword %13, %16, 0x2c\n\ts_load_dword %14, %16, 0x58\n\ts_waitcnt lgkmcnt(0)"
            : "=&s"(l0), "=&s"(l1), "=&s"(l2), "=&s"(l3), "=&s"(l4), "=&s"(l5), "=&s"(l6), "=&s"(l7), "=&s"(l8), "=&s"(l9), "=&s"(l10),
              "=&s"(l11), "=&s"(t0), "=&s"(t1), "=&s"(t2)
            : "s"(ap), "s"(np)
            : "memory");
        uint32_t m = 0;  // arcs of the block that carry the label, in arc order
        m |= (l0 == label ? 1u : 0u) | (l1 == label ? 2u : 0u) | (l2 == label ? 4u : 0u) | (l3 == label ? 8u : 0u);
        m |= (l4 == label ? 16u : 0u) | (l5 == label ? 32u : 0u) | (l6 == label ? 64u : 0u) | (l7 == label ? 128u : 0u);
        m |= (l8 == label ? 256u : 0u) | (l9 == label ? 512u : 0u) | (l10 == label ? 1024u : 0u) | (l11 == label ? 2048u : 0u);
        m &= (1u << fc) - 1u;
        n_arcs += (uint32_t)__popc(m);
        while (m) {
          const uint32_t k = (uint32_t)__ffs((int)m) - 1u;
          m &= m - 1u;
          // step 2: the matched arc and its destination's range: both lines are in the scalar cache now
          typedef uint32_t sv4 __attribute__((ext_vector_type(4)));
          typedef uint32_t sv2 __attribute__((ext_vector_type(2)));
          sv4 a;
          sv2 nx;
          const uint32_t o16 = k * 16u, o8 = k * 8u;
          asm volatile("s_load_dwordx4 %0, %2, %4\n\ts_load_dwordx2 %1, %3, %5\n\ts_waitcnt lgkmcnt(0)"
                       : "=&s"(a), "=&s"(nx)
                       : "s"(ap), "s"(np), "s"(o16), "s"(o8)
                       : "memory");
          if (!on_match(0u, fd, a[3], a[1], nx[0], nx[1], __uint_as_float(a[2]))) {
            ok = false;
            break;
          }
        }
      }
    }
    // A narrow level: two to four frontier states, every block within one chunk.  The rows of all of them are asked for at
    // once and taken in the loop's order, state by state and arc by arc: one trip to memory where the loop below pays one
    // per state.
    bool took_together = false;
    if (!took_scalar && ok && F >= 2u && F <= 4u && __ballot(lane < F && nc > 64u) == 0ull) {
      took_together = true;
      PT_MARK(2)
      uint4 ta[4];
      uint2 tn[4];
#pragma unroll
      for (uint32_t f = 0; f < 4u; ++f) {
        ta[f] = make_uint4(0, 0, 0, 0);
        tn[f] = make_uint2(0, 0);
        if (f < F) {
          const uint32_t fb = rl(nb, f), fc = rl(nc, f);
          if (lane < fc) {
            ta[f] = ld_global16(f2.arcs + fb + lane);
            tn[f] = *reinterpret_cast<const uint2*>(reinterpret_cast<const char*>(f2.anext) + 8ull * (fb + lane));
          }
        }
      }
      PT_MARK(2)
      PT_ROWS_IN()
      PT_MARK(0)
#pragma unroll
      for (uint32_t f = 0; f < 4u; ++f) {
        if (f < F && ok) {
          const uint32_t fc = rl(nc, f);
          const float fd = __uint_as_float(rl(__float_as_uint(d), f));
          uint64_t m = __ballot(lane < fc && ta[f].x == label);
          n_arcs += (uint32_t)__popcll(m);
          while (m) {
            const uint32_t l = (uint32_t)__ffsll((unsigned long long)m) - 1u;
            m &= m - 1;
            if (!on_match(f, fd, rl(ta[f].w, l), rl(ta[f].y, l), rl(tn[f].x, l), rl(tn[f].y, l), __uint_as_float(rl(ta[f].z, l)))) {
              ok = false;
              break;
            }
          }
        }
      }
    }
    for (uint32_t f = 0; f < F && ok && !took_scalar && !took_together; ++f) {
      const uint32_t fb = rl(nb, f), fc = rl(nc, f);
      const float fd = __uint_as_float(rl(__float_as_uint(d), f));
      for (uint32_t base = 0; base < fc && ok; base += 64) {
        const bool have = base + lane < fc;
        uint4 a = make_uint4(0, 0, 0, 0);
        uint2 nx = make_uint2(0, 0);
        if (use_pf && base == 0u) {  // (F == 1: f == 0)
          a = pf_a;
          nx = pf_nx;
          PT_MARK(1)  // general level: bookkeeping since the early issue (under the load)
        } else {
          PT_MARK(2)  // general level: from the rows' arrival to the next rows' issue
          if (have) {
            a = ld_global16(f2.arcs + fb + base + lane);
            nx = *reinterpret_cast<const uint2*>(reinterpret_cast<const char*>(f2.anext) + 8ull * (fb + base + lane));
          }
        }
        PT_ROWS_IN()
        PT_MARK(0)  // general level: waiting for the rows
        uint64_t m = __ballot(have && a.x == label);  // the label-equal run of fst2's (sorted) block, in arc order
        n_arcs += (uint32_t)__popcll(m);
        if (F == 1u && fc <= 64u && !scalar_rows && pos + 1u < L_u && m != 0ull && (m & (m - 1ull)) == 0ull) {
          // the one match makes the one state of level pos + 1 (on_match: n_new = 1, its block = [xb, xb + xc)).  Everything
          // of this level's rows is read off first, so that nothing below waits for vector memory again.
          const uint32_t l = (uint32_t)__ffsll((unsigned long long)m) - 1u;
          const uint32_t qd = rl(a.w, l), ol = rl(a.y, l), xb = rl(nx.x, l), xc = rl(nx.y, l);
          const float w2 = __uint_as_float(rl(a.z, l));
          pf_a = make_uint4(0, 0, 0, 0);
          pf_nx = make_uint2(0, 0);
          if (lane < xc) {
            pf_a = ld_global16(f2.arcs + xb + lane);
            pf_nx = *reinterpret_cast<const uint2*>(reinterpret_cast<const char*>(f2.anext) + 8ull * (xb + lane));
          }
          pf = true;
          PT_MARK(2)
          if (!on_match(f, fd, qd, ol, xb, xc, w2)) ok = false;
          m = 0;
        }
        while (m) {
          const uint32_t l = (uint32_t)__ffsll((unsigned long long)m) - 1u;
          m &= m - 1;
          if (!on_match(f, fd, rl(a.w, l), rl(a.y, l), rl(nx.x, l), rl(nx.y, l), __uint_as_float(rl(a.z, l)))) {
            ok = false;
            break;
          }
        }
      }
    }
    lo = hi;
    hi += n_new;
    F = n_new;
    q = nq;
    nb = nnb;
    nc = nnc;
    d = nd;
    if (F) level = pos + 1;
  }
  PT_MARK(2)
  if (!ok) {
    res.status = ST_NOT_A_STRING_CASE;
    STR_RESULT();
    return;
  }
  res.n_states = hi;
  res.n_arcs = n_arcs;
  res.n_levels = level + 1u;
  // final states: only level L can be final (fst1's single final state); rho = rho1 (x) rho2 (compose_fst_op.rs:420-449)
  lds_handoff();
  unsigned long long best = KEY_INF;
  float my_fin = INF;
  if (F && level == L) {  // the whole string was consumed
    const float fin1 = __uint_as_float(ld_global16(f1.srec + L).z);
    if (lane < F) {
      const float fin2 = __uint_as_float(ld_global16(f2.srec + q).z);
      if (fin1 != INF && fin2 != INF) my_fin = wtimes(fin1, fin2);
      if (d < INF && my_fin < INF) {
        const float tot = (d + my_fin) + 0.0f;
        if (tot < INF) best = ((unsigned long long)f32_key(tot) << 32) | (lo + lane);
      }
    }
  }
  best = wave_min_u64(best);
  if (best != KEY_INF) {
    const uint32_t fp = (uint32_t)best;
    res.has_path = 1;
    res.hops = L;
    res.final_weight = __uint_as_float(rl(__float_as_uint(my_fin), fp - lo));
    res.total = key_f32((uint32_t)(best >> 32));
    // The parents walked back by the whole wave: s_pth[k] = the k-th ancestor of fp (state k of the walk is in level L - k),
    // by pointer jumping in ceil(log2 L) rounds instead of L dependent LDS round trips of one lane.  Round r knows
    // s_pth[0 .. m) (m = 2^r) and J = "the m-th ancestor" of every state: s_pth[k] = J(s_pth[k - m]) for k in [m, 2m), then
    // J <- J o J.  J lives in one 16-bit half of s_par (state ids are below STR_MAXS; 0xFFFF = none, the low half of
    // STR_NONE) and the next J is written into the other half, so that no lane reads what another one writes in a round.
    static_assert(STR_MAXS <= 0x8000u, "state ids of the string kernel must fit 16 bits next to the `none` value");
    if (lane == 0) s_pth[0] = fp;
    lds_handoff();
    uint32_t sh = 0;  // the half of s_par that holds J
    for (uint32_t m = 1; m < L; m <<= 1, sh ^= 16u) {
      for (uint32_t k = m + lane; k < 2u * m && k < L; k += 64) {
        const uint32_t a = (s_par[s_pth[k - m]] >> sh) & 0xFFFFu;
        s_pth[k] = a == 0xFFFFu ? 0u : a;  // (never `none` below hop L: the chain from fp to state 0 has exactly L arcs)
      }
      if (2u * m < L) {
        for (uint32_t base = 0; base < hi; base += 256) {  // four loads in flight, then their four dependent loads
          uint32_t w[4], t[4];
#pragma unroll
          for (uint32_t c = 0; c < 4; ++c) {
            const uint32_t i = base + c * 64u + lane;
            w[c] = i < hi ? s_par[i] : STR_NONE;
          }
#pragma unroll
          for (uint32_t c = 0; c < 4; ++c) {
            const uint32_t a = (w[c] >> sh) & 0xFFFFu;
            t[c] = a == 0xFFFFu ? STR_NONE : s_par[a];
          }
#pragma unroll
          for (uint32_t c = 0; c < 4; ++c) {
            const uint32_t i = base + c * 64u + lane;
            const uint32_t keep = (w[c] >> sh) & 0xFFFFu, next = (t[c] >> sh) & 0xFFFFu;
            if (i < hi) s_par[i] = sh ? (keep << 16) | next : (next << 16) | keep;
          }
        }
      }
      lds_handoff();
    }
    if ((uint64_t)poff + L > path_cap) {
      res.status = ST_OVERFLOW_PATH;
    } else {
      res.path_off = poff;
      uint32_t facts = 0;
      for (uint32_t k = lane; k < L; k += 64) {  // arc k enters the k-th state created by the backtrace (shortest_path.rs:257-272)
        const uint32_t st = s_pth[k];
        const uint32_t il = ld_global16(f1.arcs + (L - 1u - k)).x;
        const uint32_t ol = s_ol[st];
        const float w = s_w[st];
        store_arc(path_buf + poff + k, il, ol, w, k);
        facts |= props::path_arc_facts(il, ol, w);
      }
      for (int d = 32; d >= 1; d >>= 1) facts |= __shfl_xor(facts, d);
      res.facts = facts;
    }
  }
  PT_MARK(7)  // epilogue: finals, pointer jumping, path write
  STR_RESULT();
}

#undef STR_RESULT

// ---------------------------------------------------------------- host side
FstView view_of(const wfst_fst* f) {
  FstView v;
  v.offsets = f->dev.offsets;
  v.arcs = f->dev.arcs;
  v.finals = f->dev.finals;
  v.noeps = f->dev.noeps;
  v.srec = f->dev.srec;
  v.anext = nullptr;
  v.n_states = f->n_states;
  v.start = (int32_t)f->start;
  v.n_arcs = f->n_arcs;
  return v;
}

uint32_t next_pow2(uint64_t x) {
  uint64_t p = 1;
  while (p < x) p <<= 1;
  if (p > 0x80000000ull) throw Error("composition too large for the wave-per-problem path");
  return (uint32_t)p;
}

Caps make_caps(uint64_t est_states, uint64_t est_arcs) {
  Caps c;
  uint64_t S = std::max<uint64_t>(est_states, 64);
  uint64_t A = std::max<uint64_t>(est_arcs, 128);
  if (S > 0x7FFFFFF0ull || A > 0x7FFFFFF0ull) throw Error("composition too large for the wave-per-problem path");
  c.S = (uint32_t)S;
  c.A = (uint32_t)A;
  c.H = next_pow2(2 * S + 128);
  c.W = 0;
  return c;
}

struct BatchRun {
  std::vector<Result> results;
  DBuf<char> arena;
  size_t stride = 0;
  Caps caps{};
  DBuf<wfst_tr> paths;
  std::vector<wfst_tr> h_paths;
  // in flight between launch_begin and launch_end
  size_t n = 0;
  bool want_paths = false;
  uint32_t path_cap = 1;
  DBuf<ProblemDesc> d_desc;
  DBuf<Result> d_res;
  DBuf<uint32_t> d_cursor;
  Result* h_res = nullptr;      // pinned (ctx->pinned_big): one batch in flight per context
  uint32_t* h_cursor = nullptr;
  // the first `eager` path records are copied to pinned memory right behind the kernel (no second round trip when
  // the paths fit, which they do unless T has input-epsilon cycles that stretch a path beyond its acceptor)
  wfst_tr* h_eager = nullptr;
  uint32_t eager = 0;
  const wfst_tr* host_paths = nullptr;
  bool string_kernel = false;  // this run went through string_compose_sp_kernel
  uint32_t str_used = 0;       // ... and this many arcs of its path buffer were handed out (ProblemDesc::path_off)
  const EnvSnap* env = nullptr;  // the WFST_* variables as the batch call found them (null: none of them is asked)
  uint32_t done_ticket = 0;    // ... with results in pinned memory: what every Result::done holds when its problem is finished
  // descriptors read from, results and path arcs written to pinned host memory by the kernel itself: no copy commands
  // (each is a ~3 us API call on the host and a ~5 us command on the GPU) — when the whole path buffer fits there
  bool zero_copy = false;
};
constexpr uint32_t ZERO_COPY_ARCS = 1u << 18;  // 4 MB of pinned memory per run
// ... of the string o T kernel, whose path buffer is exact (a path through A_i o T has |A_i| - 1 arcs at most when T has no
// input epsilons): 64 MB of pinned memory — a batch of 4096 strings of 200 labels writes its 13 MB of path arcs to the host
// while it runs, instead of a copy command behind the kernel
constexpr uint32_t ZERO_COPY_ARCS_STRING = 1u << 22;

inline size_t run_pinned_bytes(size_t n, uint32_t eager) {
  return ((n * (sizeof(ProblemDesc) + sizeof(Result)) + 64 + (size_t)eager * sizeof(wfst_tr)) + 255) & ~(size_t)255;
}

// Enqueues descriptors, the kernel and the result copies on ctx's stream and returns without waiting.
// `pinned` (optional): where this run's staging lives inside ctx->pinned_big (two runs of one job share the buffer);
// `string_kernel`: launch string_compose_sp_kernel (no arena) instead of compose_wave_kernel.
template <uint32_t FLAGS>
void launch_begin(wfst_ctx* ctx, const std::vector<ProblemDesc>& descs, const FstView& f2, const Caps& caps, BatchRun& run,
                  bool want_paths, uint32_t eager_paths = 0, char* pinned = nullptr, bool string_kernel = false,
                  uint32_t max_f1_states = 0, uint32_t exact_path_cap = 0) {
  const size_t n = descs.size();
  DevicePool& pool = *ctx->pool;
  hipStream_t st = ctx->stream;
  run.n = n;
  run.want_paths = want_paths;
  run.caps = caps;
  run.string_kernel = string_kernel;
  run.stride = string_kernel ? 0 : arena_bytes(caps);
  uint32_t path_cap = want_paths ? (uint32_t)std::min<uint64_t>((uint64_t)caps.S * n, 0x7FFFFFFFull) : 1u;
  if (exact_path_cap && want_paths) path_cap = std::min(path_cap, exact_path_cap);  // (see ZERO_COPY_ARCS_STRING)
  run.path_cap = path_cap;
  run.eager = want_paths ? std::min(eager_paths, path_cap) : 0u;
  run.zero_copy = want_paths && pinned && run.eager == path_cap && !ctx->profiling;
  // device blocks: only what the run's kernel reads or writes (a zero-copy string run: none at all — every take and return
  // of a pool block is host time in front of the launch)
  if (!string_kernel) {
    run.arena = DBuf<char>(pool, run.stride * n);
    run.d_cursor = DBuf<uint32_t>(pool, 1);
  }
  if (!run.zero_copy) {
    run.d_desc = DBuf<ProblemDesc>(pool, n);
    run.d_res = DBuf<Result>(pool, n);
    run.paths = DBuf<wfst_tr>(pool, path_cap);
  }
  ProblemDesc* h_desc = (ProblemDesc*)(pinned ? pinned : (char*)ctx->pinned_big.get(run_pinned_bytes(n, run.eager)));
  std::memcpy(h_desc, descs.data(), n * sizeof(ProblemDesc));
  run.str_used = 0;
  if (string_kernel) {
    // the path of problem i has at most n_states_i - 1 arcs (no input epsilons in fst2): its slice is known here, so the
    // kernel needs no cursor — no memset command in front of it, no returning atomic at the end of every wave
    uint64_t off = 0;
    for (size_t i = 0; i < n; ++i) {
      h_desc[i].path_off = (uint32_t)off;
      off += h_desc[i].f1.n_states ? h_desc[i].f1.n_states - 1u : 0u;
    }
    if (want_paths && off > path_cap) throw Error("compose_shortest_path_batch: the string run's paths exceed its path buffer (internal error)");
    run.str_used = (uint32_t)off;
  }
  run.h_res = (Result*)((char*)h_desc + n * sizeof(ProblemDesc));
  run.h_cursor = (uint32_t*)((char*)run.h_res + n * sizeof(Result));
  run.h_eager = (wfst_tr*)((char*)run.h_cursor + 64);
  const ProblemDesc* k_desc = run.zero_copy ? h_desc : run.d_desc.p;
  Result* k_res = run.zero_copy ? run.h_res : run.d_res.p;
  wfst_tr* k_paths = run.zero_copy ? run.h_eager : run.paths.p;
  if (!run.zero_copy) HIP_CHECK(hipMemcpyAsync(run.d_desc.p, h_desc, n * sizeof(ProblemDesc), hipMemcpyHostToDevice, st));
  if (!string_kernel) HIP_CHECK(hipMemsetAsync(run.d_cursor.p, 0, sizeof(uint32_t), st));
  if (ctx->profiling) HIP_CHECK(hipEventRecord(ctx->ev0, st));
  if (string_kernel) {
    // states per problem, then waves per workgroup (string_placement.h): 64 KB of LDS per workgroup at most
    uint32_t maxs = STR_MAXS;
    const EnvSnap none;
    const EnvSnap& env = run.env ? *run.env : none;
    const bool unpacked = env.has("WFST_STRING_UNPACKED");
    if (!unpacked && n >= STRING_PACK_MIN) {
      // a string of L arcs against an input-deterministic-ish T composes to a little more than L states; a problem that
      // outgrows its slice reports ST_NOT_A_STRING_CASE and is redone by the general kernel like any other misfit
      const uint64_t need = max_f1_states ? 2ull * max_f1_states + 64 : STR_MAXS;
      maxs = need <= 512 ? 512u : (need <= 1024 ? 1024u : STR_MAXS);
    }
    // (WFST_STRING_UNPACKED: one wave per workgroup whatever else is set; WFST_STRING_WPB=8: the packing of every batch of 16
    // strings or more before the rule)
    const StringPlacement pl = string_placement(n, maxs, (uint32_t)std::max(ctx->n_cus, 1), resident_grid_at_work(ctx->device),
                                                unpacked ? 1u : string_forced_wpb(env.get("WFST_STRING_WPB")));
    const uint32_t wpb = pl.wpb;
    ctx->string_placement = {wpb, maxs, pl.workgroups, pl.packed_for_resident ? 1u : 0u, pl.forced ? 1u : 0u};
    // tickets for serving-size batches only: the fence in front of a ticket writes the L2 back, and thousands of waves doing
    // that made a 4096-problem batch 0.7 ms slower; a kernel of milliseconds does not care about 10 us of wake-up latency
    static std::atomic<uint32_t> tickets{0};
    run.done_ticket = 0;
    if (run.zero_copy && n <= 1024 && !ctx->profiling && !env.has("WFST_BATCH_STREAM_WAIT")) {
      do run.done_ticket = tickets.fetch_add(1, std::memory_order_relaxed) + 1u; while (run.done_ticket == 0u);
      for (size_t i = 0; i < n; ++i) run.h_res[i].done = 0u;
    }
    string_compose_sp_kernel<<<(uint32_t)((n + wpb - 1) / wpb), 64 * wpb, (size_t)wpb * 16u * maxs, st>>>(
        k_desc, f2, k_res, k_paths, path_cap, (uint32_t)n, maxs, f2.n_arcs,
        // scalar arc-block loads for a handful of strings: -7 % per level.  Not for a batch, even where every wave is alone on
        // its SIMD (string_placement.h): 64 strings at one wave per workgroup take 104.3 us of batch finish with scalar rows and
        // the run forced on them against 95.0 with vector rows (profiles/string_placement_ab.md section 7)
        env.has("WFST_STRING_SCALAR") ? (uint32_t)std::atoi(env.get("WFST_STRING_SCALAR")) : (n <= 8 ? 1u : 0u),
        // the chase run of the vector path (WFST_STRING_RUN=0: every level is the general one; 2: also on the scalar-row path:
        // a measurement setting — profiles/string_run_ab.md has its figure; launches of <= 8 strings keep their route)
        env.has("WFST_STRING_RUN") ? (uint32_t)std::min(std::max(std::atoi(env.get("WFST_STRING_RUN")), 0), 2) : 1u,
        // pair levels inside the run of the vector path (WFST_STRING_PAIR=0: a run ends at every level that is not one state
        // with one match, as before profiles/string_pair_ab.md)
        env.has("WFST_STRING_PAIR") ? (std::atoi(env.get("WFST_STRING_PAIR")) != 0 ? 1u : 0u) : 1u, run.done_ticket);
  } else {
    compose_wave_kernel<FLAGS><<<(uint32_t)n, 64, 0, st>>>(k_desc, f2, caps, run.arena.p, run.stride, k_res, k_paths, path_cap,
                                                            run.d_cursor.p);
    ctx->compose_path.caps_states = caps.S;
    ctx->compose_path.caps_arcs = caps.A;
    ctx->compose_path.caps_hash = caps.H;
  }
  HIP_CHECK(hipGetLastError());
  if (ctx->profiling) HIP_CHECK(hipEventRecord(ctx->ev1, st));
  if (run.zero_copy) return;
  HIP_CHECK(hipMemcpyAsync(run.h_res, run.d_res.p, n * sizeof(Result), hipMemcpyDeviceToHost, st));
  if (!string_kernel) HIP_CHECK(hipMemcpyAsync(run.h_cursor, run.d_cursor.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  if (run.eager)
    HIP_CHECK(hipMemcpyAsync(run.h_eager, run.paths.p, (size_t)run.eager * sizeof(wfst_tr), hipMemcpyDeviceToHost, st));
}

// Waits for the batch enqueued by launch_begin and brings results (and the path arcs) to the host.
void launch_end(wfst_ctx* ctx, BatchRun& run) {
  const size_t n = run.n;
  hipStream_t st = ctx->stream;
  Result* h_res = run.h_res;
  uint32_t* h_cursor = run.h_cursor;
  const bool want_paths = run.want_paths;
  const uint32_t path_cap = run.path_cap;
  // The string kernel's results in pinned memory carry a ticket each: the host reads them as they land — a stream wait first
  // retires whatever else has finished on the stream and wakes up ~10 us after the kernel — and falls back to the stream.
  bool seen = false;
  if (run.string_kernel && run.done_ticket != 0u) {
    const auto t0 = std::chrono::steady_clock::now();
    size_t next = 0;
    for (uint32_t spins = 0;; ++spins) {
      while (next < n && ((const volatile Result*)h_res)[next].done == run.done_ticket) ++next;
      if (next == n) {
        std::atomic_thread_fence(std::memory_order_acquire);
        seen = true;
        break;
      }
      cpu_relax();
      if ((spins & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;  // (a long batch: sleep on the stream)
    }
  }
  if (!seen) HIP_CHECK(hipStreamSynchronize(st));
  else HIP_CHECK(hipPeekAtLastError());  // (no stream wait on this path.  Reports launch-configuration / sticky API errors the runtime has already
                                              // seen — NOT an asynchronous kernel fault: a chain that faults never writes its ticket, and the spin above then
                                              // ends in the stream wait, which reports it.  Peek, not Get: the error may belong to another thread's launch)
  if (ctx->profiling) {
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    ctx->stats.compose_ms = ms;
  }
  run.results.assign(h_res, h_res + n);
#ifdef WFST_PHASE_TIMING
  if (run.string_kernel) {
    unsigned long long tot[8] = {0, 0, 0, 0, 0, 0, 0, 0}, lv = 0, rlv = 0;
    for (size_t i = 0; i < n; ++i) {
      for (int k = 0; k < 8; ++k) tot[k] += h_res[i].dbg[k];
      lv += h_res[i].n_levels;
      rlv += h_res[i].run_levels;
    }
    if (std::getenv("WFST_PHASE_PER_PROBLEM"))  // one line per problem: its stamped total against the levels it took outside runs
      for (size_t i = 0; i < n; ++i) {
        unsigned long long sum = 0;
        for (int k = 0; k < 8; ++k) sum += h_res[i].dbg[k];
        std::fprintf(stderr, "[string problem] %zu cycles %llu levels %u in_runs %u pair_levels %u\n", i, sum, h_res[i].n_levels, h_res[i].run_levels, h_res[i].pair_levels);
      }
    {  // where the waves landed: a compute unit is (XCD, SE, SH, CU), a SIMD one of its four
      std::map<uint32_t, uint32_t> per_cu, per_simd;
      uint32_t xcds = 0;
      for (size_t i = 0; i < n; ++i) {
        const uint32_t hw = h_res[i].hw_id, xcc = h_res[i].xcc_id & 15u;
        const uint32_t cu = (xcc << 8) | (((hw >> 13) & 7u) << 5) | (((hw >> 12) & 1u) << 4) | ((hw >> 8) & 15u);
        per_cu[cu] += 1;
        per_simd[(cu << 2) | ((hw >> 4) & 3u)] += 1;
        xcds |= 1u << xcc;
      }
      uint32_t max_cu = 0, max_simd = 0;
      for (const auto& kv : per_cu) max_cu = std::max(max_cu, kv.second);
      for (const auto& kv : per_simd) max_simd = std::max(max_simd, kv.second);
      std::fprintf(stderr, "[string landing] %u waves per workgroup, %u workgroups: waves per CU: max %u / mean %.2f (%zu CUs); waves per SIMD: max %u / mean %.2f (%zu SIMDs); XCDs used %d\n",
                   (unsigned)ctx->string_placement.waves_per_workgroup, (unsigned)ctx->string_placement.workgroups, max_cu, (double)n / per_cu.size(),
                   per_cu.size(), max_simd, (double)n / per_simd.size(), per_simd.size(), __builtin_popcount(xcds));
    }
    std::fprintf(stderr, "[string phase ticks/problem] general: rows wait %llu | under the early load %llu | arrival->issue %llu || run: rows wait %llu | arrival->issue %llu | under the load %llu || prologue %llu | epilogue %llu  (n=%zu, levels/problem %.1f, of them in runs %.1f)\n",
                 tot[0] / n, tot[1] / n, tot[2] / n, tot[4] / n, tot[5] / n, tot[3] / n, tot[6] / n, tot[7] / n, n, (double)lv / n, (double)rlv / n);
  }
  if (!run.string_kernel) {
    unsigned long long tot[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t i = 0; i < n; ++i)
      for (int k = 0; k < 8; ++k) tot[k] += h_res[i].dbg[k];
    std::fprintf(stderr, "[phase cycles/problem] clear %llu | expand %llu | dedupe %llu | hash %llu | store+compact %llu | general %llu | epilogue %llu  (n=%zu, levels of problem 0: %u)\n",
                 tot[0] / n, tot[1] / n, tot[2] / n, tot[3] / n, tot[4] / n, tot[5] / n, tot[6] / n, n, h_res[0].n_levels);
  }
#endif
  if (want_paths && run.zero_copy) {
    run.host_paths = run.h_eager;  // written by the kernel
  } else if (want_paths) {
    // (arcs of the path buffer in use: the host's own sum for a string run, the kernel's cursor otherwise)
    const uint32_t used = std::min<uint32_t>(run.string_kernel ? run.str_used : *h_cursor, path_cap);
    if (used <= run.eager) {
      run.host_paths = run.h_eager;
    } else {
      run.h_paths.resize(used);
      HIP_CHECK(hipMemcpyAsync(run.h_paths.data(), run.paths.p, (size_t)used * sizeof(wfst_tr), hipMemcpyDeviceToHost, st));
      HIP_CHECK(hipStreamSynchronize(st));
      run.host_paths = run.h_paths.data();
    }
  }
}

template <uint32_t FLAGS>
void launch(wfst_ctx* ctx, const std::vector<ProblemDesc>& descs, const FstView& f2, const Caps& caps, BatchRun& run,
            bool want_paths) {
  launch_begin<FLAGS>(ctx, descs, f2, caps, run, want_paths);
  launch_end(ctx, run);
}

// builds the reference's linear shortest-path FST (see fst_store.hip::make_path_fst)
wfst_fst* path_to_fst(wfst_ctx* ctx, const Result& r, const wfst_tr* path_arcs) {
  HostCsr h;
  uint32_t n_states = 0;
  int64_t start = -1;
  if (r.has_path) {
    n_states = r.hops + 1;
    h.finals.assign(n_states, INF);
    h.finals[0] = r.final_weight;
    if (r.hops) h.arcs.assign(path_arcs, path_arcs + r.hops);
    h.offsets.resize((size_t)n_states + 1);
    h.offsets[0] = 0;
    for (uint32_t k = 0; k <= r.hops; ++k) h.offsets[k + 1] = k;
    start = r.hops;
  } else {
    h.offsets.push_back(0);
  }
  const uint64_t p = r.has_path && r.facts != props::PATH_FACTS_NONE
                         ? props::linear_path_props_from_facts(true, r.hops, r.final_weight, r.facts)
                         : props::linear_path_props(r.has_path != 0, r.hops, r.final_weight, path_arcs);
  return make_host_fst(ctx, n_states, start, p, std::move(h));
}

// ... the same FST as a view: the arcs stay where the kernel wrote them (the job's pinned block, kept alive by the handle)
// until somebody reads the FST's arrays (ensure_host).  A batch of 64 costs ~8 us this way instead of ~47 (three vectors,
// 5 KB written and 3 KB copied per path), behind the kernel, on the critical path of a serving loop.
wfst_fst* path_view_fst(wfst_ctx* ctx, const Result& r, const wfst_tr* path_arcs, const std::shared_ptr<PinnedBlock>& block) {
  auto f = std::make_unique<wfst_fst>();
  f->ctx = ctx;
  f->owner_pool = ctx->pool;
  f->device = ctx->device;
  f->n_states = r.hops + 1;
  f->n_arcs = r.hops;
  f->start = r.hops;
  f->props = (r.facts != props::PATH_FACTS_NONE ? props::linear_path_props_from_facts(true, r.hops, r.final_weight, r.facts)
                                                : props::linear_path_props(true, r.hops, r.final_weight, path_arcs)) & props::ALL;
  f->path_block = block;
  f->path_arcs = path_arcs;
  f->path_final = r.final_weight;
  f->path_form = true;
  return f.release();
}

const char* status_name(uint32_t s) {
  switch (s) {
    case ST_OVERFLOW_STATES: return "states";
    case ST_OVERFLOW_ARCS: return "arcs";
    case ST_OVERFLOW_HASH: return "hash";
    case ST_OVERFLOW_PATH: return "path";
    default: return "ok";
  }
}

// wfst_ctx_get_compose_path_stats: one status word of a finished launch.  `first`: this launch was the problem's first
// on compose_wave_kernel (ST_OK then counts as answered there); string-kernel results pass first = false.
void tally_status(wfst_ctx* ctx, uint32_t status, bool string_kernel, bool first) {
  wfst_ctx::ComposePathStats& c = ctx->compose_path;
  switch (status) {
    case ST_OK: if (string_kernel) c.string_answered++; else if (first) c.wave_first++; break;
    case ST_OVERFLOW_STATES: c.relaunch_states++; break;
    case ST_OVERFLOW_ARCS: c.relaunch_arcs++; break;
    case ST_OVERFLOW_HASH: c.relaunch_hash++; break;
    case ST_OVERFLOW_PATH: c.relaunch_path++; break;
    case ST_NOT_A_STRING_CASE: c.string_handed_back++; break;
    case ST_SWITCH_WIDE: c.switched_wide++; break;
    case ST_TIE_ORDER: c.two_step++; break;
    default: break;
  }
}

}  // namespace

// ComposeFstOp::match_type (compose_fst_op.rs:169-197) with SortedMatcher::match_type
// (matchers/sorted_matcher.rs:56-85): decided from the property bits only.
uint32_t decide_match_mode(uint64_t p1, uint64_t p2) {
  using namespace props;
  const bool o_sorted = p1 & O_LABEL_SORTED, o_known = p1 & (O_LABEL_SORTED | NOT_O_LABEL_SORTED);
  const bool i_sorted = p2 & I_LABEL_SORTED, i_known = p2 & (I_LABEL_SORTED | NOT_I_LABEL_SORTED);
  if (o_sorted && i_sorted) return MODE_BOTH;
  if (o_sorted) return MODE_OUTPUT;
  if (i_sorted) return MODE_INPUT;
  // neither known-sorted: match_type(true) -> properties_check fails when the bit pair is unknown
  if (!o_known) throw Error("ComposeFst: 1st argument: label-sortedness properties are not known (sort?)");
  if (!i_known) throw Error("ComposeFst: 2nd argument: label-sortedness properties are not known (sort?)");
  throw Error(
      "ComposeFst: 1st argument cannot match on output labels and 2nd argument cannot match on input labels (sort?).");
}

wfst_fst* compose(wfst_ctx* ctx, const wfst_fst* f1, const wfst_fst* f2, bool connect, uint32_t filter) {
  if (f1->n_states > TUPLE_S1_MASK) throw Error("compose: the 1st FST has more than 2^30 states");
  const uint32_t mode = decide_match_mode(f1->props, f2->props);
  ctx->compose_path = wfst_ctx::ComposePathStats{};
  ensure_device(const_cast<wfst_fst*>(f1));
  ensure_device(const_cast<wfst_fst*>(f2));
  const bool has_start = f1->start >= 0 && f2->start >= 0;
  const uint64_t out_props = props::compose_result(f1->props, f2->props, connect, has_start);
  if (!has_start) {  // compute_start -> None: empty FST (lazy_fst.rs:229-232)
    HostCsr h;
    h.offsets.push_back(0);
    return make_host_fst(ctx, 0, -1, out_props, std::move(h));
  }
  std::vector<ProblemDesc> descs(1);
  descs[0].f1 = view_of(f1);
  descs[0].mode = mode;
  descs[0].filter = filter;
  const FstView v2 = view_of(f2);
  // first guess from the SMALLER operand (acceptor o transducer lattices are a few times the acceptor; the arena and its
  // hash table are cleared per attempt, so a guess from a 5M-state operand costs tens of ms before any work): larger
  // results retry with 4x
  uint64_t est_s = 4ull * std::max<uint64_t>(std::min(f1->n_states, f2->n_states), 64) + 1024;
  uint64_t est_a = 4ull * est_s;
  bool wide_ok = true;  // WFST_COMPOSE_PATH=wave pins the wave-per-problem kernel, =wide the wide driver (tests)
  if (const char* e = std::getenv("WFST_COMPOSE_PATH")) {
    if (std::strcmp(e, "wave") == 0) wide_ok = false;
    if (std::strcmp(e, "wide") == 0) return compose_wide(ctx, f1, f2, mode, filter, connect, out_props, est_s);
  }
  for (int attempt = 0;; ++attempt) {
    Caps caps = make_caps(est_s, est_a);
    if (wide_ok) caps.W = WIDE_COMPOSE_WIDTH;
    BatchRun run;
    if (connect)
      launch<FLAG_TRIM>(ctx, descs, v2, caps, run, false);
    else
      launch<0>(ctx, descs, v2, caps, run, false);
    const Result& r = run.results[0];
    ctx->stats.compose_states = r.n_states;
    ctx->stats.compose_arcs = r.n_arcs;
    tally_status(ctx, r.status, false, attempt == 0);
    if (r.status == ST_OK) {
      const Arena a = carve_arena(run.arena.p, run.caps);  // the finished arrays, where the kernel put them
      if (connect)
        return adopt_device(ctx, r.t_states, r.t_arcs, r.t_start, out_props, a.t_off, a.t_arcs, a.t_fin);
      return adopt_device(ctx, r.n_states, r.n_arcs, r.n_states ? 0 : -1, out_props, a.off, a.arcs, a.fin);
    }
    if (r.status == ST_SWITCH_WIDE) return compose_wide(ctx, f1, f2, mode, filter, connect, out_props, 4 * est_s);
    ctx->stats.compose_retries++;
    if (attempt > 24) throw Error(std::string("compose: arena overflow (") + status_name(r.status) + ") after retries");
    est_s *= 4;
    est_a *= 4;
    // a result that has outgrown WIDE_COMPOSE_STATES is not a job for ONE wave: the wide driver (compose_wide.hip: one
    // wave per composed state of a BFS level) does a million states in tens of ms where this kernel needs seconds
    if (wide_ok && est_s > WIDE_COMPOSE_STATES) {
      ctx->compose_path.switched_wide++;
      return compose_wide(ctx, f1, f2, mode, filter, connect, out_props, est_s);
    }
  }
}

// ================================================================ list form (wfst_compose_batch)
namespace {

constexpr size_t COMPOSE_BATCH_MAX_SLAB = (size_t)8 << 30;  // all slices of one launch together; beyond: KO before that launch

// one item's arena out of the slab: carve_arena's arrays without skey / parent (the fused shortest path's); ar == nullptr
// only measures
size_t carve_compose_slice(Slab s, const Caps& c, Arena* ar) {
  Arena a{};
  a.tuples = s.take<uint64_t>(c.S);
  a.hkeys = s.take<uint64_t>(c.H);
  a.arcs = s.take<wfst_tr>(c.A);
  a.t_arcs = s.take<wfst_tr>(c.A);
  a.hvals = s.take<uint32_t>(c.H);
  a.off = s.take<uint32_t>((size_t)c.S + 1);
  a.t_off = s.take<uint32_t>((size_t)c.S + 1);
  a.fin = s.take<float>(c.S);
  a.t_fin = s.take<float>(c.S);
  a.aux = s.take<uint32_t>(c.S);
  a.aux2 = s.take<uint32_t>(c.S);
  a.lvl = s.take<uint32_t>((size_t)c.S + 1);
  if (ar) *ar = a;
  return s.at();
}

}  // namespace

// The routing rule is stated in include/wfst.h; the host loop is batch_driver.h's.
void compose_batch(wfst_ctx* ctx, const wfst_fst* const* f1s, size_t n1, const wfst_fst* const* f2s, size_t n2, bool connect,
                   uint32_t filter, wfst_fst** outs, uint8_t* in_kernel) {
  wfst_ctx::ComposeBatchCounters& stats = ctx->compose_batch;
  const size_t n = std::max(n1, n2);
  check_items_owned(ctx, f1s, n1, "compose_batch");
  check_items_owned(ctx, f2s, n2, "compose_batch");
  auto first = [&](size_t i) { return f1s[n1 == 1 ? 0 : i]; };
  auto second = [&](size_t i) { return f2s[n2 == 1 ? 0 : i]; };
  enum : uint8_t { NO_START, KERNEL, SINGLE, WIDE };
  struct Item {
    uint8_t kind = NO_START;
    uint32_t mode = 0;
    uint64_t out_props = 0;
    uint64_t est_s = 0, est_a = 0;  // the next attempt's estimate (compose()'s sequence)
    ComposeBatchCtl ctl{};          // of the attempt that finished
    Arena ar{};
  };
  std::vector<Item> items(n);
  // the single call's own errors, lowest index first, before anything is launched
  size_t live = 0;
  for (size_t i = 0; i < n; ++i) {
    const wfst_fst *f1 = first(i), *f2 = second(i);
    try {
      if (f1->n_states > TUPLE_S1_MASK) throw Error("compose: the 1st FST has more than 2^30 states");
      items[i].mode = decide_match_mode(f1->props, f2->props);
    } catch (const std::exception& e) {
      throw Error("item " + std::to_string(i) + ": " + e.what());
    }
    const bool has_start = f1->start >= 0 && f2->start >= 0;
    items[i].out_props = props::compose_result(f1->props, f2->props, connect, has_start);
    if (has_start) {
      items[i].kind = KERNEL;
      live += 1;
    }
  }
  const bool arena_min = arena_min_knob("WFST_COMPOSE_BATCH_ARENA");
  stats = {};  // (every refusal that needs no launch is behind us: such a call leaves the last call's counters alone)
  std::vector<size_t> open;
  for (size_t i = 0; i < n; ++i) {
    Item& it = items[i];
    if (it.kind != KERNEL) continue;
    if (live == 1) {  // the single call, limits and all
      it.kind = SINGLE;
      continue;
    }
    const wfst_fst *f1 = first(i), *f2 = second(i);
    it.est_s = arena_min ? 64 : 4ull * std::max<uint64_t>(std::min(f1->n_states, f2->n_states), 64) + 1024;
    it.est_a = arena_min ? 128 : 4ull * it.est_s;
    ensure_device(const_cast<wfst_fst*>(f1));
    ensure_device(const_cast<wfst_fst*>(f2));
    if (it.est_s > WIDE_COMPOSE_STATES) {  // (k = 0: min(n_states1, n_states2) > 3840)
      it.kind = WIDE;
      continue;
    }
    open.push_back(i);
  }
  hipStream_t st = ctx->stream;
  auto carve = [&](size_t i, Slab s, ComposeBatchItem* out) {
    const Caps caps = make_caps(items[i].est_s, items[i].est_a);  // (W = 0: no width hand-over in a list)
    Arena ar{};
    const size_t end = carve_compose_slice(s, caps, &ar);
    if (out) {
      out->f1 = view_of(first(i));
      out->f2 = view_of(second(i));
      out->mode = items[i].mode;
      out->filter = filter;
      out->caps = caps;
      out->ar = ar;
    }
    return end;
  };
  auto launch = [&](const ComposeBatchItem* d_items, uint32_t m) {
    if (connect)
      compose_batch_kernel<FLAG_TRIM><<<m, 64, 0, st>>>(d_items);
    else
      compose_batch_kernel<0><<<m, 64, 0, st>>>(d_items);
  };
  auto classify = [&](size_t i, const ComposeBatchCtl& c, const ComposeBatchItem& sent) {
    Item& it = items[i];
    if (c.done != 1u || c.status > ST_OVERFLOW_HASH || c.n_states > sent.caps.S || c.n_arcs > sent.caps.A ||
        c.t_states > c.n_states || c.t_arcs > c.n_arcs)
      throw Error("compose_batch: internal error: the kernel left item " + std::to_string(i) + " with status " +
                  std::to_string(c.status));
    if (c.status == ST_OK) {
      it.ctl = c;
      it.ar = sent.ar;
      return BatchExit::FINISHED;
    }
    (c.status == ST_OVERFLOW_STATES ? stats.regrown_states : c.status == ST_OVERFLOW_ARCS ? stats.regrown_arcs : stats.regrown_hash) += 1;
    it.est_s *= 4;
    it.est_a *= 4;
    if (it.est_s > WIDE_COMPOSE_STATES) {  // not a job for one wave: the wide driver, with this estimate
      it.kind = WIDE;
      return BatchExit::SINGLE;
    }
    return BatchExit::GREW;
  };
  const auto slabs = batch_launch_loop<ComposeBatchItem, ComposeBatchCtl>(
      ctx, stats, {"compose_batch", BATCH_MAX_LAUNCHES, "an arena", COMPOSE_BATCH_MAX_SLAB, "launch"}, std::move(open), carve, nullptr,
      launch, classify);
  auto outcome = [&](size_t i) {
    const Item& it = items[i];
    if (it.kind == SINGLE || it.kind == WIDE) return BatchOutcome::single();
    if (it.kind == NO_START) {  // compute_start -> None: the empty FST (lazy_fst.rs:229-232)
      HostCsr h;
      h.offsets.push_back(0);
      stats.items_no_start += 1;
      return BatchOutcome::handle(make_host_fst(ctx, 0, -1, it.out_props, std::move(h)));
    }
    const ComposeBatchCtl& c = it.ctl;
    if (connect) return BatchOutcome::adopt({c.t_states, c.t_arcs, (int64_t)c.t_start, it.out_props, it.ar.t_off, it.ar.t_arcs, it.ar.t_fin});
    return BatchOutcome::adopt({c.n_states, c.n_arcs, c.n_states ? 0 : -1, it.out_props, it.ar.off, it.ar.arcs, it.ar.fin});
  };
  auto single = [&](size_t i) {
    const Item& it = items[i];
    if (it.kind == SINGLE) return compose(ctx, first(i), second(i), connect, filter);
    return compose_wide(ctx, first(i), second(i), it.mode, filter, connect, it.out_props, it.est_s);
  };
  batch_finish(ctx, stats, n, outs, in_kernel, outcome, single);
}

}  // namespace wfst

// One fused batch in flight: begin enqueues everything on the context's stream and returns; end waits,
// re-runs the (rare) problems whose arena overflowed with 4x capacities, and assembles the path FSTs.
struct wfst_batch_job {
  wfst_ctx* ctx = nullptr;
  size_t n = 0;
  wfst::FstView v2{};
  std::vector<wfst::ProblemDesc> descs;
  std::vector<const wfst_fst*> accs;  // the operands (borrowed): problems the fused kernel hands back (ST_TIE_ORDER)
  const wfst_fst* t = nullptr;
  uint32_t filter = 0;
  std::vector<size_t> slow;           // ... are redone as compose + shortest_path at the end
  std::vector<size_t> todo;
  uint64_t est_s = 0, est_a = 0;
  wfst::BatchRun run;
  // problems that took the string o T kernel (fst1 a linear epsilon-free acceptor, fst2 without input epsilons)
  std::vector<size_t> todo_s;
  wfst::BatchRun run_s;
  wfst::FstView v2_s{};  // fst2 with its per-arc destination ranges
  std::shared_ptr<wfst::PinnedBlock> pin_block;  // descriptors, results and path arcs of the job's runs (pinned host memory)
  wfst::EnvSnap env;  // the WFST_* variables when the call began: asked by begin, both launch halves and end
  std::vector<uint8_t> seen_wave;  // wfst_ctx_get_compose_path_stats: problems with a wave-kernel launch behind them (sized
                                   // by the first relaunch: empty on the usual call)
  bool first_wave(size_t idx) const { return seen_wave.empty() || !seen_wave[idx]; }
  void mark_wave(size_t idx) {
    if (seen_wave.empty()) seen_wave.assign(n, 0);
    seen_wave[idx] = 1;
  }
};

namespace wfst {

wfst_batch_job* compose_shortest_path_batch_begin(wfst_ctx* ctx, const wfst_fst* const* accs, size_t n, const wfst_fst* t,
                                                  uint32_t filter) {
  auto job = std::make_unique<wfst_batch_job>();
  job->ctx = ctx;
  job->n = n;
  ctx->compose_path = wfst_ctx::ComposePathStats{};
  ctx->string_run = {};
  ctx->string_pair = {};
  ctx->string_placement = {};
  if (n == 0) return job.release();
  job->env = EnvSnap::take();
  job->run_s.env = &job->env;
  ensure_device(const_cast<wfst_fst*>(t));
  job->v2 = view_of(t);
  job->accs.assign(accs, accs + n);
  job->t = t;
  job->filter = filter;
  job->descs.resize(n);
  job->todo.resize(n);
  uint64_t max_states = 64;
  for (size_t i = 0; i < n; ++i) {
    if (!accs[i]) throw Error("null acceptor in batch");
    if (accs[i]->n_states > TUPLE_S1_MASK) throw Error("compose: a 1st FST has more than 2^30 states");
    job->descs[i].mode = decide_match_mode(accs[i]->props, t->props);
    ensure_device(const_cast<wfst_fst*>(accs[i]));
    job->descs[i].f1 = view_of(accs[i]);
    job->descs[i].filter = filter;
    job->todo[i] = i;
    max_states = std::max<uint64_t>(max_states, accs[i]->n_states);
  }
  job->est_s = 4ull * max_states + 256;
  job->est_a = 2ull * job->est_s;
  // which problems are "string o T" (the decoding case)?
  bool string_ok = (filter == 0 || filter == 3) && t->n_arcs > 0 && t->n_arcs < 0xFFFFFFFFull;
  if (const char* e = job->env.get("WFST_STRING_KERNEL")) string_ok = string_ok && std::atoi(e) != 0;
  if (string_ok) {
    bool any = false;
    for (size_t i = 0; i < n && !any; ++i) any = accs[i]->is_string && accs[i]->n_states <= STR_MAXS;
    string_ok = any && !has_input_epsilons(ctx, t);
  }
  std::vector<ProblemDesc> d_str, d_gen;
  std::vector<size_t> todo_gen;
  uint64_t eager_s = 0, eager_g = 0;  // a path through A_i o T has at most |A_i| - 1 arcs unless T loops on input epsilons
  uint32_t max_str_states = 0;
  if (string_ok) {
    job->v2_s = job->v2;
    job->v2_s.anext = ensure_anext(ctx, t);
    string_ok = job->v2_s.anext != nullptr;
  }
  for (size_t i = 0; i < n; ++i) {
    if (string_ok && accs[i]->is_string && accs[i]->n_states <= STR_MAXS) {
      job->todo_s.push_back(i);
      d_str.push_back(job->descs[i]);
      eager_s += accs[i]->n_states;
      max_str_states = std::max(max_str_states, accs[i]->n_states);
    } else {
      todo_gen.push_back(i);
      d_gen.push_back(job->descs[i]);
      eager_g += accs[i]->n_states;
    }
  }
  job->todo.swap(todo_gen);
  uint32_t e_s = (uint32_t)std::min<uint64_t>(eager_s, 1u << 22), e_g = (uint32_t)std::min<uint64_t>(eager_g, 1u << 22);
  {  // a run whose whole path buffer fits in pinned memory writes there itself (launch_begin: zero_copy)
    const Caps c0 = make_caps(job->est_s, job->est_a);
    const uint64_t cap_s = (uint64_t)c0.S * d_str.size(), cap_g = (uint64_t)c0.S * d_gen.size();
    const bool allow = !job->env.has("WFST_BATCH_COPY");  // tests: the copy-command path
    if (allow && cap_s && cap_s <= ZERO_COPY_ARCS) e_s = (uint32_t)cap_s;
    else if (allow && eager_s && eager_s <= ZERO_COPY_ARCS_STRING) e_s = (uint32_t)eager_s;  // = the run's whole path buffer
    if (allow && cap_g && cap_g <= ZERO_COPY_ARCS) e_g = (uint32_t)cap_g;
  }
  const size_t pin_s = d_str.empty() ? 0 : run_pinned_bytes(d_str.size(), e_s);
  const size_t pin_g = d_gen.empty() ? 0 : run_pinned_bytes(d_gen.size(), e_g);
  // (a block of the context's ring, not its one staging buffer: the path FSTs this job returns keep pointing into it)
  job->pin_block = ctx->pinned_ring->take(pin_s + pin_g + 256);
  char* pin = (char*)job->pin_block->p;
  if (!d_str.empty())
    launch_begin<FLAG_SP>(ctx, d_str, job->v2_s, make_caps(job->est_s, job->est_a), job->run_s, true, e_s, pin, true, max_str_states,
                          (uint32_t)std::min<uint64_t>(eager_s, 0x7FFFFFFFull));
  if (!d_gen.empty())
    launch_begin<FLAG_SP>(ctx, d_gen, job->v2, make_caps(job->est_s, job->est_a), job->run, true, e_g, pin + pin_s, false);
  return job.release();
}

void compose_shortest_path_batch_end(wfst_batch_job* job_raw, wfst_fst** outs, uint64_t* composed_arcs, const PackedSink* sink) {
  std::unique_ptr<wfst_batch_job> job(job_raw);  // consumed whatever happens
  wfst_ctx* ctx = job->ctx;
  const size_t n = job->n;
  if (composed_arcs) *composed_arcs = 0;
  if (n == 0) return;
  if (!sink)
    for (size_t i = 0; i < n; ++i) outs[i] = nullptr;
  // result i: a path FST handle, or (sink) its record — straight from the kernel's result and path buffers
  const size_t rec_words = sink ? 4 + 4 * (size_t)sink->max_arcs : 0;
  // (views only into blocks of serving size: one surviving result would otherwise keep tens of MB pinned)
  const bool views = job->pin_block && job->pin_block->cap <= (4u << 20) && !job->env.has("WFST_BATCH_EAGER_PATHS");
  auto emit = [&](size_t i, const Result& r, const wfst_tr* arcs, bool in_block) {
    if (sink) pack_path_record(sink->out + i * rec_words, sink->max_arcs, r.has_path != 0, r.hops, r.final_weight, arcs);
    else if (views && in_block && r.has_path && r.hops) outs[i] = path_view_fst(ctx, r, arcs, job->pin_block);
    else outs[i] = path_to_fst(ctx, r, arcs);
  };
  uint64_t tot_arcs = 0, tot_states = 0, n_string_ok = 0;
  double ms = 0;
  const bool timing = job->env.has("WFST_HOST_TIMING");
  auto tnow = [] { return std::chrono::steady_clock::now(); };
  auto t_a = tnow();
  try {
    if (!job->todo_s.empty()) {  // results of the string o T kernel; what it did not cover joins the general list
      launch_end(ctx, job->run_s);
      const auto t_w = tnow();
      ms += ctx->stats.compose_ms;
      std::vector<size_t> more, ok;
      for (size_t k = 0; k < job->todo_s.size(); ++k) {
        const Result& r = job->run_s.results[k];
        tally_status(ctx, r.status, true, false);
        if (r.status != ST_OK) {
          (r.status == ST_TIE_ORDER ? job->slow : more).push_back(job->todo_s[k]);
          continue;
        }
        tot_arcs += r.n_arcs;
        tot_states += r.n_states;
        n_string_ok += 1;
        ctx->string_run.run_levels += r.run_levels;
        ctx->string_run.runs += r.runs;
        ctx->string_pair.pair_levels += r.pair_levels;
        ctx->string_pair.pair_splits += r.pair_splits;
        ok.push_back(k);
      }
      // the path FSTs (three small vectors and a handle each: ~0.4 us): a large batch shares them out among host threads
      // (records are a copy of ~3 KB each: fewer threads than for handles — creating a thread costs as much as ~50 records)
      const char* env_thr = job->env.get("WFST_HOST_THREADS");
      const unsigned n_thr = env_thr ? host_threads(ok.size(), env_thr)
                                     : (unsigned)std::min<size_t>(std::min(sink ? 8u : 16u, host_threads(1u << 16, nullptr)), ok.size() / (sink ? 512 : 256));
      parallel_chunks(n_thr, ok.size(), 64, [&](unsigned, uint64_t b, uint64_t e) {
        for (uint64_t q = b; q < e; ++q) {
          const Result& r = job->run_s.results[ok[q]];
          emit(job->todo_s[ok[q]], r, r.has_path && r.hops ? job->run_s.host_paths + r.path_off : nullptr, job->run_s.zero_copy);
        }
      });
      if (timing)
        std::fprintf(stderr, "[batch_end] string run: wait %.1f us, %zu results on %u thread(s) %.1f us\n",
                     std::chrono::duration<double, std::micro>(t_w - t_a).count(), ok.size(), std::max(1u, n_thr),
                     std::chrono::duration<double, std::micro>(tnow() - t_w).count());
      if (!more.empty()) {
        if (!job->todo.empty()) {  // the general run of this job is still in flight: collect it first
          launch_end(ctx, job->run);
          std::vector<size_t> again;
          for (size_t k = 0; k < job->todo.size(); ++k) {
            const Result& r = job->run.results[k];
            tally_status(ctx, r.status, false, job->first_wave(job->todo[k]));
            if (r.status != ST_OK) {
              if (r.status != ST_TIE_ORDER) job->mark_wave(job->todo[k]);
              (r.status == ST_TIE_ORDER ? job->slow : again).push_back(job->todo[k]);
              continue;
            }
            tot_arcs += r.n_arcs;
            tot_states += r.n_states;
            emit(job->todo[k], r, r.has_path && r.hops ? job->run.host_paths + r.path_off : nullptr, job->run.zero_copy && job->run.host_paths == job->run.h_eager);
          }
          more.insert(more.end(), again.begin(), again.end());
        }
        job->todo.swap(more);
        std::vector<ProblemDesc> cur(job->todo.size());
        for (size_t k = 0; k < job->todo.size(); ++k) cur[k] = job->descs[job->todo[k]];
        job->run = BatchRun{};
        launch_begin<FLAG_SP>(ctx, cur, job->v2, make_caps(job->est_s, job->est_a), job->run, true);
      }
    }
    for (int attempt = 0; !job->todo.empty(); ++attempt) {
      launch_end(ctx, job->run);
      auto t_b = tnow();
      if (timing) std::fprintf(stderr, "[batch_end] wait+copy %.1f us\n", std::chrono::duration<double, std::micro>(t_b - t_a).count());
      ms += ctx->stats.compose_ms;
      std::vector<size_t> again;
      for (size_t k = 0; k < job->todo.size(); ++k) {
        const Result& r = job->run.results[k];
        tally_status(ctx, r.status, false, job->first_wave(job->todo[k]));
        if (r.status != ST_OK) {
          if (r.status != ST_TIE_ORDER) job->mark_wave(job->todo[k]);
          (r.status == ST_TIE_ORDER ? job->slow : again).push_back(job->todo[k]);
          continue;
        }
        tot_arcs += r.n_arcs;
        tot_states += r.n_states;
        emit(job->todo[k], r, r.has_path && r.hops ? job->run.host_paths + r.path_off : nullptr, job->run.zero_copy && job->run.host_paths == job->run.h_eager);
      }
      if (timing) std::fprintf(stderr, "[batch_end] assemble %.1f us\n", std::chrono::duration<double, std::micro>(tnow() - t_b).count());
      job->todo.swap(again);
      if (job->todo.empty()) break;
      ctx->stats.compose_retries++;
      if (attempt > 24) throw Error("compose_shortest_path_batch: arena overflow after retries");
      job->est_s *= 4;
      job->est_a *= 4;
      std::vector<ProblemDesc> cur(job->todo.size());
      for (size_t k = 0; k < job->todo.size(); ++k) cur[k] = job->descs[job->todo[k]];
      job->run = BatchRun{};
      launch_begin<FLAG_SP>(ctx, cur, job->v2, make_caps(job->est_s, job->est_a), job->run, true);
    }
    for (size_t idx : job->slow) {  // handed back by the fused kernel: the two-step route (always applicable)
      const wfst_ctx::ComposePathStats batch_tally = ctx->compose_path;  // (compose() below starts its own tally)
      std::unique_ptr<wfst_fst> c(compose(ctx, job->accs[idx], job->t, true, job->filter));
      ctx->compose_path = batch_tally;
      tot_arcs += c->n_arcs;
      tot_states += c->n_states;
      if (sink) {
        std::unique_ptr<wfst_fst> p(shortest_path_n1(ctx, c.get()));
        pack_path_record(sink->out + idx * rec_words, sink->max_arcs, p.get());
      } else {
        outs[idx] = shortest_path_n1(ctx, c.get());
      }
    }
  } catch (...) {
    (void)hipStreamSynchronize(ctx->stream);  // (a run of this job may still be in flight: its buffers go with the job)
    if (!sink)
      for (size_t i = 0; i < n; ++i) {
        delete outs[i];
        outs[i] = nullptr;
      }
    throw;
  }
  ctx->stats.compose_states = tot_states;
  ctx->stats.compose_arcs = tot_arcs;
  ctx->stats.compose_ms = ms;
  ctx->stats.string_problems = n_string_ok;
  if (composed_arcs) *composed_arcs = tot_arcs;
}

wfst_ctx* batch_job_ctx(const wfst_batch_job* job) { return job->ctx; }

void compose_shortest_path_batch_abandon(wfst_batch_job* job) {
  if (!job) return;
  if (job->n) (void)hipStreamSynchronize(job->ctx->stream);  // the kernel may still be writing into the job's buffers
  delete job;
}

void compose_shortest_path_batch(wfst_ctx* ctx, const wfst_fst* const* accs, size_t n, const wfst_fst* t, bool /*connect*/,
                                 wfst_fst** outs, uint64_t* composed_arcs, uint32_t filter) {
  compose_shortest_path_batch_end(compose_shortest_path_batch_begin(ctx, accs, n, t, filter), outs, composed_arcs);
}

// path_to_fst for a kernel of another file that reports a path the way string_compose_sp_kernel does (compose_sigma_batch.hip)
wfst_fst* batch_path_fst(wfst_ctx* ctx, bool has_path, uint32_t hops, float final_weight, uint32_t facts, const wfst_tr* path_arcs) {
  Result r{};
  r.has_path = has_path ? 1u : 0u;
  r.hops = hops;
  r.final_weight = final_weight;
  r.facts = facts;
  return path_to_fst(ctx, r, path_arcs);
}

}  // namespace wfst

// The pair levels of the last fused-batch call of ctx (common.h: wfst_ctx::string_pair), beside their tally in
// compose_shortest_path_batch_end.  Either out-pointer may be null.
extern "C" wfst_status wfst_ctx_get_string_pair_counts(wfst_ctx* ctx, uint64_t* pair_levels, uint64_t* pair_splits) {
  return wfst::wrap([&] {
    if (!ctx) throw wfst::Error("null pointer");
    if (pair_levels) *pair_levels = ctx->string_pair.pair_levels;
    if (pair_splits) *pair_splits = ctx->string_pair.pair_splits;
  });
}

// Where the waves of ctx's last string launch sat (common.h: wfst_ctx::string_placement), beside launch_begin, which decides
// it.  Any out-pointer may be null.
extern "C" wfst_status wfst_ctx_get_string_placement(wfst_ctx* ctx, uint64_t* waves_per_workgroup, uint64_t* slice_states,
                                                     uint64_t* workgroups, uint64_t* packed_for_resident, uint64_t* forced) {
  return wfst::wrap([&] {
    if (!ctx) throw wfst::Error("null pointer");
    const wfst_ctx::StringPlacementCounts& c = ctx->string_placement;
    if (waves_per_workgroup) *waves_per_workgroup = c.waves_per_workgroup;
    if (slice_states) *slice_states = c.slice_states;
    if (workgroups) *workgroups = c.workgroups;
    if (packed_for_resident) *packed_for_resident = c.packed_for_resident;
    if (forced) *forced = c.forced;
  });
}
