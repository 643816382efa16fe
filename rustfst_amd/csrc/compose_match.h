// compose_match.h — what every composition route needs from the sorted matcher and from the wave, stated once: the arc
// in registers and its loads, the wave primitives, the matcher's search, and the pieces of the expansion of one composed
// state that the policies of the wide driver share.  Included by compose.hip (one wave per problem), compose_wide.h (a few
// lanes per composed state; through it compose_wide.hip, compose_lookahead.hip, compose_sigma.hip and replace.hip) and
// sigma_ranges.h (through it compose_sigma_batch.hip).
//
// Like compose_wide.h, everything here sits in an anonymous namespace: each translation unit gets its own copy.
#pragma once
#include "common.h"
#include "compose_filters.h"

namespace wfst {
namespace {

constexpr uint32_t NO_LABEL = WFST_NO_LABEL;
enum : uint32_t { MODE_BOTH = 0, MODE_INPUT = 1, MODE_OUTPUT = 2 };  // MatchType after match_type() (decide_match_mode)

// ---------------------------------------------------------------- wave helpers (wave = 64 lanes)
__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }
__device__ __forceinline__ uint32_t lanes_below(uint64_t mask) {  // popcount of mask bits below this lane
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}
__device__ __forceinline__ uint32_t wave_excl_scan(uint32_t v, uint32_t lane, uint32_t* total) {
  uint32_t x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    uint32_t y = __shfl_up(x, d);
    if (lane >= (uint32_t)d) x += y;
  }
  *total = __shfl(x, 63);
  return x - v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = max(v, (uint32_t)__shfl_xor(v, d));
  return v;
}
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    unsigned long long o = __shfl_xor(v, d);
    v = o < v ? o : v;
  }
  return v;
}
__device__ __forceinline__ uint64_t shfl64(uint64_t v, uint32_t src) {
  return ((uint64_t)(uint32_t)__shfl((uint32_t)(v >> 32), src) << 32) | (uint32_t)__shfl((uint32_t)v, src);
}
// broadcast from a wave-uniform lane: v_readlane (scalar path) instead of a ds_bpermute round trip
__device__ __forceinline__ uint32_t rl(uint32_t v, uint32_t src) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)src);
}
__device__ __forceinline__ uint64_t rl64(uint64_t v, uint32_t src) {
  return ((uint64_t)rl((uint32_t)(v >> 32), src) << 32) | rl((uint32_t)v, src);
}
__device__ __forceinline__ uint4 rl128(uint4 v, uint32_t src) {
  return make_uint4(rl(v.x, src), rl(v.y, src), rl(v.z, src), rl(v.w, src));
}
__device__ __forceinline__ float rlf(float v, uint32_t src) { return __uint_as_float(rl(__float_as_uint(v), src)); }
// LDS traffic of one wave is processed in issue order, so what one lane wrote to LDS is read by the other lanes of the
// same wave behind this: they only need the compiler not to reorder around the hand-off and the LDS counter drained:
// no vmcnt wait, no s_barrier.
__device__ __forceinline__ void lds_handoff() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
// The wave is a whole workgroup (blockDim == 64): __syncthreads() is the wave-level fence that makes
// the lanes' global-memory writes visible to each other between phases.
__device__ __forceinline__ void wave_sync() { __syncthreads(); }

template <class T>
__device__ __forceinline__ T ld_l2(const T* p) {  // L2-served load for words other lanes update atomically
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <class T>
__device__ __forceinline__ void st_l2(T* p, T v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------- arcs in registers
// Pointers that reach the kernel through a descriptor in memory (fst1 of every problem) are generic to the compiler,
// which then emits FLAT loads: slower, and they tie the LDS and the vector-memory wait counters together.  Everything an
// FstView points to is device memory, so say so.
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef const u32x4_t __attribute__((address_space(1)))* global_u4_ptr;
__device__ __forceinline__ uint4 ld_global16(const void* p) {
  // (the integer round trip is what makes the compiler drop "generic")
  const u32x4_t v = *(global_u4_ptr)(unsigned long long)p;
  return make_uint4(v.x, v.y, v.z, v.w);
}
typedef const uint32_t __attribute__((address_space(1)))* global_u32_ptr;
__device__ __forceinline__ uint32_t ld_global4(const void* p) { return *(global_u32_ptr)(unsigned long long)p; }
// How load_arc and equal_range read: AnyLoad wherever the pointer points — the wide driver's la_emit moves the searched
// side's arcs to LDS and hands the policies that copy, so its callers cannot promise device memory —, GlobalLoad the
// forced-global form above (the wave kernels of compose.hip).
struct AnyLoad {
  static __device__ __forceinline__ uint4 u128(const void* p) { return *reinterpret_cast<const uint4*>(p); }
  static __device__ __forceinline__ uint32_t u32(const void* p) { return *reinterpret_cast<const uint32_t*>(p); }
};
struct GlobalLoad {
  static __device__ __forceinline__ uint4 u128(const void* p) { return ld_global16(p); }
  static __device__ __forceinline__ uint32_t u32(const void* p) { return ld_global4(p); }
};

struct ArcReg {
  uint32_t il, ol;
  float w;
  uint32_t ns;
};
template <class Ld = AnyLoad>
__device__ __forceinline__ ArcReg load_arc(const wfst_tr* p) {
  const uint4 v = Ld::u128(p);  // one 16-B load
  return ArcReg{v.x, v.y, __uint_as_float(v.z), v.w};
}
__device__ __forceinline__ void store_arc(wfst_tr* p, uint32_t il, uint32_t ol, float w, uint32_t ns) {
  *reinterpret_cast<uint4*>(p) = make_uint4(il, ol, __float_as_uint(w), ns);
}
__device__ __forceinline__ ArcReg shfl_arc(const ArcReg& a, uint32_t src) {
  return ArcReg{(uint32_t)__shfl(a.il, src), (uint32_t)__shfl(a.ol, src), __shfl(a.w, src), (uint32_t)__shfl(a.ns, src)};
}

// ---------------------------------------------------------------- the sorted matcher
// The run of `key` on the matched tape of a sorted arc block, [*lo_out, *lo_out + *cnt_out) relative to its first arc:
// lower / upper bound on the key column (superslice lower_bound_by, matchers/sorted_matcher.rs:141-142), per lane.
template <class Ld = AnyLoad>
__device__ void equal_range(const wfst_tr* arcs, uint32_t n, bool by_ilabel, uint32_t key, uint32_t* lo_out, uint32_t* cnt_out) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    uint32_t mid = lo + ((hi - lo) >> 1);
    uint32_t k = Ld::u32(by_ilabel ? &arcs[mid].ilabel : &arcs[mid].olabel);
    if (k < key) lo = mid + 1; else hi = mid;
  }
  uint32_t first = lo;
  hi = n;
  while (lo < hi) {
    uint32_t mid = lo + ((hi - lo) >> 1);
    uint32_t k = Ld::u32(by_ilabel ? &arcs[mid].ilabel : &arcs[mid].olabel);
    if (k <= key) lo = mid + 1; else hi = mid;
  }
  *lo_out = first;
  *cnt_out = lo - first;
}

// ---------------------------------------------------------------- expansion of one composed state (s1, s2), shared pieces
// match_input (compose_fst_op.rs:199-219) has decided `mi`: fst1 is iterated and fst2 searched, or the other way round.
// X is a policy's Expand: it_arcs / se_arcs, n_it / n_se, and sa / sb = the state of the searched / iterated side.
// (SigmaPolicy selects for itself: a state where both sides require has no items, and routed through here that cost its
// la_emit a step of occupancy.  So did, for every policy, a helper for the tail of eval_item that writes or keeps an
// emitted pair, which therefore stays where it was: profiles/compose_match_ab.md.)
template <class X>
__device__ __forceinline__ void select_sides(X& x, bool mi, const wfst_tr* arcs1, uint32_t n1, uint32_t s1, const wfst_tr* arcs2,
                                             uint32_t n2, uint32_t s2) {
  x.mi = mi;
  x.it_arcs = mi ? arcs1 : arcs2;
  x.se_arcs = mi ? arcs2 : arcs1;
  x.n_it = mi ? n1 : n2;
  x.n_se = mi ? n2 : n1;
  x.sa = mi ? s2 : s1;
  x.sb = mi ? s1 : s2;
}
// item 0 of a state: the loop pseudo-arc of the iterated side (ordered_expand, compose_fst_op.rs:229-233)
__device__ __forceinline__ ArcReg loop_item(bool mi, uint32_t sb) {
  return mi ? ArcReg{0u, NO_LABEL, 0.0f, sb} : ArcReg{NO_LABEL, 0u, 0.0f, sb};
}
// what the searched side's matcher yields first for label 0 (eps_loop, matchers/mod.rs:98-105)
__device__ __forceinline__ ArcReg eps_loop(bool mi, uint32_t sa) {
  return mi ? ArcReg{NO_LABEL, 0u, 0.0f, sa} : ArcReg{0u, NO_LABEL, 0.0f, sa};
}

}  // namespace
}  // namespace wfst
