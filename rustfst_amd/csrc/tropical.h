// tropical.h — TropicalWeight (f32; plus = min, times = +, zero = +inf, one = 0) with the reference's semantics, for host
// and device code alike.  These rules are the parity contract with rustfst: every file uses them from here.
// The header carries no floating-point contraction pragma: each function is compiled under the setting of the file that
// includes it (determinize.hip, minimize.hip and tr_sum.hip switch contraction off BEFORE including it).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define WFST_HD __host__ __device__
#else
#define WFST_HD
#endif

namespace wfst {

constexpr float INF = __builtin_huge_valf();
constexpr float KDELTA = 1.0f / 1024.0f;  // lib.rs:266

// plus_assign: the minimum by an exact < (semirings/tropical_weight.rs:42-58)
WFST_HD inline float wplus(float a, float b) { return b < a ? b : a; }
// times_assign: inf (x) x = x (x) inf = inf, else a + b in f32 (tropical_weight.rs:60-70)
WFST_HD inline float wtimes(float a, float b) { return a == INF ? a : (b == INF ? b : a + b); }
// the one-wavefront n-best kernels' times: (a + b) + 0.0f, which turns a -0.0 sum into +0.0 where wtimes keeps the sign.
// Their results are compared bit by bit with it; not to be merged with wtimes.
WFST_HD inline float nb_times(float a, float b) { return a == INF ? a : (b == INF ? b : (a + b) + 0.0f); }
// divide: a - b in f32, no inf check; DivideLeft == DivideRight (tropical_weight.rs:128-131)
WFST_HD inline float wdivide(float a, float b) { return a - b; }
// TropicalWeight's PartialEq: the APPROXIMATE == with KDELTA (semirings/semiring.rs:159-168)
WFST_HD inline bool weq(float a, float b) { return a <= b + KDELTA && b <= a + KDELTA; }
// is_zero / is_one go through that == (semiring.rs:68-73): a weight within 1/1024 of 0 is one
WFST_HD inline bool is_zero(float w) { return weq(w, INF); }
WFST_HD inline bool is_one(float w) { return weq(w, 0.0f); }
// what sets WEIGHTED in the property word (mutate_properties.rs:83-86, trs_iter_mut.rs:279-291)
WFST_HD inline bool weighted(float w) { return !is_zero(w) && !is_one(w); }
// quantize (semiring.rs:132-145)
WFST_HD inline float quantize(float v, float delta) {
  if (__builtin_isinf(v)) return v;
  return __builtin_floorf((v / delta) + 0.5f) * delta;
}
// approx_equal(delta) of the shortest-path searches (shortest_path.rs:288-338, shortest_distance.rs:216)
WFST_HD inline bool approx_equal(float a, float b, float delta) { return __builtin_fabsf(a - b) <= delta; }
// natural_less (shortest_path.rs:284-286)
WFST_HD inline bool natural_less(float w1, float w2) { return weq(wplus(w1, w2), w1) && !weq(w1, w2); }

// order-preserving u32 key of an f32 (negative weights included), for atomicMin on distances, and its inverse
WFST_HD inline uint32_t f32_key(float f) {
  uint32_t b;
  __builtin_memcpy(&b, &f, 4);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
WFST_HD inline float key_f32(uint32_t e) {
  const uint32_t b = (e & 0x80000000u) ? (e & 0x7FFFFFFFu) : ~e;
  float f;
  __builtin_memcpy(&f, &b, 4);
  return f;
}

}  // namespace wfst
