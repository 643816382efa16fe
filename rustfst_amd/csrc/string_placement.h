// string_placement.h — how many waves of a one-wave-per-string kernel share a workgroup (string_compose_sp_kernel of
// compose.hip, string_sigma_sp_kernel of compose_sigma_batch.hip).  Every wave owns a slice of 16 * maxs bytes of the
// workgroup's dynamic LDS and the waves never meet, so the number decides only WHERE the waves sit: w waves behind one L1,
// ceil(n / w) compute units in use.  No HIP here: tests/placement_check.cpp includes it alone.
#pragma once
#include <cstdint>

namespace wfst {
constexpr uint32_t STRING_LDS_BYTES = 64u << 10;  // dynamic LDS of one workgroup of either kernel
constexpr uint32_t STRING_PACK_MIN = 16;          // launches of fewer strings: one wave per workgroup

struct StringPlacement {
  uint32_t wpb;            // waves per workgroup: 1, 2, 4 or 8
  uint32_t workgroups;     // ceil(n / wpb)
  bool packed_for_resident;  // the resident-grid line of the rule decided
  bool forced;             // the caller's value decided
};

// WFST_STRING_WPB as the rule takes it: the next lower power of two of a number >= 1, at most 8; 0 for a missing value, a
// zero and anything that does not begin with a digit.
inline uint32_t string_forced_wpb(const char* text) {
  if (!text || *text < '0' || *text > '9') return 0u;
  uint64_t v = 0;
  for (const char* c = text; *c >= '0' && *c <= '9' && v < 1000u; ++c) v = v * 10u + (uint64_t)(*c - '0');
  return v >= 8u ? 8u : (v >= 4u ? 4u : (v >= 2u ? 2u : (v >= 1u ? 1u : 0u)));
}

// n strings with slices of maxs states (512, 1024 or 2048) on a context of n_cus compute units.
//   forced 1, 2, 4, 8      -> that many, as far as the LDS holds them
//   fewer than 16 strings  -> 1
//   a resident grid works  -> what the LDS holds: a lone wave of these kernels keeps its whole compute unit from the
//                             1024-thread, 128-VGPR workgroups of a resident relaxation launch, which needs ~245 whole
//                             units at once and gives up after its wait limit
//   otherwise              -> the fewest waves per workgroup with a compute unit for every workgroup: a wave alone on its
//                             SIMD, a workgroup alone behind its L1, for as long as the context has them
inline StringPlacement string_placement(uint64_t n, uint32_t maxs, uint32_t n_cus, bool resident_at_work, uint32_t forced) {
  const uint32_t room = STRING_LDS_BYTES / (16u * (maxs ? maxs : 1u));
  const uint32_t cap = room >= 8u ? 8u : (room >= 4u ? 4u : (room >= 2u ? 2u : 1u));
  StringPlacement p{1u, 0u, false, false};
  if (forced) {
    const uint32_t f = forced >= 8u ? 8u : (forced >= 4u ? 4u : (forced >= 2u ? 2u : 1u));
    p.wpb = f < cap ? f : cap;
    p.forced = true;
  } else if (n < STRING_PACK_MIN) {
    p.wpb = 1u;
  } else if (resident_at_work) {
    p.wpb = cap;
    p.packed_for_resident = true;
  } else {
    uint32_t w = 1u;
    while (w < cap && (n + w - 1u) / w > (uint64_t)(n_cus ? n_cus : 1u)) w *= 2u;
    p.wpb = w;
  }
  p.workgroups = (uint32_t)((n + p.wpb - 1u) / p.wpb);
  return p;
}
}  // namespace wfst
