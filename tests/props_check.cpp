#include <cfloat>
#include <cstdio>
#include <cstring>
#include <vector>
#include <cstdint>
#include <cmath>
// Test program (tests/test_host.py::test_path_props_from_fact_union): linear_path_props_from_facts == linear_path_props on
// every sequence of up to six arcs over the fact combinations one arc can have.  Built with g++ -I<repo>/rustfst_amd/csrc.
// With the argument "arc_facts" (test_arc_facts_fold): add_tr folded over the two arcs of a state == add_trs_by_facts of the
// OR of their arc_facts.  With "tropical" (test_tropical_host_grid): the host side of tropical.h against literal restatements.
#include "fst_props.h"
using namespace wfst::props;

static uint32_t bits_of(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

// every state with two arcs over labels {0, 3, 5} (all epsilon / acceptor combinations, both label orders between the arcs),
// nextstate below, at and above the state, and the weights one, within KDELTA of one, weighted and zero
static int check_arc_facts() {
  const uint32_t labels[3] = {0u, 3u, 5u}, state = 4u;
  const float weights[4] = {0.0f, 0.0005f, 0.75f, INFINITY};
  std::vector<wfst_tr> arcs;
  for (uint32_t il : labels)
    for (uint32_t ol : labels)
      for (float w : weights)
        for (uint32_t ns = state - 1; ns <= state + 1; ++ns) arcs.push_back(wfst_tr{il, ol, w, ns});
  const uint64_t words[3] = {NULL_PROPS, add_state(NULL_PROPS), 0};
  long long n = 0, bad = 0;
  for (const wfst_tr& a : arcs) {
    const uint32_t fa = arc_facts(a, nullptr, state);
    if (path_arc_facts(a.ilabel, a.olabel, a.weight) != (fa | FACT_NOT_TOP_SORTED)) ++bad;
    if (fa & (FACT_NOT_I_SORTED | FACT_NOT_O_SORTED | FACT_FINAL_WEIGHTED)) ++bad;  // no predecessor: no label-order facts
    for (const wfst_tr& b : arcs) {
      const uint32_t facts = fa | arc_facts(b, &a, state);
      for (uint64_t in : words) {
        const uint64_t fold = add_tr(add_tr(in, state, a, nullptr), state, b, &a);
        ++n;
        if (fold != add_trs_by_facts(in, facts)) {
          if (bad < 5) printf("mismatch (%u %u %g %u) (%u %u %g %u) facts %u\n", a.ilabel, a.olabel, a.weight, a.nextstate, b.ilabel,
                              b.olabel, b.weight, b.nextstate, facts);
          ++bad;
        }
      }
    }
  }
  printf("%lld cases, %lld mismatches (%zu arcs)\n", n, bad, arcs.size());
  return bad != 0;
}

// +-0, denormals, +-KDELTA and its neighbours, the values next to FLT_MAX, inf (and a few ordinary weights); bit-exact
static int check_tropical() {
  using namespace wfst;
  std::vector<float> grid = {0.0f, -0.0f, FLT_TRUE_MIN, -FLT_TRUE_MIN, FLT_MIN / 2, -FLT_MIN / 2, FLT_MIN, -FLT_MIN, KDELTA, -KDELTA,
                             std::nextafter(KDELTA, 0.0f), std::nextafter(KDELTA, 1.0f), std::nextafter(-KDELTA, 0.0f),
                             std::nextafter(-KDELTA, -1.0f), KDELTA / 2, 1.5f * KDELTA, 0.5f, 0.75f, -2.25f, 1000.3f, FLT_MAX, -FLT_MAX,
                             std::nextafter(FLT_MAX, 0.0f), std::nextafter(-FLT_MAX, 0.0f), INFINITY};
  long long n = 0, bad = 0;
  auto expect = [&](const char* what, float a, float b, uint32_t got, uint32_t want) {
    ++n;
    if (got != want) {
      if (bad < 5) printf("%s(%a, %a): %08x, expected %08x\n", what, a, b, got, want);
      ++bad;
    }
  };
  for (float a : grid) {
    for (float b : grid) {
      const volatile float sum = a + b;
      expect("wtimes", a, b, bits_of(wtimes(a, b)), bits_of(a == INFINITY ? a : (b == INFINITY ? b : sum)));
      if (a < b) expect("f32_key order", a, b, f32_key(a) < f32_key(b), 1u);
    }
    for (float delta : {1.0f / 1024.0f, 1e-6f}) {
      const volatile float scaled = a / delta;
      const volatile float rounded = std::floor(scaled + 0.5f);
      expect("quantize", a, delta, bits_of(quantize(a, delta)), bits_of(std::isinf(a) ? a : rounded * delta));
    }
    expect("key_f32(f32_key)", a, 0.0f, bits_of(key_f32(f32_key(a))), bits_of(a));
    expect("is_zero", a, 0.0f, is_zero(a), a == INFINITY);
    expect("is_one", a, 0.0f, is_one(a), std::fabs(a) <= KDELTA);
  }
  printf("%lld cases, %lld mismatches (%zu values)\n", n, bad, grid.size());
  return bad != 0;
}

static wfst_tr arc_of(uint32_t f, uint32_t state) {  // facts bits 1,2,4,8,16 -> an arc of `state`
  wfst_tr a{};
  a.ilabel = (f & 2u) ? 0u : 3u;
  a.olabel = (f & 4u) ? 0u : ((f & 1u) ? 5u : a.ilabel);
  a.weight = (f & 8u) ? 0.75f : ((f & 1u) ? 0.0005f : 0.0f);
  a.nextstate = (f & 16u) ? state - 1 : state + 1;
  return a;
}
static bool consistent(uint32_t f) {  // il==0 && ol==0 -> il == ol: fact 1 must be clear; il==0 xor ol==0 -> il != ol
  const bool ie = f & 2u, oe = f & 4u, ne = f & 1u;
  if (ie && oe) return !ne;
  if (ie != oe) return ne;
  return true;
}
int main(int argc, char** argv) {
  if (argc > 1 && !std::strcmp(argv[1], "arc_facts")) return check_arc_facts();
  if (argc > 1 && !std::strcmp(argv[1], "tropical")) return check_tropical();
  long long n = 0, bad = 0;
  std::vector<uint32_t> codes;
  for (uint32_t f = 16; f < 32; ++f) if (consistent(f)) codes.push_back(f);
  const float finals[3] = {0.0f, 0.5f, 1e-5f};
  for (int len = 0; len <= 6; ++len) {
    std::vector<int> idx(len, 0);
    for (;;) {
      std::vector<wfst_tr> arcs(len);
      uint32_t uni = 0;
      for (int k = 0; k < len; ++k) { arcs[k] = arc_of(codes[idx[k]], (uint32_t)k + 1); uni |= path_arc_facts(arcs[k].ilabel, arcs[k].olabel, arcs[k].weight); }
      for (float fw : finals) {
        const uint64_t a = linear_path_props(true, (uint32_t)len, fw, arcs.data());
        const uint64_t b = linear_path_props_from_facts(true, (uint32_t)len, fw, uni);
        ++n; if (a != b) { if (bad < 5) printf("mismatch len %d uni %u: %llx vs %llx\n", len, uni, (unsigned long long)a, (unsigned long long)b); ++bad; }
      }
      int k = len - 1;
      while (k >= 0 && ++idx[k] == (int)codes.size()) idx[k--] = 0;
      if (k < 0) break;
    }
  }
  printf("%lld cases, %lld mismatches (%zu consistent fact codes)\n", n, bad, codes.size());
  return bad != 0;
}
