#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
// Test program (tests/test_string_placement.py): string_placement.h against the rule as its issue states it, written out
// here a second time as a table of thresholds, at the edges of every line of the rule; and for every case the two bounds no
// launch may break: wpb * 16 * maxs <= 64 KB of LDS, and ceil(n / wpb) workgroups of wpb waves hold all n strings.
// Without arguments: the sweep ("<cases> cases, <bad> mismatches").  With `n maxs n_cus hint forced_text`: one line
// "wpb workgroups packed_for_resident forced" — what the GPU tests compare Context.string_placement() with.
// Built with g++ -fsanitize=address,undefined -I<repo>/rustfst_amd/csrc.
#include "string_placement.h"

// the issue's rule, step by step
static uint32_t expected_wpb(uint64_t n, uint32_t maxs, uint32_t n_cus, bool hint, uint32_t forced, bool* packed, bool* was_forced) {
  const uint32_t cap = (64u * 1024u) / (16u * maxs);  // 8, 4, 2
  *packed = *was_forced = false;
  if (forced == 1 || forced == 2 || forced == 4 || forced == 8) {
    *was_forced = true;
    return forced < cap ? forced : cap;
  }
  if (n < 16) return 1;
  if (hint) {
    *packed = true;
    return cap;
  }
  const uint32_t ws[4] = {1, 2, 4, 8};
  for (uint32_t w : ws) {
    if (w >= cap) return cap;
    if ((n + w - 1) / w <= n_cus) return w;
  }
  return cap;
}

int main(int argc, char** argv) {
  if (argc == 6) {
    const wfst::StringPlacement p = wfst::string_placement(std::strtoull(argv[1], nullptr, 10), (uint32_t)std::atoi(argv[2]), (uint32_t)std::atoi(argv[3]),
                                                           std::atoi(argv[4]) != 0, wfst::string_forced_wpb(argv[5]));
    printf("%u %u %d %d\n", p.wpb, p.workgroups, p.packed_for_resident ? 1 : 0, p.forced ? 1 : 0);
    return 0;
  }
  long long cases = 0, bad = 0;
  auto expect = [&](bool ok, const char* what, uint64_t n, uint32_t maxs, uint32_t cus, int hint, const char* forced) {
    ++cases;
    if (!ok) {
      if (bad < 10) printf("n %llu maxs %u n_cus %u hint %d forced '%s': %s\n", (unsigned long long)n, maxs, cus, hint, forced, what);
      ++bad;
    }
  };
  // the knob's text -> the forced value: other numbers go to the next lower power of two, 0 and non-numbers are ignored
  struct Knob {
    const char* text;
    uint32_t value;
  };
  const Knob knobs[] = {{nullptr, 0}, {"", 0},   {"0", 0},  {"1", 1},  {"2", 2},   {"3", 2},    {"4", 4},        {"5", 4},
                        {"7", 4},     {"8", 8},  {"9", 8},  {"64", 8}, {"x", 0},   {"-1", 0},   {"99999999999999999999", 8}, {"08", 8}};
  for (const Knob& k : knobs) expect(wfst::string_forced_wpb(k.text) == k.value, "string_forced_wpb", 0, 0, 0, 0, k.text ? k.text : "(null)");
  const uint32_t cus_set[4] = {1, 4, 256, 304}, slices[3] = {512, 1024, 2048};
  const char* forced_set[7] = {"0", "1", "2", "3", "4", "8", "9"};
  const uint32_t forced_val[7] = {0, 1, 2, 2, 4, 8, 8};
  for (uint32_t cus : cus_set) {
    const uint64_t ns[] = {1, 15, 16, 17, cus, cus + 1ull, 2ull * cus, 2ull * cus + 1, 4ull * cus, 4ull * cus + 1, 8ull * cus, 8ull * cus + 1, 4096, 1ull << 20};
    for (uint64_t n : ns)
      for (uint32_t maxs : slices)
        for (int hint = 0; hint < 2; ++hint)
          for (int f = 0; f < 7; ++f) {
            const wfst::StringPlacement p = wfst::string_placement(n, maxs, cus, hint != 0, wfst::string_forced_wpb(forced_set[f]));
            bool packed = false, was_forced = false;
            const uint32_t want = expected_wpb(n, maxs, cus, hint != 0, forced_val[f], &packed, &was_forced);
            expect(p.wpb == want, "waves per workgroup", n, maxs, cus, hint, forced_set[f]);
            expect(p.packed_for_resident == packed && p.forced == was_forced, "which line decided", n, maxs, cus, hint, forced_set[f]);
            expect(p.wpb == 1 || p.wpb == 2 || p.wpb == 4 || p.wpb == 8, "not 1, 2, 4 or 8", n, maxs, cus, hint, forced_set[f]);
            expect((uint64_t)p.wpb * 16u * maxs <= 64u * 1024u, "more LDS than a workgroup has", n, maxs, cus, hint, forced_set[f]);
            expect(p.workgroups == (n + p.wpb - 1) / p.wpb && (uint64_t)p.workgroups * p.wpb >= n, "the grid does not hold the batch", n, maxs,
                   cus, hint, forced_set[f]);
          }
  }
  // the thresholds in numbers, at 256 compute units and the 512-state slice: 1 up to 256 strings, 2 up to 512, 4 up to 1024, 8 above
  const uint64_t at[8] = {16, 256, 257, 512, 513, 1024, 1025, 4096};
  const uint32_t w256[8] = {1, 1, 2, 2, 4, 4, 8, 8};
  for (int k = 0; k < 8; ++k) expect(wfst::string_placement(at[k], 512, 256, false, 0).wpb == w256[k], "the table at 256 CUs", at[k], 512, 256, 0, "0");
  printf("%lld cases, %lld mismatches\n", cases, bad);
  return bad != 0;
}
