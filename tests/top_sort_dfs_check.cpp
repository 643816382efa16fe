#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
// Test program (tests/test_top_sort_batch.py): the search of top_sort_dfs.h, which top_sort_batch_kernel runs on arrays in
// LDS, on heap arrays of exactly the documented sizes — next[E], off[n + 1], rank[n], stack[n] — so that a step outside
// one of them is the sanitizer's to report.  Built with g++ -fsanitize=address,undefined -I<repo>/rustfst_amd/csrc.
// stdin: the number of cases, then per case n, start, the n + 1 offsets and the offsets[n] nextstates.
// argv[1] (optional): the step bound in place of 2 * n + E + 2.
// stdout, one line per case: the search's return code (0 acyclic, 1 cyclic, 2 step bound passed), then for 0 the order and
// for 1 the identity, as the kernel takes it.
#include "top_sort_dfs.h"

static bool read_u32(uint32_t* v) {
  unsigned long long x = 0;
  if (scanf("%llu", &x) != 1) return false;
  *v = (uint32_t)x;
  return true;
}

int main(int argc, char** argv) {
  const long bound = argc > 1 ? atol(argv[1]) : -1;
  uint32_t cases = 0;
  if (!read_u32(&cases)) return 2;
  for (uint32_t c = 0; c < cases; ++c) {
    uint32_t n = 0, start = 0;
    if (!read_u32(&n) || !read_u32(&start) || n == 0 || n >= wfst::TSD_GREY || start >= n) return 2;
    std::unique_ptr<uint16_t[]> off(new uint16_t[n + 1]), rank(new uint16_t[n]), stack(new uint16_t[n]);
    for (uint32_t s = 0; s <= n; ++s) {
      uint32_t o = 0;
      if (!read_u32(&o) || o > 0xFFFFu || (s && o < off[s - 1]) || (!s && o)) return 2;
      off[s] = (uint16_t)o;
    }
    const uint32_t E = off[n];
    std::unique_ptr<uint16_t[]> next(new uint16_t[E]);
    for (uint32_t i = 0; i < E; ++i) {
      uint32_t t = 0;
      if (!read_u32(&t) || t >= n) return 2;
      next[i] = (uint16_t)t;
    }
    for (uint32_t s = 0; s < n; ++s) rank[s] = wfst::TSD_WHITE;
    const uint32_t max_steps = bound >= 0 ? (uint32_t)bound : wfst::top_sort_dfs_max_steps(n, E);
    const uint32_t code = wfst::top_sort_dfs(next.get(), off.get(), n, start, rank.get(), stack.get(), max_steps);
    printf("%u", code);
    if (code != wfst::TSD_STEPS)
      for (uint32_t s = 0; s < n; ++s) printf(" %u", code == wfst::TSD_CYCLIC ? s : (uint32_t)rank[s]);
    printf("\n");
  }
  return 0;
}
