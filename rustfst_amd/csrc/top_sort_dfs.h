// top_sort_dfs.h — the reference's depth-first search with TopOrderVisitor (rustfst dfs_visit.rs:97-187, top_sort.rs:12-61)
// on 16-bit arrays, written out as the sequential walk it is: for host and device code alike.  top_sort_batch_kernel
// (top_sort.hip) runs it in one lane on arrays in LDS; tests/top_sort_dfs_check.cpp runs it on vectors of exactly these sizes.
// No HIP here.
//   next[E]       nextstate of every arc, rows one after the other
//   off[n + 1]    row s = next[off[s], off[s + 1])
//   rank[n]       colour and result in one word: TSD_WHITE everywhere on entry; TSD_GREY while the state is on the stack;
//                 a finished state holds n - 1 - (its finishing rank), which on TSD_ACYCLIC is order[s], the new id of s
//   stack[n]      arc cursors only: entry d is the position (in next) of the tree arc from the state at depth d to the one at
//                 depth d + 1, so the state at depth d > 0 is next[stack[d - 1]] and the one at depth 0 is the root; the
//                 cursor of the state on top lives in a register.  At most n - 1 entries are in use.
// n <= 65534 (the two sentinels), E <= 65535.  Roots: `start`, then the white states in id order; arcs in stored order.
// The first grey target ends the search (TSD_CYCLIC; rank is then of no use: the caller's order is the identity).
// Every step pushes a white state, advances a cursor over a black target or pops, so an acyclic input ends within
// 2 * n + E steps; beyond `max_steps` the search gives up with TSD_STEPS instead of trusting its input to let it end.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define WFST_TSD_HD __host__ __device__
#else
#define WFST_TSD_HD
#endif

namespace wfst {

constexpr uint16_t TSD_WHITE = 0xFFFFu, TSD_GREY = 0xFFFEu;
enum : uint32_t { TSD_ACYCLIC = 0, TSD_CYCLIC = 1, TSD_STEPS = 2 };  // what top_sort_dfs returns

constexpr uint32_t top_sort_dfs_max_steps(uint32_t n, uint32_t E) { return 2u * n + E + 2u; }

WFST_TSD_HD inline uint32_t top_sort_dfs(const uint16_t* next, const uint16_t* off, uint32_t n, uint32_t start, uint16_t* rank,
                                         uint16_t* stack, uint32_t max_steps) {
  uint32_t finished = 0, steps = 0;
  for (uint32_t root = start; root < n;) {
    uint32_t depth = 0, s = root, cur = off[s], end = off[s + 1];
    rank[s] = TSD_GREY;
    ++steps;
    for (;;) {
      if (steps > max_steps) return TSD_STEPS;
      ++steps;
      if (cur < end) {
        const uint32_t t = next[cur];
        const uint16_t colour = rank[t];
        if (colour == TSD_WHITE) {  // tree arc: the cursor stays on it until t is finished
          stack[depth++] = (uint16_t)cur;
          s = t;
          rank[s] = TSD_GREY;
          cur = off[s];
          end = off[s + 1];
        } else if (colour == TSD_GREY) {  // back arc
          return TSD_CYCLIC;
        } else {  // forward or cross arc
          ++cur;
        }
        continue;
      }
      rank[s] = (uint16_t)(n - 1u - finished);  // finish_state
      ++finished;
      if (depth == 0) break;
      --depth;
      cur = (uint32_t)stack[depth] + 1u;
      s = depth ? next[stack[depth - 1u]] : root;
      end = off[s + 1];
    }
    root = root == start ? 0u : root + 1u;
    while (root < n && rank[root] != TSD_WHITE) ++root;
  }
  return TSD_ACYCLIC;
}

}  // namespace wfst
