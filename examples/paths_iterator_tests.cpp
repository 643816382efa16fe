// paths_iterator_tests.cpp — the reference's own tests of paths_iter, written against wfst.hpp so that they read like the
// originals.  They are written for IntegerWeight there; here on tropical weights, the semiring of this library, so the
// products of the expected weights become sums:
//   rustfst/src/fst_traits/paths_iterator.rs:77-82     test_paths_iterator_empty_fst
//   rustfst/src/fst_traits/paths_iterator.rs:84-98     test_paths_iterator_single_state_start_and_final
//   rustfst/src/fst_traits/paths_iterator.rs:100-114   test_paths_iterator_linear_fst
//   rustfst/src/fst_traits/paths_iterator.rs:116-161   test_paths_iterator_small_fst_one_final_state
//   rustfst/src/fst_traits/paths_iterator.rs:163-218   test_paths_iterator_small_fst_multiple_final_states
// The originals compare multisets; the iterator's order — (number of arcs, arc positions) — is asserted here as well.
//
//   g++ -std=c++17 -I include examples/paths_iterator_tests.cpp -L rustfst_amd/lib -lwfst_amd -Wl,-rpath,$PWD/rustfst_amd/lib -o paths_iterator_tests
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "wfst.hpp"

using namespace wfst_amd;

static int failures = 0;
#define ASSERT(cond)                                                      \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::printf("ASSERT FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                         \
    }                                                                     \
  } while (0)

static Tr tr(Label il, Label ol, float w, StateId ns) { return Tr{il, ol, w, ns}; }
static FstPath path(std::vector<Label> labels, float w) { return FstPath{labels, labels, w}; }
// Counter equality of the originals: the same paths with the same multiplicities
static bool same_multiset(std::vector<FstPath> a, std::vector<FstPath> b) {
  if (a.size() != b.size()) return false;
  for (const FstPath& p : a) {
    auto it = std::find(b.begin(), b.end(), p);
    if (it == b.end()) return false;
    b.erase(it);
  }
  return true;
}

static void test_paths_iterator_empty_fst() {
  VectorFst fst;
  ASSERT(fst.paths_iter().size() == 0);
}

static void test_paths_iterator_single_state_start_and_final() {
  VectorFst fst;
  const StateId s = fst.add_state();
  fst.set_start(s);
  fst.set_final(s);  // one()
  ASSERT(same_multiset(fst.paths_iter(), {FstPath{}}));
}

static void test_paths_iterator_linear_fst() {
  const std::vector<Label> labels{153, 45, 96};
  VectorFst fst;  // utils::acceptor(&labels, one())
  StateId cur = fst.add_state();
  fst.set_start(cur);
  for (Label l : labels) {
    const StateId nxt = fst.add_state();
    fst.add_tr(cur, tr(l, l, 0.0f, nxt));
    cur = nxt;
  }
  fst.set_final(cur);
  const std::vector<FstPath> paths = fst.paths_iter();
  ASSERT(paths.size() == 1);
  for (const FstPath& p : paths) ASSERT(p == path(labels, 0.0f));
}

static VectorFst small_fst() {
  VectorFst fst;
  const StateId s1 = fst.add_state(), s2 = fst.add_state(), s3 = fst.add_state(), s4 = fst.add_state();
  fst.set_start(s1);
  fst.add_tr(s1, tr(1, 1, 1.0f, s2));
  fst.add_tr(s1, tr(2, 2, 2.0f, s3));
  fst.add_tr(s1, tr(3, 3, 3.0f, s4));
  fst.add_tr(s2, tr(4, 4, 4.0f, s4));
  fst.add_tr(s3, tr(5, 5, 5.0f, s4));
  return fst;
}

static void test_paths_iterator_small_fst_one_final_state() {
  VectorFst fst = small_fst();
  fst.set_final(3, 18.0f);
  const std::vector<FstPath> paths = fst.paths_iter();
  ASSERT(paths.size() == 3);
  const std::vector<FstPath> paths_ref{path({1, 4}, 1.0f + 4.0f + 18.0f), path({2, 5}, 2.0f + 5.0f + 18.0f), path({3}, 3.0f + 18.0f)};
  ASSERT(same_multiset(paths, paths_ref));
  const std::vector<FstPath> in_order{paths_ref[2], paths_ref[0], paths_ref[1]};
  ASSERT(paths == in_order);
}

static void test_paths_iterator_small_fst_multiple_final_states() {
  VectorFst fst = small_fst();
  fst.set_final(0, 38.0f);
  fst.set_final(1, 41.0f);
  fst.set_final(2, 53.0f);
  fst.set_final(3, 185.0f);
  const std::vector<FstPath> paths = fst.paths_iter();
  ASSERT(paths.size() == 6);
  const std::vector<FstPath> paths_ref{path({}, 38.0f),
                                       path({1}, 1.0f + 41.0f),
                                       path({2}, 2.0f + 53.0f),
                                       path({1, 4}, 1.0f + 4.0f + 185.0f),
                                       path({2, 5}, 2.0f + 5.0f + 185.0f),
                                       path({3}, 3.0f + 185.0f)};
  ASSERT(same_multiset(paths, paths_ref));
  const std::vector<FstPath> in_order{paths_ref[0], paths_ref[1], paths_ref[2], paths_ref[5], paths_ref[3], paths_ref[4]};
  ASSERT(paths == in_order);
}

// what the reference cannot return from: a cycle the start state reaches; and the bound on the table
static void test_errors() {
  VectorFst fst = small_fst();
  fst.set_final(3);
  try {
    fst.paths_iter(2);
    ASSERT(false);
  } catch (const Error& e) {
    ASSERT(std::string(e.what()).find("has 3 paths, more than max_paths") != std::string::npos);
  }
  fst.add_tr(3, tr(9, 9, 0.0f, 0));
  try {
    fst.paths_iter();
    ASSERT(false);
  } catch (const Error& e) {
    ASSERT(std::string(e.what()).find("cycle is accessible from the start state") != std::string::npos);
  }
}

int main() {
  try {
    test_paths_iterator_empty_fst();
    test_paths_iterator_single_state_start_and_final();
    test_paths_iterator_linear_fst();
    test_paths_iterator_small_fst_one_final_state();
    test_paths_iterator_small_fst_multiple_final_states();
    test_errors();
  } catch (const std::exception& e) {
    std::printf("exception: %s\n", e.what());
    return 1;
  }
  if (failures) return 1;
  std::printf("all paths_iterator tests passed\n");
  return 0;
}
