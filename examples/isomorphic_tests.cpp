// isomorphic_tests.cpp — the reference's own tests of isomorphic and invert, written against wfst.hpp so that they read like
// the originals (on tropical weights, the semiring of this library):
//   rustfst/src/algorithms/isomorphic.rs:224-238                     test_isomorphic_1
//   rustfst/src/algorithms/isomorphic.rs:240-255                     test_isomorphic_2
//   rustfst-python/tests/algorithms/test_inversion.py:4-49           test_invert
//   the order-dependent verdicts of isomorphic.rs:134-158: not symmetric, the error and the context after it
//
//   g++ -std=c++17 -I include examples/isomorphic_tests.cpp -L rustfst_amd/lib -lwfst_amd -Wl,-rpath,$PWD/rustfst_amd/lib -o isomorphic_tests
#include <cstdio>
#include <string>

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

// "0\t1\t12\t25\n1\n"
static VectorFst one_arc(StateId from, StateId to) {
  VectorFst fst;
  fst.add_state();
  fst.add_state();
  fst.set_start(from);
  fst.set_final(to);
  fst.add_tr(from, tr(12, 25, 0.0f, to));
  return fst;
}

static void test_isomorphic_1() {
  const VectorFst fst_1 = one_arc(0, 1);
  VectorFst fst_2 = fst_1;
  ASSERT(isomorphic(fst_1, fst_2));
  fst_2.add_tr(0, tr(33, 45, 0.3f, 1));
  ASSERT(!isomorphic(fst_1, fst_2));
}

static void test_isomorphic_2() {
  const VectorFst fst_1 = one_arc(0, 1), fst_2 = one_arc(1, 0);
  ASSERT(isomorphic(fst_1, fst_2));
  ASSERT(isomorphic_with_config(fst_1, fst_2, IsomorphicConfig(0.0f)));
}

static void test_invert() {
  VectorFst fst1;
  StateId s1 = fst1.add_state(), s2 = fst1.add_state(), s3 = fst1.add_state();
  fst1.set_start(s1);
  fst1.set_final(s3, 1.0f);
  fst1.add_tr(s1, tr(1, 2, 1.0f, s2));
  fst1.add_tr(s1, tr(3, 4, 2.0f, s2));
  fst1.add_tr(s2, tr(5, 6, 1.5f, s2));
  fst1.add_tr(s2, tr(3, 5, 1.0f, s3));
  const VectorFst original = fst1;
  invert(fst1);

  VectorFst expected_fst;
  s1 = expected_fst.add_state(), s2 = expected_fst.add_state(), s3 = expected_fst.add_state();
  expected_fst.set_start(s1);
  expected_fst.set_final(s3, 1.0f);
  expected_fst.add_tr(s1, tr(2, 1, 1.0f, s2));
  expected_fst.add_tr(s1, tr(4, 3, 2.0f, s2));
  expected_fst.add_tr(s2, tr(6, 5, 1.5f, s2));
  expected_fst.add_tr(s2, tr(5, 3, 1.0f, s3));
  ASSERT(expected_fst == fst1);
  ASSERT(isomorphic(expected_fst, fst1));
  ASSERT(!isomorphic(original, fst1));
  invert(fst1);
  ASSERT(original == fst1);
}

// fst1 = 0 -a-> 1, 0 -b-> 2, both targets final; fst2 = 0 -a-> 1, 0 -b-> 1: only states of fst1 are recorded as paired
static void test_not_symmetric() {
  VectorFst fst1, fst2;
  for (int k = 0; k < 3; ++k) fst1.add_state();
  fst1.set_start(0);
  fst1.set_final(1);
  fst1.set_final(2);
  fst1.add_tr(0, tr(1, 1, 0.0f, 1));
  fst1.add_tr(0, tr(2, 2, 0.0f, 2));
  for (int k = 0; k < 2; ++k) fst2.add_state();
  fst2.set_start(0);
  fst2.set_final(1);
  fst2.add_tr(0, tr(1, 1, 0.0f, 1));
  fst2.add_tr(0, tr(2, 2, 0.0f, 1));
  ASSERT(isomorphic(fst1, fst2));
  ASSERT(!isomorphic(fst2, fst1));
}

// a mark in front of the failure of the same state: the reference's error, and the context works on
static void test_non_determinism() {
  VectorFst fst1, fst2;
  for (int k = 0; k < 3; ++k) fst1.add_state(), fst2.add_state();
  fst1.set_start(0), fst2.set_start(0);
  fst1.set_final(1), fst1.set_final(2), fst2.set_final(1), fst2.set_final(2);
  for (VectorFst* f : {&fst1, &fst2}) {
    f->add_tr(0, tr(1, 1, 0.0f, 1));
    f->add_tr(0, tr(1, 1, 0.0f, 2));
  }
  fst1.add_tr(0, tr(2, 2, 0.0f, 1));
  fst2.add_tr(0, tr(2, 2, 0.0f, 2));  // state 1 of fst1 is already paired with state 1
  try {
    isomorphic(fst1, fst2);
    ASSERT(false);
  } catch (const Error& e) {
    ASSERT(std::string(e.what()) == "Isomorphic: Non-determinism as an unweighted automaton. state1 = 0 state2 = 0");
  }
  ASSERT(isomorphic(fst1, fst1));
}

int main() {
  try {
    test_isomorphic_1();
    test_isomorphic_2();
    test_invert();
    test_not_symmetric();
    test_non_determinism();
  } catch (const std::exception& e) {
    std::printf("exception: %s\n", e.what());
    return 1;
  }
  if (failures) return 1;
  std::printf("all isomorphic tests passed\n");
  return 0;
}
