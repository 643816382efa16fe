// sigma_batch_tests.cpp — "play <sigma> please" (rustfst/src/algorithms/compose/matchers/sigma_matcher.rs:486-546) for three
// utterances in ONE call: compose_shortest_path_batch with a SigmaMatcher on the grammar equals, utterance by utterance, the
// loop of compose_with_config + shortest_path the reference's caller writes.  Written against wfst.hpp like
// examples/sigma_matcher_tests.cpp.
//
//   g++ -std=c++17 -I include examples/sigma_batch_tests.cpp -L rustfst_amd/lib -lwfst_amd -Wl,-rpath,$PWD/rustfst_amd/lib -o sigma_batch
//   ./sigma_batch
#include <cstdio>

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

enum : Label { SIGMA = 1, PLAY = 2, BOWIE = 3, QUEEN = 4, PLEASE = 5, RADIOHEAD = 6 };  // create_symt :324-334

static VectorFst query_fst(Label artist) {  // :347-357, utils::acceptor with W::one()
  const Label labels[3] = {PLAY, artist, PLEASE};
  VectorFst f;
  f.add_states(4);
  f.set_start(0);
  for (StateId i = 0; i < 3; ++i) f.add_tr(i, Tr{labels[i], labels[i], 0.0f, i + 1});
  f.set_final(3);
  tr_sort(f, OLabelCompare{});
  return f;
}
static VectorFst grammar_fst_sigma() {  // :421-443
  VectorFst fst;
  fst.add_states(4);
  fst.add_tr(0, Tr{PLAY, PLAY, 0.0f, 1});
  fst.add_tr(1, Tr{SIGMA, SIGMA, 0.0f, 2});
  fst.add_tr(2, Tr{PLEASE, PLEASE, 0.0f, 3});
  fst.set_start(0);
  fst.set_final(3);
  tr_sort(fst, ILabelCompare{});
  return fst;
}
static ComposeConfig sigma_config(std::optional<std::vector<Label>> allowed) {
  ComposeConfig config{ComposeFilterEnum::SequenceFilter, true};
  config.matcher2_config.sigma_matcher_config = SigmaMatcherConfig{SIGMA, MatcherRewriteMode::MatcherRewriteAuto, std::move(allowed)};
  return config;
}

static void test_batch_equals_the_loop(std::optional<std::vector<Label>> allowed, size_t expected_paths) {
  const std::vector<VectorFst> utterances{query_fst(BOWIE), query_fst(RADIOHEAD), query_fst(QUEEN)};
  const VectorFst g_fst = grammar_fst_sigma();
  const ComposeConfig config = sigma_config(std::move(allowed));
  const std::vector<VectorFst> paths = compose_shortest_path_batch(utterances, g_fst, config);
  ASSERT(paths.size() == 3);
  size_t found = 0;
  for (size_t i = 0; i < paths.size(); ++i) {
    ASSERT(paths[i] == shortest_path(compose_with_config(utterances[i], g_fst, config)));
    found += paths[i].num_states() == 4 ? 1 : 0;  // the utterance itself: three arcs
  }
  ASSERT(found == expected_paths);
}

static void test_errors() {
  const std::vector<VectorFst> utterances{query_fst(BOWIE), query_fst(SIGMA)};  // the second one says sigma itself
  try {
    compose_shortest_path_batch(utterances, grammar_fst_sigma(), sigma_config(std::nullopt));
    ASSERT(false);
  } catch (const Error& e) {
    ASSERT(std::string(e.what()) == "SigmaMatcher::Find: bad label (sigma)");  // sigma_matcher.rs:199-201
  }
  test_batch_equals_the_loop(std::nullopt, 3);  // the context works on
}

int main() {
  try {
    test_batch_equals_the_loop(std::nullopt, 3);
    test_batch_equals_the_loop(std::vector<Label>{RADIOHEAD, QUEEN}, 2);  // "Bowie should NOT match" :501-546
    test_errors();
  } catch (const std::exception& e) {
    std::printf("exception: %s\n", e.what());
    return 1;
  }
  if (failures) return 1;
  std::printf("all sigma-batch tests passed\n");
  return 0;
}
