// sigma_matcher_tests.cpp — the reference's three sigma-matcher tests (rustfst/src/algorithms/compose/matchers/
// sigma_matcher.rs:486-596), written against wfst.hpp so that they read like the originals:
//   test_sigma_matcher                              "play <sigma> please" answers "play bowie please" like the loop grammar
//   test_sigma_matcher_with_limited_allowed_values  ... radiohead and queen too under {radiohead, queen}; bowie does not
//   test_sigma_matcher_2                            the data files of the reference's test: 4 complete paths
// The originals build ComposeFst with a SigmaMatcher as matcher2 and the sequence filter and call compute(): here that is
// compose_with_config with matcher2_config, SequenceFilter and connect = false.
//
//   g++ -std=c++17 -I include examples/sigma_matcher_tests.cpp -L rustfst_amd/lib -lwfst_amd -Wl,-rpath,$PWD/rustfst_amd/lib -o sigma_tests
//   ./sigma_tests tests/golden        (the directory that holds sigma_matcher_2_{left,right}.fst)
#include <cstdio>
#include <fstream>
#include <iterator>
#include <map>

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

// create_symt :324-334 (<eps> is 0)
enum : Label { SIGMA = 1, PLAY = 2, BOWIE = 3, QUEEN = 4, PLEASE = 5, RADIOHEAD = 6 };

static VectorFst acceptor(const std::vector<Label>& labels) {  // utils::acceptor with W::one()
  VectorFst f;
  f.add_states(labels.size() + 1);
  f.set_start(0);
  for (size_t i = 0; i < labels.size(); ++i) f.add_tr((StateId)i, Tr{labels[i], labels[i], 0.0f, (StateId)(i + 1)});
  f.set_final((StateId)labels.size());
  return f;
}
static VectorFst query_fst(Label artist) { return acceptor({PLAY, artist, PLEASE}); }  // :347-357

static VectorFst grammar_fst_loop() {  // :359-393
  VectorFst fst;
  fst.add_states(4);
  fst.add_tr(0, Tr{PLAY, PLAY, 0.0f, 1});
  fst.add_tr(1, Tr{BOWIE, BOWIE, 0.0f, 2});
  fst.add_tr(1, Tr{QUEEN, QUEEN, 0.0f, 2});
  fst.add_tr(1, Tr{RADIOHEAD, RADIOHEAD, 0.0f, 2});
  fst.add_tr(2, Tr{PLEASE, PLEASE, 0.0f, 3});
  fst.set_start(0);
  fst.set_final(3);
  return fst;
}
static VectorFst grammar_fst_sigma() {  // :421-443
  VectorFst fst;
  fst.add_states(4);
  fst.add_tr(0, Tr{PLAY, PLAY, 0.0f, 1});
  fst.add_tr(1, Tr{SIGMA, SIGMA, 0.0f, 2});
  fst.add_tr(2, Tr{PLEASE, PLEASE, 0.0f, 3});
  fst.set_start(0);
  fst.set_final(3);
  return fst;
}

static ComposeConfig sigma_config(std::optional<std::vector<Label>> allowed) {
  ComposeConfig config{ComposeFilterEnum::SequenceFilter, false};
  config.matcher2_config.sigma_matcher_config = SigmaMatcherConfig{SIGMA, MatcherRewriteMode::MatcherRewriteAuto, std::move(allowed)};
  return config;
}
static VectorFst xp_loop(const VectorFst& q_fst) {  // :395-419
  VectorFst g_fst = grammar_fst_loop();
  tr_sort(g_fst, ILabelCompare{});
  return compose_with_config(q_fst, g_fst, ComposeConfig{ComposeFilterEnum::SequenceFilter, false});
}
static VectorFst xp_sigma(const VectorFst& q_fst, std::optional<std::vector<Label>> allowed) {  // :445-484
  VectorFst g_fst = grammar_fst_sigma();
  tr_sort(g_fst, ILabelCompare{});
  return compose_with_config(q_fst, g_fst, sigma_config(std::move(allowed)));
}

static void test_sigma_matcher() {  // :486-499
  VectorFst q_fst = query_fst(BOWIE);
  tr_sort(q_fst, OLabelCompare{});
  ASSERT(xp_loop(q_fst) == xp_sigma(q_fst, std::nullopt));
}

static void test_sigma_matcher_with_limited_allowed_values() {  // :501-546
  const std::vector<Label> allowed{RADIOHEAD, QUEEN};
  for (Label artist : {RADIOHEAD, QUEEN}) {
    VectorFst q_fst = query_fst(artist);
    tr_sort(q_fst, OLabelCompare{});
    ASSERT(xp_loop(q_fst) == xp_sigma(q_fst, allowed));
  }
  VectorFst q_fst = query_fst(BOWIE);
  tr_sort(q_fst, OLabelCompare{});
  ASSERT(xp_loop(q_fst) != xp_sigma(q_fst, allowed));  // "Bowie should NOT match"
}

static VectorFst read_fst(const std::string& path) {  // VectorFst::read
  std::ifstream in(path, std::ios::binary);
  if (!in) throw Error("cannot open " + path);
  const std::vector<char> bytes((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  detail::DeviceFst d;
  check(wfst_fst_from_openfst_bytes(Context::current().get(), reinterpret_cast<const uint8_t*>(bytes.data()), bytes.size(), &d.h));
  return detail::download(d);
}
static size_t count_paths(const VectorFst& f, StateId s, std::map<StateId, size_t>& memo) {  // string_paths_iter().count(), acyclic
  auto it = memo.find(s);
  if (it != memo.end()) return it->second;
  size_t n = f.is_final(s) ? 1 : 0;
  for (const Tr& t : f.get_trs(s)) n += count_paths(f, t.nextstate, memo);
  return memo[s] = n;
}

static void test_sigma_matcher_2(const std::string& dir) {  // :548-596
  VectorFst left_fst = read_fst(dir + "/sigma_matcher_2_left.fst"), right_fst = read_fst(dir + "/sigma_matcher_2_right.fst");
  tr_sort(left_fst, OLabelCompare{});
  tr_sort(right_fst, ILabelCompare{});
  const VectorFst compose_vec = compose_with_config(left_fst, right_fst, sigma_config(std::nullopt));
  std::map<StateId, size_t> memo;
  ASSERT(compose_vec.start().has_value() && count_paths(compose_vec, *compose_vec.start(), memo) == 4);
  ASSERT(compose_vec.num_states() == 15);
}

static void test_errors() {
  VectorFst q_fst = query_fst(BOWIE), g_fst = grammar_fst_sigma();
  tr_sort(q_fst, OLabelCompare{});
  tr_sort(g_fst, ILabelCompare{});
  ComposeConfig config = sigma_config(std::nullopt);
  config.compose_filter = ComposeFilterEnum::AutoFilter;  // compose_static.rs:186-191
  try {
    compose_with_config(q_fst, g_fst, config);
    ASSERT(false);
  } catch (const Error& e) {
    ASSERT(std::string(e.what()) == "Custom MatcherConfig not supported with AutoFilter");
  }
  ASSERT(xp_loop(q_fst) == xp_sigma(q_fst, std::nullopt));  // the context works on
}

int main(int argc, char** argv) {
  try {
    test_sigma_matcher();
    test_sigma_matcher_with_limited_allowed_values();
    if (argc > 1) test_sigma_matcher_2(argv[1]);
    test_errors();
  } catch (const std::exception& e) {
    std::printf("exception: %s\n", e.what());
    return 1;
  }
  if (failures) return 1;
  std::printf(argc > 1 ? "all sigma-matcher tests passed\n" : "sigma-matcher tests passed (without the data files of test_sigma_matcher_2)\n");
  return 0;
}
