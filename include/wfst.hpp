// wfst.hpp — header-only C++17 mirror of the part of rustfst's Rust interface that sits on the compose -> shortest-path
// path, over the C-ABI of wfst.h.  Same names, argument meaning and error behaviour as the reference, so that host code
// (and tests) read like rustfst's own:
//
//   rustfst                                                     here (namespace wfst_amd)
//   ----------------------------------------------------------  -------------------------------------------------
//   Tr::new(ilabel, olabel, weight, nextstate)      tr.rs:6-15   Tr{ilabel, olabel, weight, nextstate} (== wfst_tr)
//   VectorFst::<TropicalWeight>::new()                           VectorFst()
//   MutableFst::{add_state, add_states, set_start, set_final,    same member names (fst_traits/mutable_fst.rs)
//               add_tr, delete_final_weight}
//   CoreFst::{start, final_weight, num_trs, get_trs},            same member names (fst_traits/fst.rs:18-250);
//   ExpandedFst::num_states, Fst::properties                     Option<T> -> std::optional<T>
//   tr_sort(&mut fst, ILabelCompare{} | OLabelCompare{})         tr_sort(fst, ILabelCompare{} | OLabelCompare{})
//   project(&mut fst, ProjectType::ProjectInput)                 project(fst, ProjectType::ProjectInput)
//   invert(&mut fst)                                             invert(fst)                                       inversion.rs:32-48
//   isomorphic(&a, &b) / isomorphic_with_config(&a, &b, config)  isomorphic(a, b) / isomorphic_with_config(a, b, config)  isomorphic.rs:184-212
//   fst.paths_iter() -> impl Iterator<Item = FstPath<W>>         fst.paths_iter() -> std::vector<FstPath>          paths_iterator.rs:24-62
//   connect(&mut fst) / rm_epsilon(&mut fst)                     connect(fst) / rm_epsilon(fst)
//   shortest_distance(&fst, reverse) -> Vec<W>                   shortest_distance(fst, reverse) -> std::vector<float>
//   reweight(&mut fst, &potentials, ReweightType::..)            reweight(fst, potentials, ReweightType::..)       reweight.rs
//   push_weights(&mut fst, ..) / push_weights_with_config(..)    push_weights(..) / push_weights_with_config(..)  push.rs:76-118
//   determinize(&fst) / determinize_with_config(&fst, config)    determinize(fst) / determinize_with_config(..)   determinize_static.rs:149-190
//   determinize_with_distance(&fst, &in_dist, delta)             determinize_with_distance(fst, in_dist, delta)   determinize_static.rs:24-39
//   (many acceptors in one call)                                 determinize_batch / determinize_with_distance_batch
//                                                                minimize_batch, rm_epsilon_batch, tr_sum_batch,
//                                                                tr_unique_batch, optimize_batch, top_sort_batch
//   minimize(&mut fst) / minimize_with_config(&mut fst, config)  minimize(fst) / minimize_with_config(fst, config)  minimize.rs:77-176
//   tr_sum(&mut fst) / tr_unique(&mut fst)                       tr_sum(fst) / tr_unique(fst)                      tr_sum.rs, tr_unique.rs
//   optimize(&mut fst)                                           optimize(fst)                                     optimize.rs:11-128
//   top_sort(&mut fst) / state_sort(&mut fst, &order)            top_sort(fst) / state_sort(fst, order)            top_sort.rs, state_sort.rs
//   union(&mut a, &b) / concat(&mut a, &b)                       union_(a, b) / concat(a, b)                       union_static.rs:55-118, concat_static.rs:53-109
//   closure(&mut fst, ClosureType)                               closure(fst, ClosureType)                         closure_static.rs:25-73
//   (rustfst-python union_list / concat_list)                    union_list(fsts) / concat_list(fsts)
//   replace(fst_list, root, epsilon_on_replace)                  replace(fst_list, root, epsilon_on_replace)       replace/replace_static.rs:44-58
//   (look-ahead recipe of rustfst-cli/src/cmds/compose.rs)       LookAheadFst(fst1).compose(fst2) / compose_lookahead
//   compose(fst1, fst2) / compose_with_config(.., ComposeConfig) compose(..) / compose_with_config(..)   compose_static.rs:166-306
//   MatcherConfig { sigma_matcher_config: Some(SigmaMatcherConfig) } ComposeConfig::matcher1_config / matcher2_config  compose_static.rs:30-54
//   (a loop of compose_with_config over many pairs)              compose_batch(fst1s, fst2s, config)
//   shortest_path(&fst) / shortest_path_with_config(..)          shortest_path(..) / shortest_path_with_config(..)  shortest_path.rs:76-133
//   (a loop of the two over many acceptors)                      compose_shortest_path_batch(acceptors, t, config)
//   anyhow::Result<T> Err(e)                                     throws wfst_amd::Error (what() = the library's message)
//
// The algorithms run on the GPU through a per-thread Context; a VectorFst lives on the host (wfst_vec_fst) and is
// flattened / rebuilt around each call exactly as the Rust shim of INTEGRATION.md does.
#ifndef WFST_AMD_HPP
#define WFST_AMD_HPP

#include <cmath>
#include <cstdint>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "wfst.h"

namespace wfst_amd {

struct Error : std::runtime_error {
  using std::runtime_error::runtime_error;
};

inline void check(wfst_status st) {  // check_ffi_error (rustfst-python/rustfst/ffi_utils.py)
  if (st == WFST_OK) return;
  char* msg = nullptr;
  std::string text = "unknown error";
  if (wfst_last_error(&msg) == WFST_OK && msg) {
    text = msg;
    wfst_string_destroy(msg);
  }
  throw Error(text);
}

using Tr = wfst_tr;
using StateId = uint32_t;
using Label = uint32_t;
constexpr Label EPS_LABEL = 0;

enum class ComposeFilterEnum : uint32_t {  // compose_static.rs:19-33
  AutoFilter = 0, NullFilter = 1, TrivialFilter = 2, SequenceFilter = 3, AltSequenceFilter = 4, MatchFilter = 5, NoMatchFilter = 6
};
enum class MatcherRewriteMode : uint32_t { MatcherRewriteAuto = 0, MatcherRewriteAlways = 1, MatcherRewriteNever = 2 };  // matchers/mod.rs
struct SigmaMatcherConfig {  // compose_static.rs:30-35
  Label sigma_label = 0;
  MatcherRewriteMode rewrite_mode = MatcherRewriteMode::MatcherRewriteAuto;
  std::optional<std::vector<Label>> sigma_allowed_matches = std::nullopt;
};
struct MatcherConfig {  // compose_static.rs:37-46
  std::optional<SigmaMatcherConfig> sigma_matcher_config = std::nullopt;
  bool empty() const { return !sigma_matcher_config.has_value(); }
};
struct ComposeConfig {  // compose_static.rs:48-65 (default: AutoFilter, connect = true, no matcher configs); the matcher configs
  ComposeFilterEnum compose_filter = ComposeFilterEnum::AutoFilter;  // come last here, so that {filter, connect} still initialises
  bool connect = true;
  MatcherConfig matcher1_config = {};
  MatcherConfig matcher2_config = {};
};
struct ShortestPathConfig {  // shortest_path.rs:26-74 (default: delta 1e-6, nshortest 1, unique false)
  float delta = 1e-6f;
  size_t nshortest = 1;
  bool unique = false;
  ShortestPathConfig with_nshortest(size_t n) const { ShortestPathConfig c = *this; c.nshortest = n; return c; }
  ShortestPathConfig with_unique(bool u) const { ShortestPathConfig c = *this; c.unique = u; return c; }
};
struct ILabelCompare {};
struct OLabelCompare {};

class Context {  // one per (thread, GPU)
 public:
  explicit Context(int device = 0) { check(wfst_ctx_create(device, &h_)); }
  ~Context() { if (h_) wfst_ctx_destroy(h_); }
  Context(const Context&) = delete;
  Context& operator=(const Context&) = delete;
  wfst_ctx* get() const { return h_; }
  static Context& current() {
    static thread_local Context ctx(0);
    return ctx;
  }

 private:
  wfst_ctx* h_ = nullptr;
};

// FstPath (fst_path.rs:13-20): labels with epsilons dropped per tape, and the weight; == is exact
struct FstPath {
  std::vector<Label> ilabels, olabels;
  float weight = 0.0f;  // W::one()
  bool operator==(const FstPath& o) const { return ilabels == o.ilabels && olabels == o.olabels && weight == o.weight; }
};

class VectorFst {
 public:
  VectorFst() { check(wfst_vec_fst_new(&h_)); }
  ~VectorFst() { if (h_) wfst_vec_fst_destroy(h_); }
  VectorFst(const VectorFst& o) { check(wfst_vec_fst_copy(o.h_, &h_)); }
  VectorFst(VectorFst&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  VectorFst& operator=(VectorFst o) noexcept { std::swap(h_, o.h_); return *this; }

  StateId add_state() { StateId s; check(wfst_vec_fst_add_state(h_, &s)); return s; }
  void add_states(size_t n) { for (size_t i = 0; i < n; ++i) add_state(); }
  void set_start(StateId s) { check(wfst_vec_fst_set_start(h_, s)); }
  void set_final(StateId s, float weight = 0.0f) { check(wfst_vec_fst_set_final(h_, s, weight)); }  // W::one() by default
  void delete_final_weight(StateId s) { check(wfst_vec_fst_del_final_weight(h_, s)); }
  void add_tr(StateId s, const Tr& tr) { check(wfst_vec_fst_add_tr(h_, s, &tr)); }

  size_t num_states() const { uint32_t n; check(wfst_vec_fst_num_states(h_, &n)); return n; }
  std::optional<StateId> start() const {
    int64_t s;
    check(wfst_vec_fst_start(h_, &s));
    return s < 0 ? std::nullopt : std::optional<StateId>((StateId)s);
  }
  std::optional<float> final_weight(StateId s) const {
    float w;
    int some;
    check(wfst_vec_fst_final_weight(h_, s, &w, &some));
    return some ? std::optional<float>(w) : std::nullopt;
  }
  bool is_final(StateId s) const { return final_weight(s).has_value(); }
  size_t num_trs(StateId s) const { uint64_t n; check(wfst_vec_fst_num_trs(h_, s, &n)); return (size_t)n; }
  std::vector<Tr> get_trs(StateId s) const {
    uint64_t n = 0;
    check(wfst_vec_fst_num_trs(h_, s, &n));
    std::vector<Tr> out((size_t)n);
    check(wfst_vec_fst_get_trs(h_, s, out.data(), n, &n));
    return out;
  }
  uint64_t properties() const { uint64_t p; check(wfst_vec_fst_properties(h_, &p)); return p; }
  // PartialEq of VectorFst (vector_fst/data_structure.rs:36-41): states, arcs, finals (approximate weights), start
  bool operator==(const VectorFst& o) const { int eq; check(wfst_vec_fst_equals(h_, o.h_, &eq)); return eq != 0; }
  bool operator!=(const VectorFst& o) const { return !(*this == o); }
  // Fst::paths_iter (fst_traits/paths_iterator.rs:24-62): every successful path, in the iterator's order; enumerated on the
  // device (defined below).  Throws when a cycle is accessible from the start state or the FST has more than max_paths paths.
  std::vector<FstPath> paths_iter(uint64_t max_paths = 1u << 20) const;

  wfst_vec_fst* raw() const { return h_; }
  static VectorFst adopt(wfst_vec_fst* h) { VectorFst f(nullptr); f.h_ = h; return f; }

 private:
  explicit VectorFst(std::nullptr_t) {}
  wfst_vec_fst* h_ = nullptr;
};

inline void tr_sort(VectorFst& fst, ILabelCompare) { check(wfst_vec_fst_tr_sort(fst.raw(), 1)); }  // tr_sort.rs:13-62
inline void tr_sort(VectorFst& fst, OLabelCompare) { check(wfst_vec_fst_tr_sort(fst.raw(), 0)); }

namespace detail {
struct DeviceFst {  // owned wfst_fst handle
  wfst_fst* h = nullptr;
  DeviceFst() = default;
  DeviceFst(const DeviceFst&) = delete;
  ~DeviceFst() { if (h) wfst_fst_destroy(h); }
};
inline void upload(const VectorFst& f, DeviceFst& d) { check(wfst_vec_fst_to_device(Context::current().get(), f.raw(), &d.h)); }
inline VectorFst download(const DeviceFst& d) {
  wfst_vec_fst* out = nullptr;
  check(wfst_vec_fst_from_device(d.h, &out));
  return VectorFst::adopt(out);
}
// the two matcher configs of a ComposeConfig in the C-ABI's form (they point into `config`: it must outlive them).  A
// SigmaMatcherConfig goes through the ..._with_matchers calls; Some(empty list) is None there (rustfst-ffi compose.rs:199-211)
struct MatcherPair {
  wfst_matcher_config m[2];
  bool some[2];
  explicit MatcherPair(const ComposeConfig& config) {
    const MatcherConfig* mc[2] = {&config.matcher1_config, &config.matcher2_config};
    for (int i = 0; i < 2; ++i) {
      some[i] = !mc[i]->empty();
      if (!some[i]) continue;
      const SigmaMatcherConfig& sc = *mc[i]->sigma_matcher_config;
      const bool list = sc.sigma_allowed_matches.has_value() && !sc.sigma_allowed_matches->empty();
      m[i] = wfst_matcher_config{sc.sigma_label, (uint32_t)sc.rewrite_mode, list ? sc.sigma_allowed_matches->data() : nullptr,
                                 list ? sc.sigma_allowed_matches->size() : 0};
    }
  }
  const wfst_matcher_config* side(int i) const { return some[i] ? &m[i] : nullptr; }
};
}  // namespace detail

// compose_with_config (compose_static.rs:166-266): Err when neither side is known label-sorted ("... (sort?)")
inline VectorFst compose_with_config(const VectorFst& fst1, const VectorFst& fst2, const ComposeConfig& config) {
  detail::DeviceFst a, b, c;
  detail::upload(fst1, a);
  detail::upload(fst2, b);
  const wfst_compose_config cfg{(uint32_t)config.compose_filter, config.connect ? 1u : 0u};
  const detail::MatcherPair m(config);
  check(wfst_compose_with_matchers(Context::current().get(), a.h, b.h, &cfg, m.side(0), m.side(1), &c.h));
  return detail::download(c);
}
inline VectorFst compose(const VectorFst& fst1, const VectorFst& fst2) {  // compose_static.rs:293-303
  return compose_with_config(fst1, fst2, ComposeConfig{});
}

// for i: compose_with_config(fst1s[i or 0], fst2s[i or 0], config) as ONE call (wfst_compose_batch): equal lengths, or a list
// of one on either side, which serves every item.  Matcher configs are not part of this call.
inline std::vector<VectorFst> compose_batch(const std::vector<VectorFst>& fst1s, const std::vector<VectorFst>& fst2s,
                                            const ComposeConfig& config = ComposeConfig{}) {
  if (!config.matcher1_config.empty() || !config.matcher2_config.empty())
    throw Error("unsupported: a MatcherConfig (sigma matcher) in compose_batch");
  const size_t n1 = fst1s.size(), n2 = fst2s.size(), n = n1 > n2 ? n1 : n2;
  std::vector<detail::DeviceFst> a(n1), b(n2), out(n);
  std::vector<const wfst_fst*> h1(n1), h2(n2);
  std::vector<wfst_fst*> res(n, nullptr);
  for (size_t i = 0; i < n1; ++i) {
    detail::upload(fst1s[i], a[i]);
    h1[i] = a[i].h;
  }
  for (size_t i = 0; i < n2; ++i) {
    detail::upload(fst2s[i], b[i]);
    h2[i] = b[i].h;
  }
  const wfst_compose_config cfg{(uint32_t)config.compose_filter, config.connect ? 1u : 0u};
  check(wfst_compose_batch(Context::current().get(), h1.data(), n1, h2.data(), n2, &cfg, res.data(), nullptr));
  std::vector<VectorFst> fsts;
  for (size_t i = 0; i < n; ++i) {
    out[i].h = res[i];
    fsts.push_back(detail::download(out[i]));
  }
  return fsts;
}

// shortest_path_with_config (shortest_path.rs:107-170)
inline VectorFst shortest_path_with_config(const VectorFst& ifst, const ShortestPathConfig& config) {
  detail::DeviceFst a, c;
  detail::upload(ifst, a);
  const wfst_shortest_path_config cfg{config.delta, (uint64_t)config.nshortest, config.unique ? 1u : 0u};
  check(wfst_shortest_path(Context::current().get(), a.h, &cfg, &c.h));
  return detail::download(c);
}
inline VectorFst shortest_path(const VectorFst& ifst) { return shortest_path_with_config(ifst, ShortestPathConfig{}); }

// for a in acceptors: shortest_path_with_config(compose_with_config(a, t, compose_config), shortest_path_config) as ONE call
// (wfst_compose_shortest_path_batch_with_matchers; without matcher configs that is wfst_compose_shortest_path_batch): strings
// against a sigma matcher on t run one wavefront each in one launch.  nshortest must be 1.
inline std::vector<VectorFst> compose_shortest_path_batch(const std::vector<VectorFst>& acceptors, const VectorFst& t,
                                                          const ComposeConfig& compose_config,
                                                          const ShortestPathConfig& shortest_path_config = ShortestPathConfig{}) {
  const size_t n = acceptors.size();
  if (n == 0) return {};
  std::vector<detail::DeviceFst> a(n), out(n);
  detail::DeviceFst b;
  std::vector<const wfst_fst*> in(n);
  std::vector<wfst_fst*> res(n, nullptr);
  for (size_t i = 0; i < n; ++i) {
    detail::upload(acceptors[i], a[i]);
    in[i] = a[i].h;
  }
  detail::upload(t, b);
  const wfst_compose_config ccfg{(uint32_t)compose_config.compose_filter, compose_config.connect ? 1u : 0u};
  const wfst_shortest_path_config scfg{shortest_path_config.delta, (uint64_t)shortest_path_config.nshortest,
                                       shortest_path_config.unique ? 1u : 0u};
  const detail::MatcherPair m(compose_config);
  check(wfst_compose_shortest_path_batch_with_matchers(Context::current().get(), in.data(), n, b.h, &ccfg, m.side(0), m.side(1), &scfg,
                                                       res.data(), nullptr));
  std::vector<VectorFst> paths;
  for (size_t i = 0; i < n; ++i) {
    out[i].h = res[i];
    paths.push_back(detail::download(out[i]));
  }
  return paths;
}

// project (algorithms/projection.rs:65-95): in place, like the reference
enum class ProjectType { ProjectInput, ProjectOutput };  // projection.rs:7-13
inline void project(VectorFst& fst, ProjectType project_type) {
  detail::DeviceFst a;
  detail::upload(fst, a);
  check(wfst_fst_project(Context::current().get(), a.h, project_type == ProjectType::ProjectOutput ? 1 : 0));
  fst = detail::download(a);
}

// invert (algorithms/inversion.rs:32-48): in place, like the reference
inline void invert(VectorFst& fst) {
  detail::DeviceFst a;
  detail::upload(fst, a);
  check(wfst_fst_invert(Context::current().get(), a.h));
  fst = detail::download(a);
}

// isomorphic / isomorphic_with_config (algorithms/isomorphic.rs:162-212): the reference's verdict, its error thrown
struct IsomorphicConfig {  // isomorphic.rs:162-176
  float delta = 1.0f / 1024.0f;  // KDELTA
  IsomorphicConfig() = default;
  explicit IsomorphicConfig(float d) : delta(d) {}
};
inline bool isomorphic_with_config(const VectorFst& fst_1, const VectorFst& fst_2, const IsomorphicConfig& config) {
  detail::DeviceFst a, b;
  detail::upload(fst_1, a);
  detail::upload(fst_2, b);
  const wfst_isomorphic_config cfg{config.delta};
  int res = 0;
  check(wfst_isomorphic(Context::current().get(), a.h, b.h, &cfg, &res));
  return res != 0;
}
inline bool isomorphic(const VectorFst& fst_1, const VectorFst& fst_2) { return isomorphic_with_config(fst_1, fst_2, IsomorphicConfig{}); }

inline std::vector<FstPath> VectorFst::paths_iter(uint64_t max_paths) const {
  detail::DeviceFst a;
  detail::upload(*this, a);
  wfst_paths* t = nullptr;
  check(wfst_fst_paths(Context::current().get(), a.h, max_paths, &t));
  struct Guard {
    wfst_paths* t;
    ~Guard() { wfst_paths_destroy(t); }
  } guard{t};
  uint64_t n_paths = 0, n_il = 0, n_ol = 0;
  check(wfst_paths_info(t, nullptr, &n_paths, &n_il, &n_ol));
  std::vector<float> weights(n_paths);
  std::vector<uint64_t> iloff(n_paths + 1), oloff(n_paths + 1);
  std::vector<uint32_t> il(n_il), ol(n_ol);
  check(wfst_paths_download(Context::current().get(), t, nullptr, weights.data(), iloff.data(), il.data(), oloff.data(), ol.data()));
  std::vector<FstPath> out(n_paths);
  for (uint64_t k = 0; k < n_paths; ++k) {
    out[k].ilabels.assign(il.begin() + iloff[k], il.begin() + iloff[k + 1]);
    out[k].olabels.assign(ol.begin() + oloff[k], ol.begin() + oloff[k + 1]);
    out[k].weight = weights[k];
  }
  return out;
}

// connect (algorithms/connect.rs:51-66) and rm_epsilon (algorithms/rm_epsilon/rm_epsilon_static.rs:50-163): in place
inline void connect(VectorFst& fst) {
  detail::DeviceFst a, c;
  detail::upload(fst, a);
  check(wfst_connect(Context::current().get(), a.h, &c.h));
  fst = detail::download(c);
}
inline void rm_epsilon(VectorFst& fst) {
  detail::DeviceFst a, c;
  detail::upload(fst, a);
  check(wfst_rm_epsilon(Context::current().get(), a.h, &c.h));
  fst = detail::download(c);
}

// shortest_distance (shortest_distance.rs:307-336): the reference's Vec, its length included
inline std::vector<float> shortest_distance_with_config(const VectorFst& fst, bool reverse, float delta = 1e-6f) {
  detail::DeviceFst a;
  detail::upload(fst, a);
  uint32_t n = 0, len = 0;
  check(wfst_fst_info(a.h, &n, nullptr, nullptr, nullptr));
  std::vector<float> d(n);
  const wfst_shortest_distance_config cfg{reverse ? 1u : 0u, delta};
  check(wfst_shortest_distance_with_config(Context::current().get(), a.h, &cfg, d.data(), &len));
  d.resize(len);
  return d;
}
inline std::vector<float> shortest_distance(const VectorFst& fst, bool reverse) { return shortest_distance_with_config(fst, reverse); }

// reweight (reweight.rs:29-154) and push_weights[_with_config] (push.rs:76-118): in place, like the reference
enum class ReweightType : uint32_t { ReweightToInitial = 0, ReweightToFinal = 1 };  // reweight.rs:11-17
struct PushWeightsConfig {  // push.rs:34-48
  float delta = 1.0f / 1024.0f;
  bool remove_total_weight = false;
};
inline void reweight(VectorFst& fst, const std::vector<float>& potentials, ReweightType reweight_type) {
  detail::DeviceFst a, c;
  detail::upload(fst, a);
  check(wfst_reweight(Context::current().get(), a.h, potentials.data(), potentials.size(), (uint32_t)reweight_type, &c.h));
  fst = detail::download(c);
}
inline void push_weights_with_config(VectorFst& fst, ReweightType reweight_type, const PushWeightsConfig& config) {
  detail::DeviceFst a, c;
  detail::upload(fst, a);
  const wfst_push_weights_config cfg{config.delta, config.remove_total_weight ? 1u : 0u};
  check(wfst_push_weights(Context::current().get(), a.h, (uint32_t)reweight_type, &cfg, &c.h));
  fst = detail::download(c);
}
inline void push_weights(VectorFst& fst, ReweightType reweight_type) { push_weights_with_config(fst, reweight_type, PushWeightsConfig{}); }

// determinize[_with_config] (determinize_static.rs:149-190): acceptors only (a transducer throws); a new FST, like the reference
enum class DeterminizeType : uint32_t { DeterminizeFunctional = 0, DeterminizeNonFunctional = 1, DeterminizeDisambiguate = 2 };
struct DeterminizeConfig {  // determinize_static.rs:128-147
  float delta = 1.0f / 1024.0f;
  DeterminizeType det_type = DeterminizeType::DeterminizeFunctional;
};
inline VectorFst determinize_with_config(const VectorFst& fst, const DeterminizeConfig& config) {
  detail::DeviceFst a, c;
  detail::upload(fst, a);
  const wfst_determinize_config cfg{config.delta, (uint32_t)config.det_type};
  check(wfst_determinize(Context::current().get(), a.h, &cfg, &c.h));
  return detail::download(c);
}
inline VectorFst determinize(const VectorFst& fst) { return determinize_with_config(fst, DeterminizeConfig{}); }
// determinize_with_config of many acceptors in one call (wfst_determinize_batch): one workgroup per FST
inline std::vector<VectorFst> determinize_batch(const std::vector<VectorFst>& fsts, const DeterminizeConfig& config = DeterminizeConfig{}) {
  std::vector<detail::DeviceFst> in(fsts.size()), out(fsts.size());
  std::vector<const wfst_fst*> hs(fsts.size());
  std::vector<wfst_fst*> os(fsts.size(), nullptr);
  for (size_t i = 0; i < fsts.size(); ++i) {
    detail::upload(fsts[i], in[i]);
    hs[i] = in[i].h;
  }
  const wfst_determinize_config cfg{config.delta, (uint32_t)config.det_type};
  check(wfst_determinize_batch(Context::current().get(), hs.data(), hs.size(), &cfg, os.data(), nullptr));
  std::vector<VectorFst> res;
  for (size_t i = 0; i < fsts.size(); ++i) {
    out[i].h = os[i];
    res.push_back(detail::download(out[i]));
  }
  return res;
}
// determinize_with_distance (determinize_static.rs:24-39): (determinized FST, out_dist)
inline std::pair<VectorFst, std::vector<float>> determinize_with_distance(const VectorFst& fst, const std::vector<float>& in_dist,
                                                                          float delta = 1.0f / 1024.0f) {
  detail::DeviceFst a, c;
  detail::upload(fst, a);
  float* d = nullptr;
  uint64_t nd = 0;
  check(wfst_determinize_with_distance(Context::current().get(), a.h, in_dist.data(), in_dist.size(), delta, &c.h, &d, &nd));
  std::vector<float> dist(d, d + nd);
  wfst_bytes_destroy(reinterpret_cast<uint8_t*>(d));
  return {detail::download(c), std::move(dist)};
}
inline std::vector<std::pair<VectorFst, std::vector<float>>> determinize_with_distance_batch(
    const std::vector<VectorFst>& fsts, const std::vector<std::vector<float>>& in_dists, float delta = 1.0f / 1024.0f) {
  if (in_dists.size() != fsts.size()) throw Error("determinize_with_distance_batch: one in_dist per FST");
  const size_t n = fsts.size();
  std::vector<detail::DeviceFst> in(n), out(n);
  std::vector<const wfst_fst*> hs(n);
  std::vector<wfst_fst*> os(n, nullptr);
  std::vector<const float*> ps(n);
  std::vector<uint64_t> ns(n), off(n + 1, 0);
  for (size_t i = 0; i < n; ++i) {
    detail::upload(fsts[i], in[i]);
    hs[i] = in[i].h;
    ps[i] = in_dists[i].data();
    ns[i] = in_dists[i].size();
  }
  float* d = nullptr;
  check(wfst_determinize_with_distance_batch(Context::current().get(), hs.data(), n, ps.data(), ns.data(), delta, os.data(), &d,
                                             off.data(), nullptr));
  std::vector<std::pair<VectorFst, std::vector<float>>> res;
  for (size_t i = 0; i < n; ++i) {
    out[i].h = os[i];
    res.emplace_back(detail::download(out[i]), std::vector<float>(d + off[i], d + off[i + 1]));
  }
  wfst_bytes_destroy(reinterpret_cast<uint8_t*>(d));
  return res;
}

// minimize[_with_config] (minimize.rs:77-176): deterministic acyclic acceptors only (anything else throws); in place, like
// the reference
struct MinimizeConfig {  // minimize.rs:41-75
  float delta = 1e-6f;  // KSHORTESTDELTA
  bool allow_nondet = false;
};
inline void minimize_with_config(VectorFst& fst, const MinimizeConfig& config) {
  detail::DeviceFst a, c;
  detail::upload(fst, a);
  const wfst_minimize_config cfg{config.delta, config.allow_nondet ? 1u : 0u};
  check(wfst_minimize(Context::current().get(), a.h, &cfg, &c.h));
  fst = detail::download(c);
}
inline void minimize(VectorFst& fst) { minimize_with_config(fst, MinimizeConfig{}); }
// minimize_with_config of many acceptors in one call (wfst_minimize_batch): one workgroup per FST, one launch for all; the
// minimized FSTs (the arguments are left as they are)
inline std::vector<VectorFst> minimize_batch(const std::vector<VectorFst>& fsts, const MinimizeConfig& config = MinimizeConfig{}) {
  std::vector<detail::DeviceFst> in(fsts.size()), out(fsts.size());
  std::vector<const wfst_fst*> hs(fsts.size());
  std::vector<wfst_fst*> os(fsts.size(), nullptr);
  for (size_t i = 0; i < fsts.size(); ++i) {
    detail::upload(fsts[i], in[i]);
    hs[i] = in[i].h;
  }
  const wfst_minimize_config cfg{config.delta, config.allow_nondet ? 1u : 0u};
  check(wfst_minimize_batch(Context::current().get(), hs.data(), hs.size(), &cfg, os.data(), nullptr));
  std::vector<VectorFst> res;
  for (size_t i = 0; i < fsts.size(); ++i) {
    out[i].h = os[i];
    res.push_back(detail::download(out[i]));
  }
  return res;
}
// rm_epsilon of many FSTs in one call (wfst_rm_epsilon_batch): one workgroup per FST, the step in front of
// determinize_batch and minimize_batch; the results (the arguments are left as they are)
inline std::vector<VectorFst> rm_epsilon_batch(const std::vector<VectorFst>& fsts) {
  std::vector<detail::DeviceFst> in(fsts.size()), out(fsts.size());
  std::vector<const wfst_fst*> hs(fsts.size());
  std::vector<wfst_fst*> os(fsts.size(), nullptr);
  for (size_t i = 0; i < fsts.size(); ++i) {
    detail::upload(fsts[i], in[i]);
    hs[i] = in[i].h;
  }
  check(wfst_rm_epsilon_batch(Context::current().get(), hs.data(), hs.size(), os.data(), nullptr));
  std::vector<VectorFst> res;
  for (size_t i = 0; i < fsts.size(); ++i) {
    out[i].h = os[i];
    res.push_back(detail::download(out[i]));
  }
  return res;
}

// top_sort (top_sort.rs:76-94) and state_sort (state_sort.rs:16-78): in place, like the reference; a cyclic FST comes back
// unchanged but for CYCLIC | NOT_TOP_SORTED in its word
inline void top_sort(VectorFst& fst) {
  detail::DeviceFst a, c;
  detail::upload(fst, a);
  check(wfst_top_sort(Context::current().get(), a.h, &c.h));
  fst = detail::download(c);
}
inline void state_sort(VectorFst& fst, const std::vector<uint32_t>& order) {
  detail::DeviceFst a, c;
  detail::upload(fst, a);
  check(wfst_state_sort(Context::current().get(), a.h, order.data(), order.size(), &c.h));
  fst = detail::download(c);
}

// tr_sum (tr_sum.rs:7-22), tr_unique (tr_unique.rs:38-51) and optimize (optimize.rs:11-128; acyclic inputs, anything else
// throws): in place, like the reference
inline void tr_sum(VectorFst& fst) {
  detail::DeviceFst a, c;
  detail::upload(fst, a);
  check(wfst_tr_sum(Context::current().get(), a.h, &c.h));
  fst = detail::download(c);
}
inline void tr_unique(VectorFst& fst) {
  detail::DeviceFst a, c;
  detail::upload(fst, a);
  check(wfst_tr_unique(Context::current().get(), a.h, &c.h));
  fst = detail::download(c);
}
inline void optimize(VectorFst& fst) {
  detail::DeviceFst a, c;
  detail::upload(fst, a);
  check(wfst_optimize(Context::current().get(), a.h, &c.h));
  fst = detail::download(c);
}
// tr_sum, tr_unique and optimize of many FSTs in one call each (wfst_tr_sum_batch, wfst_tr_unique_batch,
// wfst_optimize_batch): the results (the arguments are left as they are)
namespace detail {
template <class Call>
inline std::vector<VectorFst> batch_call(const std::vector<VectorFst>& fsts, Call call) {
  std::vector<DeviceFst> in(fsts.size()), out(fsts.size());
  std::vector<const wfst_fst*> hs(fsts.size());
  std::vector<wfst_fst*> os(fsts.size(), nullptr);
  for (size_t i = 0; i < fsts.size(); ++i) {
    upload(fsts[i], in[i]);
    hs[i] = in[i].h;
  }
  check(call(Context::current().get(), hs.data(), hs.size(), os.data(), nullptr));
  std::vector<VectorFst> res;
  for (size_t i = 0; i < fsts.size(); ++i) {
    out[i].h = os[i];
    res.push_back(download(out[i]));
  }
  return res;
}
}  // namespace detail
inline std::vector<VectorFst> tr_sum_batch(const std::vector<VectorFst>& fsts) { return detail::batch_call(fsts, wfst_tr_sum_batch); }
inline std::vector<VectorFst> tr_unique_batch(const std::vector<VectorFst>& fsts) { return detail::batch_call(fsts, wfst_tr_unique_batch); }
inline std::vector<VectorFst> optimize_batch(const std::vector<VectorFst>& fsts) { return detail::batch_call(fsts, wfst_optimize_batch); }
// top_sort of many FSTs in one call (wfst_top_sort_batch): in place like top_sort, every fsts[i] replaced by its result
inline void top_sort_batch(std::vector<VectorFst>& fsts) { fsts = detail::batch_call(fsts, wfst_top_sort_batch); }

// union (union/union_static.rs:55-118), concat (concat/concat_static.rs:53-109) and closure (closure/closure_static.rs:25-73):
// the first operand is changed in place, like the reference (`union` is a C++ keyword, hence union_).  Results are in general
// not label-sorted: tr_sort before compose.
enum class ClosureType : uint32_t { ClosureStar = 0, ClosurePlus = 1 };  // closure/mod.rs:9-12
inline void union_(VectorFst& a, const VectorFst& b) {
  detail::DeviceFst x, y, c;
  detail::upload(a, x);
  detail::upload(b, y);
  check(wfst_union(Context::current().get(), x.h, y.h, &c.h));
  a = detail::download(c);
}
inline void concat(VectorFst& a, const VectorFst& b) {
  detail::DeviceFst x, y, c;
  detail::upload(a, x);
  detail::upload(b, y);
  check(wfst_concat(Context::current().get(), x.h, y.h, &c.h));
  a = detail::download(c);
}
inline void closure(VectorFst& fst, ClosureType closure_type) {
  detail::DeviceFst a, c;
  detail::upload(fst, a);
  check(wfst_closure(Context::current().get(), a.h, (uint32_t)closure_type, &c.h));
  fst = detail::download(c);
}
// the left folds of rustfst-python's union_list / concat_list in one device call each (wfst_union_list, wfst_concat_list);
// an empty list throws "fsts must be at least of len 1"
namespace detail {
template <class Call>
inline VectorFst list_call(const std::vector<VectorFst>& fsts, Call call) {
  std::vector<DeviceFst> in(fsts.size());
  std::vector<const wfst_fst*> hs(fsts.size());
  for (size_t i = 0; i < fsts.size(); ++i) {
    upload(fsts[i], in[i]);
    hs[i] = in[i].h;
  }
  DeviceFst c;
  check(call(Context::current().get(), hs.data(), hs.size(), &c.h));
  return download(c);
}
}  // namespace detail
inline VectorFst union_list(const std::vector<VectorFst>& fsts) { return detail::list_call(fsts, wfst_union_list); }
inline VectorFst concat_list(const std::vector<VectorFst>& fsts) { return detail::list_call(fsts, wfst_concat_list); }

// replace(fst_list, root, epsilon_on_replace) (replace/replace_static.rs:44-58) in one device call (wfst_replace): the
// recursive transition network over the (label, fst) pairs, expanded from the FST whose label is `root`.  Throws the
// reference's message when no pair has that label, and on a grammar whose expansion reaches a recursive call (the reference
// does not terminate there).  A null entry throws the library's "item {i}: null FST in list"; an FST named more than once is
// uploaded once.
inline VectorFst replace(const std::vector<std::pair<Label, const VectorFst*>>& fst_list, Label root, bool epsilon_on_replace) {
  std::vector<detail::DeviceFst> in(fst_list.size());
  std::vector<wfst_label_fst_pair> pairs(fst_list.size());
  for (size_t i = 0; i < fst_list.size(); ++i) {
    if (!fst_list[i].second) throw Error("item " + std::to_string(i) + ": null FST in list");
    size_t first = 0;
    while (fst_list[first].second != fst_list[i].second) ++first;
    if (first == i) detail::upload(*fst_list[i].second, in[i]);
    pairs[i] = wfst_label_fst_pair{fst_list[i].first, in[first].h};
  }
  detail::DeviceFst c;
  check(wfst_replace(Context::current().get(), root, pairs.data(), pairs.size(), epsilon_on_replace ? 1u : 0u, &c.h));
  return detail::download(c);
}

// Look-ahead composition.  The reference has no single function for it: callers assemble MatcherFst::new_with_relabeling,
// a LabelLookAheadMatcher and the PushLabels(PushWeights(LookAhead(AltSequence))) filter by hand and call compute()
// (rustfst-cli/src/cmds/compose.rs:77-181).  LookAheadFst is the MatcherFst of that recipe (keep it while the same first
// operand meets further second operands); compose_lookahead is the whole recipe for one pair.  The result is not connected.
class LookAheadFst {
 public:
  explicit LookAheadFst(const VectorFst& fst1) {  // MatcherFst::new, compose/matcher_fst.rs:55-71
    detail::DeviceFst a;
    detail::upload(fst1, a);
    check(wfst_lookahead_create(Context::current().get(), a.h, &h_));
  }
  ~LookAheadFst() { if (h_) wfst_lookahead_destroy(h_); }
  LookAheadFst(const LookAheadFst&) = delete;
  LookAheadFst& operator=(const LookAheadFst&) = delete;
  // LabelLookAheadRelabeler::relabel(fst2, .., true) + tr_sort(ILabelCompare), then ComposeFst::new_with_options(..).compute()
  VectorFst compose(const VectorFst& fst2) const {
    detail::DeviceFst b, br, c;
    detail::upload(fst2, b);
    check(wfst_lookahead_relabel(h_, b.h, &br.h));
    check(wfst_compose_lookahead(Context::current().get(), h_, br.h, &c.h));
    return detail::download(c);
  }
  wfst_lookahead* raw() const { return h_; }

 private:
  wfst_lookahead* h_ = nullptr;
};
inline VectorFst compose_lookahead(const VectorFst& fst1, const VectorFst& fst2) { return LookAheadFst(fst1).compose(fst2); }

}  // namespace wfst_amd

#endif  // WFST_AMD_HPP
