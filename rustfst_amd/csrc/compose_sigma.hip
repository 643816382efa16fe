// compose_sigma.hip — composition with a SigmaMatcher on one or both sides (compose_with_config with a non-empty
// matcher1_config / matcher2_config, compose/compose_static.rs:166-266) on the wide driver of compose_wide.h: a NEW handle,
// bit for bit what the reference returns.  One arc labelled sigma on the matched tape stands for "any other label".
//
// SigmaPolicy is PlainPolicy (compose_wide.hip) with the matcher of a side replaced by SigmaMatcher<SortedMatcher>
// (compose/matchers/sigma_matcher.rs:33-307).  What changes, with the reference's lines:
//   which side is iterated   match_input, compose_fst_op.rs:199-219, BOTH mode only: a state of a sigma side has
//                            REQUIRE_PRIORITY iff it carries an arc labelled sigma on the matched tape (has_sigma :33-45,
//                            priority :134-144).  Both require: Err "Both sides can't require match" (:207-209); side 1
//                            requires: fst2 is iterated (:210-212); side 2 requires: fst1 (:213-215); neither: n1 <= n2 (:216).
//   iter(state, label)       IteratorSigmaMatcher::new, sigma_matcher.rs:190-239:
//                              label == sigma (sigma real): Err "SigmaMatcher::Find: bad label (sigma)" (:199-201), whether
//                                or not the state has a sigma arc;
//                              the sorted matcher yields something for `label` (:206-208; for label 0 the EpsLoop and then the
//                                real epsilons, so never nothing; for NO_LABEL the real epsilons, sorted_matcher.rs:124-184):
//                                that is the whole answer, nothing is rewritten (sigma_match = NO_LABEL, :243-244);
//                              else the sigma arcs of the state, in order and rewritten, iff the state has one, `label` is
//                                neither 0 nor NO_LABEL and the allowed set is absent or holds `label` (:211-217);
//                              else nothing (find_empty, :218-223).
//                            There is no fall-through from exhausted exact matches to the sigma arcs: next_openfst's branch
//                            (:270-284) needs `r.is_none()`, and next() (:296-306) only calls it after a successful peek.
//   rewriting                value_openfst, :246-266: rewrite_both (Auto: the sigma operand's word has ACCEPTOR, Always,
//                            Never; :67-75) sets each of ilabel / olabel that equals sigma to the matched label; without it
//                            only the matched tape's label is set (ilabel under MatchInput, olabel under MatchOutput).
//   filters                  a rewritten pair has a real, equal, non-epsilon label on both matched tapes: class M of
//                            compose_filters.h, every filter answers 0.  set_state's epsilon facts do not look at matchers.
//   property word            ComposeFstOp::new asks the filter alone (compose_fst_op.rs:154-157): props::compose_result of the
//                            operands' words, as for the plain call.
//   errors                   LazyFst::compute (lazy/lazy_fst.rs:226-269) expands states in id order and returns the first Err:
//                            the policy keeps the minimum of (state id << 32 | item << 1 | kind) in one word (kind 0: both
//                            sides require, found before the items; kind 1: bad label at item j).  Every state of a level
//                            reports its errors; once the word is set the states of later levels emit nothing, so the search
//                            ends within a level.
// Every single sigma call runs on this driver, whatever its size: the wave-per-problem kernels of compose.hip do not learn
// about sigma.  Many utterances against one sigma grammar: compose_sigma_batch.hip.
#include "compose_wide.h"
#include "fst_props.h"
#include "sigma_ranges.h"

namespace wfst {
namespace {

constexpr uint64_t SG_NO_ERROR = ~0ull;
// counters of the policy block: one 128-byte line each (same-address atomics serialise), 64-bit words
enum : uint32_t { SG_REQUIRE1 = 0, SG_REQUIRE2, SG_EXACT, SG_SIGMA_ITEMS, SG_SIGMA_ARCS, SG_REFUSED, SG_COUNTERS };
constexpr uint32_t SG_STRIDE = 16;  // 64-bit words per line; word 0 of line SG_COUNTERS is the error word

struct SgSide {
  const wfst_tr* arcs;
  const uint4* srec;        // {arc begin, arc count, final bits, SREC_* epsilon facts}
  const uint2* sig;         // [n_states] {first sigma arc within the state's arcs, how many}; null: no sigma matcher here
  const uint32_t* allowed;  // ascending and distinct; n_allowed == 0: no restriction
  uint32_t n_allowed;
  uint32_t sigma;         // NO_LABEL without a sigma matcher (has_sigma is false everywhere then, sigma_matcher.rs:40-44)
  uint32_t rewrite_both;  // sigma_matcher.rs:67-75
  uint32_t pad;
};

struct SgExpand {
  bool mi;
  const wfst_tr* it_arcs;
  const wfst_tr* se_arcs;
  uint32_t n_it, n_se, sa, sb;
  uint32_t fs_nolabel, fs_eps, fsZ, fsM;  // filter_tr outcomes of the four pair classes (compose_filters.h)
  float final_weight;
  uint32_t sig_lo, sig_n;   // the sigma arcs of the searched state, within se_arcs (whichever copy it points at)
  uint32_t wide_state_id;   // the composed state's id: set by la_emit (compose_wide.h)
  uint32_t seen_to;  // items this lane has evaluated so far: the driver walks them twice, the counters count the first walk
  bool both;         // both sides require (BOTH mode): an error, no items
  bool dead;         // an error is known: the state emits nothing
  bool req1, req2;
};

// one add per wave for the lanes (of those that are here together) whose `pred` holds
__device__ __forceinline__ void sg_count(unsigned long long* ctr, bool pred) {
  const uint64_t m = __ballot(pred);
  if (pred && lanes_below(m) == 0) atomicAdd(ctr, (unsigned long long)__popcll(m));
}

struct SigmaPolicy {
  SgSide f1, f2;
  uint32_t mode, filter;
  unsigned long long* blk;  // SG_COUNTERS lines of counters, then the error word's line
  using Expand = SgExpand;

  __device__ unsigned long long* ctr(uint32_t k) const { return blk + k * SG_STRIDE; }
  __device__ unsigned long long* err() const { return blk + SG_COUNTERS * SG_STRIDE; }

  __device__ Expand make_expand(uint64_t tlo, uint64_t thi) const {
    Expand x;
    const uint32_t s1 = (uint32_t)(tlo >> 32), s2 = (uint32_t)tlo, fs = (uint32_t)thi;
    const uint4 r1 = f1.srec[s1], r2 = f2.srec[s2];
    const uint2 g1 = f1.sig ? f1.sig[s1] : make_uint2(0u, 0u), g2 = f2.sig ? f2.sig[s2] : make_uint2(0u, 0u);
    const uint32_t n1 = r1.y, n2 = r2.y;
    const float fin1 = __uint_as_float(r1.z), fin2 = __uint_as_float(r2.z);
    x.final_weight = (fin1 != INF && fin2 != INF) ? wtimes(fin1, fin2) : INF;  // compute_final_weight, compose_fst_op.rs:420-449
    const bool alleps1 = (r1.w & SREC_ALL_OEPS) && !(fin1 != INF);
    const bool noeps1 = (r1.w & SREC_NO_OEPS) != 0;
    const bool alleps2 = (r2.w & SREC_ALL_IEPS) && !(fin2 != INF);
    const bool noeps2 = (r2.w & SREC_NO_IEPS) != 0;
    x.req1 = g1.y != 0u;  // REQUIRE_PRIORITY, sigma_matcher.rs:134-144
    x.req2 = g2.y != 0u;
    x.both = mode == MODE_BOTH && x.req1 && x.req2;  // compose_fst_op.rs:207-209
    // match_input, compose_fst_op.rs:199-219
    x.mi = mode == MODE_BOTH ? (x.req1 ? false : (x.req2 ? true : n1 <= n2)) : (mode == MODE_INPUT);
    x.it_arcs = x.mi ? f1.arcs + r1.x : f2.arcs + r2.x;
    x.se_arcs = x.mi ? f2.arcs + r2.x : f1.arcs + r1.x;
    x.n_it = x.both ? 0u : (x.mi ? n1 : n2);
    x.n_se = x.both ? 0u : (x.mi ? n2 : n1);
    x.sa = x.mi ? s2 : s1;
    x.sb = x.mi ? s1 : s2;
    x.sig_lo = x.mi ? g2.x : g1.x;
    x.sig_n = x.both ? 0u : (x.mi ? g2.y : g1.y);
    const FilterOutcomes fo = filter_outcomes(filter, fs, alleps1, noeps1, alleps2, noeps2);  // compose_filters.h
    x.fs_nolabel = x.mi ? fo.fsX : fo.fsY;
    x.fs_eps = x.mi ? fo.fsY : fo.fsX;
    x.fsZ = fo.fsZ;
    x.fsM = 0u;
    x.wide_state_id = 0u;
    x.seen_to = 0u;
    // (an error raised while this level runs is seen by the next one at the latest: what is emitted meanwhile is discarded)
    x.dead = ld_l2(err()) != SG_NO_ERROR;
    return x;
  }

  __device__ bool allowed(const SgSide& se, uint32_t label) const {  // is_match_label_allowed, sigma_matcher.rs:172-181
    if (se.n_allowed == 0u) return true;
    uint32_t lo = 0, hi = se.n_allowed;
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (se.allowed[mid] < label) lo = mid + 1; else hi = mid;
    }
    return lo < se.n_allowed && se.allowed[lo] == label;
  }

  // item 0 = the loop pseudo-arc (ordered_expand, compose_fst_op.rs:229-233), item j = the j-th arc of the iterated side
  __device__ uint32_t eval_item(Expand& x, uint32_t j, bool write, uint32_t write_pos, wfst_tr* arcs, uint64_t* a_lo,
                                uint64_t* a_hi, Emitted* first) const {
    const bool first_walk = j >= x.seen_to;  // (a lane's items ascend within a walk)
    if (first_walk) x.seen_to = j + 1;
    if (x.both) {  // (the state has item 0 alone)
      if (first_walk) atomicMin(err(), (unsigned long long)x.wide_state_id << 32);
      return 0u;
    }
    const bool mi = x.mi;
    const SgSide& se = mi ? f2 : f1;
    const ArcReg ab = j == 0 ? loop_item(mi, x.sb) : load_arc(x.it_arcs + (j - 1));
    const uint32_t label = mi ? ab.ol : ab.il;
    if (se.sigma != NO_LABEL && label == se.sigma) {  // sigma_matcher.rs:199-201
      if (first_walk) atomicMin(err(), ((unsigned long long)x.wide_state_id << 32) | ((unsigned long long)j << 1) | 1ull);
      return 0u;
    }
    if (first_walk && j == 0) {
      sg_count(ctr(SG_REQUIRE1), x.req1);
      sg_count(ctr(SG_REQUIRE2), x.req2);
    }
    if (x.dead) return 0u;
    uint32_t lo = 0, cnt = 0;
    equal_range(x.se_arcs, x.n_se, mi, label == NO_LABEL ? 0u : label, &lo, &cnt);
    uint32_t loop1 = 0, fsn;
    if (label == NO_LABEL) {
      fsn = x.fs_nolabel;
    } else if (label == 0u) {
      loop1 = x.fs_eps != FILTER_REJECT ? 1u : 0u;
      fsn = x.fsZ;
    } else {
      fsn = x.fsM;
    }
    // the fallback of sigma_matcher.rs:209-217: nothing exact (label 0 always yields the EpsLoop), a sigma arc, a real label
    // that the allowed set admits
    const bool fallback = cnt == 0u && label != 0u && label != NO_LABEL && x.sig_n != 0u;
    const bool by_sigma = fallback && allowed(se, label);
    if (by_sigma) {
      lo = x.sig_lo;
      cnt = x.sig_n;
    }
    if (first_walk && se.sigma != NO_LABEL) {
      sg_count(ctr(SG_EXACT), !fallback && (cnt != 0u || label == 0u));
      sg_count(ctr(SG_SIGMA_ITEMS), by_sigma);
      sg_count(ctr(SG_SIGMA_ARCS), by_sigma && cnt == 1u);  // (one sigma arc per state is the rule; more add their own)
      if (by_sigma && cnt > 1u) atomicAdd(ctr(SG_SIGMA_ARCS), (unsigned long long)cnt);
      sg_count(ctr(SG_REFUSED), fallback && !by_sigma);
    }
    const uint32_t n_real = fsn != FILTER_REJECT ? cnt : 0u;
    uint32_t k = 0;
    for (uint32_t m = 0; m < loop1 + n_real; ++m) {
      const bool is_loop = m < loop1;
      ArcReg aa = is_loop ? eps_loop(mi, x.sa) : load_arc(x.se_arcs + lo + (m - loop1));
      if (by_sigma) {  // value_openfst, sigma_matcher.rs:246-266
        if (se.rewrite_both) {
          if (aa.il == se.sigma) aa.il = label;
          if (aa.ol == se.sigma) aa.ol = label;
        } else if (mi) {
          aa.il = label;
        } else {
          aa.ol = label;
        }
      }
      const ArcReg a1 = mi ? ab : aa;  // arc1 from fst1, arc2 from fst2 (match_tr_selected, compose_fst_op.rs:301-319)
      const ArcReg a2 = mi ? aa : ab;
      const uint4 arc = make_uint4(a1.il, a2.ol, __float_as_uint(wtimes(a1.w, a2.w)), 0u);  // add_tr :267-285
      const uint64_t dlo = ((uint64_t)a1.ns << 32) | a2.ns, dhi = is_loop ? x.fs_eps : fsn;
      if (write) {
        *reinterpret_cast<uint4*>(arcs + write_pos + k) = arc;
        a_lo[write_pos + k] = dlo;
        a_hi[write_pos + k] = dhi;
      } else if (first && k == 0) {
        first->arc = arc;
        first->lo = dlo;
        first->hi = dhi;
      }
      k++;
    }
    return k;
  }
};

}  // namespace

// the set-up errors of compose_with_config with matcher configs, in the reference's order, and the match mode they leave:
// nothing here touches the device (compose_sigma_batch.hip decides every item of a batch with it before anything is launched)
uint32_t sigma_setup_mode(const wfst_fst* f1, const wfst_fst* f2, uint32_t filter, const SigmaSpec* m1, const SigmaSpec* m2) {
  using namespace props;
  // compose_with_config creates both matchers first (compose_static.rs:178-183): SigmaMatcher::new, sigma_matcher.rs:64-66
  for (const SigmaSpec* m : {m1, m2})
    if (m && m->sigma_label == 0u) throw Error("SigmaMatcher: 0 cannot be used as sigma_label");
  // ... only then does it look at the filter (:185-191)
  if (filter == 0u && (m1 || m2)) throw Error("Custom MatcherConfig not supported with AutoFilter");
  // REQUIRE_MATCH (sigma_matcher.rs:126-132) -> the side must be sorted on its matched tape, match_type(true)
  // (compose_fst_op.rs:169-180); an unknown bit pair fails properties_check as in the plain mode decision
  if (m1 && m1->sigma_label != NO_LABEL) {
    if (!(f1->props & (O_LABEL_SORTED | NOT_O_LABEL_SORTED))) throw Error("ComposeFst: 1st argument: label-sortedness properties are not known (sort?)");
    if (!(f1->props & O_LABEL_SORTED)) throw Error("ComposeFst: 1st argument cannot perform required matching (sort?)");
  }
  if (m2 && m2->sigma_label != NO_LABEL) {
    if (!(f2->props & (I_LABEL_SORTED | NOT_I_LABEL_SORTED))) throw Error("ComposeFst: 2nd argument: label-sortedness properties are not known (sort?)");
    if (!(f2->props & I_LABEL_SORTED)) throw Error("ComposeFst: 2nd argument cannot perform required matching (sort?)");
  }
  return decide_match_mode(f1->props, f2->props);
}

wfst_fst* compose_sigma(wfst_ctx* ctx, const wfst_fst* f1, const wfst_fst* f2, bool connect, uint32_t filter, const SigmaSpec* m1,
                        const SigmaSpec* m2) {
  using namespace props;
  ctx->compose_sigma = wfst_ctx::ComposeSigmaStats{};
  const uint32_t mode = sigma_setup_mode(f1, f2, filter, m1, m2);
  ensure_device(const_cast<wfst_fst*>(f1));
  ensure_device(const_cast<wfst_fst*>(f2));
  const bool has_start = f1->start >= 0 && f2->start >= 0;
  // the filter alone is asked for the word (compose_fst_op.rs:154-157): the plain call's
  const uint64_t out_props = compose_result(f1->props, f2->props, connect, has_start);
  if (!has_start) {  // compute_start -> None: empty FST (lazy_fst.rs:229-232)
    HostCsr h;
    h.offsets.push_back(0);
    return make_host_fst(ctx, 0, -1, out_props, std::move(h));
  }
  hipStream_t st = ctx->stream;
  SigmaTables b1, b2;
  auto side = [&](const wfst_fst* f, const SigmaSpec* m, bool by_ilabel, SigmaTables& b) {
    sigma_tables(ctx, f, m, by_ilabel, b);  // sigma_ranges.h
    return SgSide{f->dev.arcs, f->dev.srec, b.sig.p, b.allowed.p, b.n_allowed, b.sigma, b.rewrite_both, 0u};
  };
  const SgSide s1 = side(f1, m1, /*by_ilabel=*/false, b1), s2 = side(f2, m2, /*by_ilabel=*/true, b2);
  constexpr size_t BLK_WORDS = (size_t)(SG_COUNTERS + 1) * SG_STRIDE;
  DBuf<unsigned long long> d_blk(*ctx->pool, BLK_WORDS);
  HIP_CHECK(hipMemsetAsync(d_blk.p, 0, SG_COUNTERS * SG_STRIDE * sizeof(unsigned long long), st));
  HIP_CHECK(hipMemsetAsync(d_blk.p + SG_COUNTERS * SG_STRIDE, 0xFF, SG_STRIDE * sizeof(unsigned long long), st));  // SG_NO_ERROR

  const SigmaPolicy pol{s1, s2, mode, filter, d_blk.p};
  const double d1 = (double)f1->n_arcs / std::max<uint32_t>(f1->n_states, 1), d2 = (double)f2->n_arcs / std::max<uint32_t>(f2->n_states, 1);
  // the iterated side: in BOTH mode a lone sigma side is searched wherever it carries a sigma arc
  const bool sg1 = s1.sig != nullptr, sg2 = s2.sig != nullptr;
  const double items = 1.0 + (mode == MODE_INPUT ? d1 : mode == MODE_OUTPUT ? d2 : (sg1 != sg2 ? (sg2 ? d1 : d2) : std::min(d1, d2)));
  const uint64_t est_s = 4ull * std::max<uint64_t>(std::min(f1->n_states, f2->n_states), 64) + 1024;
  uint64_t grows = 0;
  const WideWho who{"compose", "composition", &grows};
  WideOutput w;
  try {
    run_wide(ctx, pol, ((uint64_t)(uint32_t)f1->start << 32) | (uint32_t)f2->start, 0ull, est_s, 4 * est_s, items, w, who);
  } catch (...) {
    ctx->stats.compose_retries += grows;
    ctx->compose_sigma.arena_grows = grows;
    throw;
  }
  ctx->stats.compose_retries += grows;
  ctx->compose_sigma.arena_grows = grows;
  unsigned long long* hb = (unsigned long long*)ctx->pinned.get(BLK_WORDS * sizeof(unsigned long long));  // (the driver's staging block is free again)
  HIP_CHECK(hipMemcpyAsync(hb, d_blk.p, BLK_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  const uint64_t e = hb[SG_COUNTERS * SG_STRIDE];
  if (e != SG_NO_ERROR) {
    if (e & 1ull) throw Error("SigmaMatcher::Find: bad label (sigma)");
    throw Error("Both sides can't require match");
  }
  ctx->compose_sigma.levels = w.n_levels;
  ctx->compose_sigma.level_launches = w.n_level_launches;
  ctx->compose_sigma.states = w.n_states;
  ctx->compose_sigma.arcs = w.n_arcs;
  ctx->compose_sigma.require1_states = hb[SG_REQUIRE1 * SG_STRIDE];
  ctx->compose_sigma.require2_states = hb[SG_REQUIRE2 * SG_STRIDE];
  ctx->compose_sigma.exact_items = hb[SG_EXACT * SG_STRIDE];
  ctx->compose_sigma.sigma_items = hb[SG_SIGMA_ITEMS * SG_STRIDE];
  ctx->compose_sigma.sigma_arcs = hb[SG_SIGMA_ARCS * SG_STRIDE];
  ctx->compose_sigma.refused_items = hb[SG_REFUSED * SG_STRIDE];
  ctx->stats.compose_states = w.n_states;
  ctx->stats.compose_arcs = w.n_arcs;
  if (!connect) return adopt_device(ctx, w.n_states, w.n_arcs, 0, out_props, w.off, w.arcs, w.fin);
  return connect_and_adopt(ctx, w.n_states, 0, w.off, w.arcs, w.fin, /*all_accessible=*/true, out_props);
}

}  // namespace wfst
