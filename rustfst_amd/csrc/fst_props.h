// fst_props.h — the 64-bit FstProperties word that crosses the C-ABI.
// Bit values: rustfst/src/fst_properties/properties.rs:22-103 (OpenFST-compatible).
// Update rules: rustfst/src/fst_properties/mutate_properties.rs (cited per function).
#pragma once
#include <cstdint>

#include "../../include/wfst.h"
#include "tropical.h"

namespace wfst::props {

// TropicalWeight's approximate ==, is_zero / is_one and "weighted" (tropical.h) decide the WEIGHTED / UNWEIGHTED bits
using wfst::is_one;
using wfst::is_zero;
using wfst::KDELTA;
using wfst::weighted;
using wfst::weq;

constexpr uint64_t ACCEPTOR = 0x0000000000010000ull, NOT_ACCEPTOR = 0x0000000000020000ull;
constexpr uint64_t I_DETERMINISTIC = 0x0000000000040000ull, NOT_I_DETERMINISTIC = 0x0000000000080000ull;
constexpr uint64_t O_DETERMINISTIC = 0x0000000000100000ull, NOT_O_DETERMINISTIC = 0x0000000000200000ull;
constexpr uint64_t EPSILONS = 0x0000000000400000ull, NO_EPSILONS = 0x0000000000800000ull;
constexpr uint64_t I_EPSILONS = 0x0000000001000000ull, NO_I_EPSILONS = 0x0000000002000000ull;
constexpr uint64_t O_EPSILONS = 0x0000000004000000ull, NO_O_EPSILONS = 0x0000000008000000ull;
constexpr uint64_t I_LABEL_SORTED = 0x0000000010000000ull, NOT_I_LABEL_SORTED = 0x0000000020000000ull;
constexpr uint64_t O_LABEL_SORTED = 0x0000000040000000ull, NOT_O_LABEL_SORTED = 0x0000000080000000ull;
constexpr uint64_t WEIGHTED = 0x0000000100000000ull, UNWEIGHTED = 0x0000000200000000ull;
constexpr uint64_t CYCLIC = 0x0000000400000000ull, ACYCLIC = 0x0000000800000000ull;
constexpr uint64_t INITIAL_CYCLIC = 0x0000001000000000ull, INITIAL_ACYCLIC = 0x0000002000000000ull;
constexpr uint64_t TOP_SORTED = 0x0000004000000000ull, NOT_TOP_SORTED = 0x0000008000000000ull;
constexpr uint64_t ACCESSIBLE = 0x0000010000000000ull, NOT_ACCESSIBLE = 0x0000020000000000ull;
constexpr uint64_t COACCESSIBLE = 0x0000040000000000ull, NOT_COACCESSIBLE = 0x0000080000000000ull;
constexpr uint64_t STRING = 0x0000100000000000ull, NOT_STRING = 0x0000200000000000ull;
constexpr uint64_t WEIGHTED_CYCLES = 0x0000400000000000ull, UNWEIGHTED_CYCLES = 0x0000800000000000ull;
constexpr uint64_t ALL = 0x0000ffffffff0000ull;  // trinary bits; EXPANDED|MUTABLE (0x3) are static (properties.rs:5-6)
constexpr uint64_t STATIC_BITS = 0x3;

// FstProperties::null_properties(): properties.rs:105-124 (VectorFst::new)
constexpr uint64_t NULL_PROPS = ACCEPTOR | I_DETERMINISTIC | O_DETERMINISTIC | NO_EPSILONS | NO_I_EPSILONS |
                                NO_O_EPSILONS | I_LABEL_SORTED | O_LABEL_SORTED | UNWEIGHTED | ACYCLIC |
                                INITIAL_ACYCLIC | TOP_SORTED | ACCESSIBLE | COACCESSIBLE | STRING | UNWEIGHTED_CYCLES;

// preserved-by masks: properties.rs:166-300
constexpr uint64_t SET_START_MASK = ACCEPTOR | NOT_ACCEPTOR | I_DETERMINISTIC | NOT_I_DETERMINISTIC | O_DETERMINISTIC |
                                    NOT_O_DETERMINISTIC | EPSILONS | NO_EPSILONS | I_EPSILONS | NO_I_EPSILONS |
                                    O_EPSILONS | NO_O_EPSILONS | I_LABEL_SORTED | NOT_I_LABEL_SORTED | O_LABEL_SORTED |
                                    NOT_O_LABEL_SORTED | WEIGHTED | UNWEIGHTED | CYCLIC | ACYCLIC | TOP_SORTED |
                                    NOT_TOP_SORTED | COACCESSIBLE | NOT_COACCESSIBLE | WEIGHTED_CYCLES |
                                    UNWEIGHTED_CYCLES;
constexpr uint64_t SET_FINAL_MASK = ACCEPTOR | NOT_ACCEPTOR | I_DETERMINISTIC | NOT_I_DETERMINISTIC | O_DETERMINISTIC |
                                    NOT_O_DETERMINISTIC | EPSILONS | NO_EPSILONS | I_EPSILONS | NO_I_EPSILONS |
                                    O_EPSILONS | NO_O_EPSILONS | I_LABEL_SORTED | NOT_I_LABEL_SORTED | O_LABEL_SORTED |
                                    NOT_O_LABEL_SORTED | CYCLIC | ACYCLIC | INITIAL_CYCLIC | INITIAL_ACYCLIC |
                                    TOP_SORTED | NOT_TOP_SORTED | ACCESSIBLE | NOT_ACCESSIBLE | WEIGHTED_CYCLES |
                                    UNWEIGHTED_CYCLES;
constexpr uint64_t ADD_STATE_MASK = ACCEPTOR | NOT_ACCEPTOR | I_DETERMINISTIC | NOT_I_DETERMINISTIC | O_DETERMINISTIC |
                                    NOT_O_DETERMINISTIC | EPSILONS | NO_EPSILONS | I_EPSILONS | NO_I_EPSILONS |
                                    O_EPSILONS | NO_O_EPSILONS | I_LABEL_SORTED | NOT_I_LABEL_SORTED | O_LABEL_SORTED |
                                    NOT_O_LABEL_SORTED | WEIGHTED | UNWEIGHTED | CYCLIC | ACYCLIC | INITIAL_CYCLIC |
                                    INITIAL_ACYCLIC | TOP_SORTED | NOT_TOP_SORTED | NOT_ACCESSIBLE | NOT_COACCESSIBLE |
                                    NOT_STRING | WEIGHTED_CYCLES | UNWEIGHTED_CYCLES;
constexpr uint64_t ADD_ARC_MASK = NOT_ACCEPTOR | NOT_I_DETERMINISTIC | NOT_O_DETERMINISTIC | EPSILONS | I_EPSILONS |
                                  O_EPSILONS | NOT_I_LABEL_SORTED | NOT_O_LABEL_SORTED | WEIGHTED | CYCLIC |
                                  INITIAL_CYCLIC | NOT_TOP_SORTED | ACCESSIBLE | COACCESSIBLE | WEIGHTED_CYCLES;
constexpr uint64_t DELETE_STATES_MASK = ACCEPTOR | I_DETERMINISTIC | O_DETERMINISTIC | NO_EPSILONS | NO_I_EPSILONS |
                                        NO_O_EPSILONS | I_LABEL_SORTED | O_LABEL_SORTED | UNWEIGHTED | ACYCLIC |
                                        INITIAL_ACYCLIC | TOP_SORTED | UNWEIGHTED_CYCLES;

inline uint64_t set_start(uint64_t in) {  // mutate_properties.rs:7-13
  uint64_t out = in & SET_START_MASK;
  if (in & ACYCLIC) out |= INITIAL_ACYCLIC;
  return out;
}
inline uint64_t set_final(uint64_t in, const float* old_w, const float* new_w) {  // :15-37
  uint64_t out = in;
  if (old_w && weighted(*old_w)) out &= ~WEIGHTED;
  if (new_w && weighted(*new_w)) {
    out |= WEIGHTED;
    out &= ~UNWEIGHTED;
  }
  return out & (SET_FINAL_MASK | WEIGHTED | UNWEIGHTED);
}
inline uint64_t add_state(uint64_t in) { return in & ADD_STATE_MASK; }  // :39-41
inline uint64_t add_tr(uint64_t in, uint32_t state, const wfst_tr& tr, const wfst_tr* prev) {  // :43-100
  uint64_t out = in;
  if (tr.ilabel != tr.olabel) out = (out | NOT_ACCEPTOR) & ~ACCEPTOR;
  if (tr.ilabel == WFST_EPS_LABEL) {
    out = (out | I_EPSILONS) & ~NO_I_EPSILONS;
    if (tr.olabel == WFST_EPS_LABEL) out = (out | EPSILONS) & ~NO_EPSILONS;
  }
  if (tr.olabel == WFST_EPS_LABEL) out = (out | O_EPSILONS) & ~NO_O_EPSILONS;
  if (prev) {
    if (prev->ilabel > tr.ilabel) out = (out | NOT_I_LABEL_SORTED) & ~I_LABEL_SORTED;
    if (prev->olabel > tr.olabel) out = (out | NOT_O_LABEL_SORTED) & ~O_LABEL_SORTED;
  }
  if (weighted(tr.weight)) out = (out | WEIGHTED) & ~UNWEIGHTED;
  if (tr.nextstate <= state) out = (out | NOT_TOP_SORTED) & ~TOP_SORTED;
  out &= ADD_ARC_MASK | ACCEPTOR | NO_EPSILONS | NO_I_EPSILONS | NO_O_EPSILONS | I_LABEL_SORTED | O_LABEL_SORTED |
         UNWEIGHTED | TOP_SORTED;
  if (out & TOP_SORTED) out |= ACYCLIC | INITIAL_ACYCLIC;
  return out;
}
// add_tr over a whole SET of arcs at once.  Every effect of add_tr is a sticky set/clear decided by one fact about the arc,
// followed by a mask that is the same for every arc, so folding add_tr over any number of arcs (in any order) equals one
// application with the union of their facts.
constexpr uint32_t FACT_NOT_ACCEPTOR = 1u;      // ilabel != olabel
constexpr uint32_t FACT_I_EPSILON = 2u;         // ilabel == 0
constexpr uint32_t FACT_EPSILON = 4u;           // ilabel == 0 && olabel == 0
constexpr uint32_t FACT_O_EPSILON = 8u;         // olabel == 0
constexpr uint32_t FACT_NOT_I_SORTED = 16u;     // ilabel below its predecessor's
constexpr uint32_t FACT_NOT_O_SORTED = 32u;     // olabel below its predecessor's
constexpr uint32_t FACT_WEIGHTED = 64u;         // arc weight neither zero nor one
constexpr uint32_t FACT_NOT_TOP_SORTED = 128u;  // nextstate <= state
constexpr uint32_t FACT_FINAL_WEIGHTED = 256u;  // a final weight that is not one (no arc fact: minimize.hip's content scan)
// the facts arc `a` of `state` contributes; prev = the arc before it in the state's list (nullptr: no label-order facts)
WFST_HD inline uint32_t arc_facts(const wfst_tr& a, const wfst_tr* prev, uint32_t state) {
  uint32_t facts = (a.ilabel != a.olabel ? FACT_NOT_ACCEPTOR : 0u) | (a.ilabel == WFST_EPS_LABEL ? FACT_I_EPSILON : 0u) |
                   (a.ilabel == WFST_EPS_LABEL && a.olabel == WFST_EPS_LABEL ? FACT_EPSILON : 0u) |
                   (a.olabel == WFST_EPS_LABEL ? FACT_O_EPSILON : 0u) | (weighted(a.weight) ? FACT_WEIGHTED : 0u) |
                   (a.nextstate <= state ? FACT_NOT_TOP_SORTED : 0u);
  if (prev) facts |= (prev->ilabel > a.ilabel ? FACT_NOT_I_SORTED : 0u) | (prev->olabel > a.olabel ? FACT_NOT_O_SORTED : 0u);
  return facts;
}
inline uint64_t add_trs_by_facts(uint64_t in, uint32_t facts) {
  uint64_t out = in;
  if (facts & FACT_NOT_ACCEPTOR) out = (out | NOT_ACCEPTOR) & ~ACCEPTOR;
  if (facts & FACT_I_EPSILON) out = (out | I_EPSILONS) & ~NO_I_EPSILONS;
  if (facts & FACT_EPSILON) out = (out | EPSILONS) & ~NO_EPSILONS;
  if (facts & FACT_O_EPSILON) out = (out | O_EPSILONS) & ~NO_O_EPSILONS;
  if (facts & FACT_NOT_I_SORTED) out = (out | NOT_I_LABEL_SORTED) & ~I_LABEL_SORTED;
  if (facts & FACT_NOT_O_SORTED) out = (out | NOT_O_LABEL_SORTED) & ~O_LABEL_SORTED;
  if (facts & FACT_WEIGHTED) out = (out | WEIGHTED) & ~UNWEIGHTED;
  if (facts & FACT_NOT_TOP_SORTED) out = (out | NOT_TOP_SORTED) & ~TOP_SORTED;
  out &= ADD_ARC_MASK | ACCEPTOR | NO_EPSILONS | NO_I_EPSILONS | NO_O_EPSILONS | I_LABEL_SORTED | O_LABEL_SORTED |
         UNWEIGHTED | TOP_SORTED;
  if (out & TOP_SORTED) out |= ACYCLIC | INITIAL_ACYCLIC;
  return out;
}
// the label / weight part of compute_fst_properties' word (compute_fst_properties.rs:60-190) from the facts of ALL arcs
// and final weights.  The STRING pair is left out (minimize.hip, its only user, never keeps either bit).
inline uint64_t content_props(uint32_t facts) {
  uint64_t p = 0;
  p |= (facts & FACT_NOT_ACCEPTOR) ? NOT_ACCEPTOR : ACCEPTOR;
  p |= (facts & FACT_I_EPSILON) ? I_EPSILONS : NO_I_EPSILONS;
  p |= (facts & FACT_EPSILON) ? EPSILONS : NO_EPSILONS;
  p |= (facts & FACT_O_EPSILON) ? O_EPSILONS : NO_O_EPSILONS;
  p |= (facts & FACT_NOT_I_SORTED) ? NOT_I_LABEL_SORTED : I_LABEL_SORTED;
  p |= (facts & FACT_NOT_O_SORTED) ? NOT_O_LABEL_SORTED : O_LABEL_SORTED;
  p |= (facts & (FACT_WEIGHTED | FACT_FINAL_WEIGHTED)) ? WEIGHTED : UNWEIGHTED;
  p |= (facts & FACT_NOT_TOP_SORTED) ? NOT_TOP_SORTED : TOP_SORTED;
  return p;
}
// set_properties_with_mask(comp, known_properties(comp)) (mutable_fst.rs:435-441, utils.rs:4-9)
inline uint64_t merge_computed(uint64_t p, uint64_t comp) {
  const uint64_t pos = 0x5555555555555555ull & ALL, neg = 0xAAAAAAAAAAAAAAAAull & ALL;
  const uint64_t known = (comp & ALL) | ((comp & pos) << 1) | ((comp & neg) >> 1);
  return (p & ~known) | comp;
}
// reverse_properties (mutate_properties.rs:622-638)
inline uint64_t reverse(uint64_t inprops, bool has_superinitial) {
  uint64_t out = (ACCEPTOR | NOT_ACCEPTOR | EPSILONS | I_EPSILONS | O_EPSILONS | UNWEIGHTED | CYCLIC | ACYCLIC |
                  WEIGHTED_CYCLES | UNWEIGHTED_CYCLES) & inprops;
  if (has_superinitial) out |= WEIGHTED & inprops;
  return out;
}

inline uint64_t delete_states(uint64_t in) { return in & DELETE_STATES_MASK; }  // :102-104
inline uint64_t compose(uint64_t p1, uint64_t p2) {                             // :151-184
  uint64_t out = 0;
  if ((p1 & ACCEPTOR) && (p2 & ACCEPTOR)) {
    out |= ACCEPTOR | ACCESSIBLE;
    out |= (NO_EPSILONS | NO_I_EPSILONS | NO_O_EPSILONS | ACYCLIC | INITIAL_ACYCLIC) & p1 & p2;
    if ((p1 & NO_I_EPSILONS) && (p2 & NO_I_EPSILONS)) out |= (I_DETERMINISTIC | O_DETERMINISTIC) & p1 & p2;
  } else {
    out |= ACCESSIBLE;
    out |= (ACCEPTOR | NO_I_EPSILONS | ACYCLIC | INITIAL_ACYCLIC) & p1 & p2;
    if ((p1 & NO_I_EPSILONS) && (p2 & NO_I_EPSILONS)) out |= I_DETERMINISTIC & p1 & p2;
  }
  return out;
}
inline uint64_t shortest_path(uint64_t p, bool tree) {  // :662-672
  uint64_t out = p | ACYCLIC | INITIAL_ACYCLIC | ACCESSIBLE | UNWEIGHTED_CYCLES;
  if (!tree) out |= COACCESSIBLE;
  return out;
}

// Property word of the linear FST single_shortest_path_backtrace builds (shortest_path.rs:241-282): state 0 final,
// state k >= 1 carries the single arc path_arcs[k-1] into state k-1, start = hops; the reference's incremental
// add_state / set_final / add_tr / set_start bookkeeping, then shortest_path_properties(.., true).
// add_tr(add_state(p), arc) is a pure function of (p, the facts the arc contributes).  Arcs are processed in
// runs of equal facts; inside a run the word reaches a fixed point after a step or two (add_state(out) == in), and
// the rest of the run is skipped — the result is exactly the incremental one.
inline uint64_t linear_path_props(bool has_path, uint32_t hops, float final_weight, const wfst_tr* path_arcs) {
  uint64_t p = NULL_PROPS;
  if (has_path) {
    p = add_state(p);
    p = set_final(p, nullptr, &final_weight);
    auto facts_of = [&](uint32_t k) { return arc_facts(path_arcs[k - 1], nullptr, k); };  // arc of state k
    uint32_t k = 1;
    while (k <= hops) {
      const uint32_t f = facts_of(k);
      uint32_t end = k;
      while (end < hops && facts_of(end + 1) == f) ++end;
      for (uint32_t j = k; j <= end; ++j) {
        const uint64_t in = add_state(p);
        p = add_tr(in, j, path_arcs[j - 1], nullptr);
        if (add_state(p) == in) break;  // fixed point: every further arc of the run maps `in` to the same `p`
      }
      k = end + 1;
    }
    p = set_start(p);
  }
  return shortest_path(p, true) & ALL;
}

// The same word from the UNION of the arcs' facts (a path's states have one arc each: no label-order facts).
// Every effect of add_tr is a sticky set / clear decided by one fact, followed by masks that are the same for every
// arc: the order of the arcs does not matter, and three applications of the union reach the fixed point.  The
// string o T kernel ORs the facts of a path's arcs while it writes them (compose.hip: Result::facts), so that the host
// does not read the arcs back to know the properties; tests/test_host.py (props_check) compares this function with
// linear_path_props on every fact sequence of up to four arcs.
constexpr uint32_t PATH_FACTS_NONE = 0xFFFFFFFFu;  // the kernel did not provide them: scan the arcs
// (arc k of a backtraced path leaves state k + 1 for state k: FACT_NOT_TOP_SORTED whatever the ids are)
WFST_HD inline uint32_t path_arc_facts(uint32_t ilabel, uint32_t olabel, float weight) {
  return arc_facts(wfst_tr{ilabel, olabel, weight, 1u}, nullptr, 0u) | FACT_NOT_TOP_SORTED;
}
inline uint64_t linear_path_props_from_facts(bool has_path, uint32_t hops, float final_weight, uint32_t facts_union) {
  uint64_t p = NULL_PROPS;
  if (has_path) {
    p = add_state(p);
    p = set_final(p, nullptr, &final_weight);
    for (uint32_t j = 0; j < (hops < 3u ? hops : 3u); ++j) p = add_trs_by_facts(add_state(p), facts_union);
    p = set_start(p);
  }
  return shortest_path(p, true) & ALL;
}

// project_properties (fst_properties/mutate_properties.rs:365-445) as applied by project() with the all_properties() mask
// (algorithms/projection.rs:91-94)
inline uint64_t project(uint64_t in, bool project_output) {
  uint64_t out = ACCEPTOR;
  out |= (WEIGHTED | UNWEIGHTED | WEIGHTED_CYCLES | UNWEIGHTED_CYCLES | CYCLIC | ACYCLIC | INITIAL_CYCLIC | INITIAL_ACYCLIC |
          TOP_SORTED | NOT_TOP_SORTED | ACCESSIBLE | NOT_ACCESSIBLE | COACCESSIBLE | NOT_COACCESSIBLE | STRING | NOT_STRING) & in;
  if (!project_output) {
    out |= (I_DETERMINISTIC | NOT_I_DETERMINISTIC | I_EPSILONS | NO_I_EPSILONS | I_LABEL_SORTED | NOT_I_LABEL_SORTED) & in;
    if (in & I_DETERMINISTIC) out |= O_DETERMINISTIC;
    if (in & NOT_I_DETERMINISTIC) out |= NOT_O_DETERMINISTIC;
    if (in & I_EPSILONS) out |= O_EPSILONS | EPSILONS;
    if (in & NO_I_EPSILONS) out |= NO_O_EPSILONS | NO_EPSILONS;
    if (in & I_LABEL_SORTED) out |= O_LABEL_SORTED;
    if (in & NOT_I_LABEL_SORTED) out |= NOT_O_LABEL_SORTED;
  } else {
    out |= (O_DETERMINISTIC | NOT_O_DETERMINISTIC | O_EPSILONS | NO_O_EPSILONS | O_LABEL_SORTED | NOT_O_LABEL_SORTED) & in;
    if (in & O_DETERMINISTIC) out |= I_DETERMINISTIC;
    if (in & NOT_O_DETERMINISTIC) out |= NOT_I_DETERMINISTIC;
    if (in & O_EPSILONS) out |= I_EPSILONS | EPSILONS;
    if (in & NO_O_EPSILONS) out |= NO_I_EPSILONS | NO_EPSILONS;
    if (in & O_LABEL_SORTED) out |= I_LABEL_SORTED;
    if (in & NOT_O_LABEL_SORTED) out |= NOT_I_LABEL_SORTED;
  }
  return (in & ~ALL) | out;
}

// invert_properties (fst_properties/mutate_properties.rs:302-363) as applied by invert() with the all_properties() mask
// (algorithms/inversion.rs:44-47): the tape-neutral pairs stay, every input-side pair changes places with its output-side one
inline uint64_t invert(uint64_t in) {
  uint64_t out = (ACCEPTOR | NOT_ACCEPTOR | EPSILONS | NO_EPSILONS | WEIGHTED | UNWEIGHTED | WEIGHTED_CYCLES | UNWEIGHTED_CYCLES |
                  CYCLIC | ACYCLIC | INITIAL_CYCLIC | INITIAL_ACYCLIC | TOP_SORTED | NOT_TOP_SORTED | ACCESSIBLE | NOT_ACCESSIBLE |
                  COACCESSIBLE | NOT_COACCESSIBLE | STRING | NOT_STRING) & in;
  if (in & I_DETERMINISTIC) out |= O_DETERMINISTIC;
  if (in & NOT_I_DETERMINISTIC) out |= NOT_O_DETERMINISTIC;
  if (in & O_DETERMINISTIC) out |= I_DETERMINISTIC;
  if (in & NOT_O_DETERMINISTIC) out |= NOT_I_DETERMINISTIC;
  if (in & I_EPSILONS) out |= O_EPSILONS;
  if (in & NO_I_EPSILONS) out |= NO_O_EPSILONS;
  if (in & O_EPSILONS) out |= I_EPSILONS;
  if (in & NO_O_EPSILONS) out |= NO_I_EPSILONS;
  if (in & I_LABEL_SORTED) out |= O_LABEL_SORTED;
  if (in & NOT_I_LABEL_SORTED) out |= NOT_O_LABEL_SORTED;
  if (in & O_LABEL_SORTED) out |= I_LABEL_SORTED;
  if (in & NOT_O_LABEL_SORTED) out |= NOT_I_LABEL_SORTED;
  return (in & ~ALL) | out;
}

// ---- reweight() / remove_weight() bookkeeping (algorithms/reweight.rs, algorithms/push.rs:150-170)
// keep_only_relevant_properties (trs_iter_mut.rs:293-305): set_arc_properties() is empty (properties.rs:278-280), so every
// set_weight_unchecked keeps the label / epsilon bits and WEIGHTED / UNWEIGHTED only
constexpr uint64_t ARC_RELEVANT = ACCEPTOR | NOT_ACCEPTOR | EPSILONS | NO_EPSILONS | I_EPSILONS | NO_I_EPSILONS | O_EPSILONS |
                                  NO_O_EPSILONS | WEIGHTED | UNWEIGHTED;
// TrsIterMut::set_weight_unchecked -> compute_new_properties_weights (trs_iter_mut.rs:210-215, 279-291, 342-350)
inline uint64_t set_weight(uint64_t in, float old_w, float new_w) {
  uint64_t out = in;
  if (weighted(old_w)) out &= ~WEIGHTED;
  if (weighted(new_w)) out = (out | WEIGHTED) & ~UNWEIGHTED;
  return out & ARC_RELEVANT;
}
// FstProperties::weight_invariant_properties (properties.rs:436-465)
constexpr uint64_t WEIGHT_INVARIANT = ACCEPTOR | NOT_ACCEPTOR | I_DETERMINISTIC | NOT_I_DETERMINISTIC | O_DETERMINISTIC |
                                      NOT_O_DETERMINISTIC | EPSILONS | NO_EPSILONS | I_EPSILONS | NO_I_EPSILONS | O_EPSILONS |
                                      NO_O_EPSILONS | I_LABEL_SORTED | NOT_I_LABEL_SORTED | O_LABEL_SORTED | NOT_O_LABEL_SORTED |
                                      CYCLIC | ACYCLIC | INITIAL_CYCLIC | INITIAL_ACYCLIC | TOP_SORTED | NOT_TOP_SORTED |
                                      ACCESSIBLE | NOT_ACCESSIBLE | COACCESSIBLE | NOT_COACCESSIBLE | STRING | NOT_STRING;
// reweight_properties (mutate_properties.rs:640-644), applied with the all_properties() mask (reweight.rs:148-151)
inline uint64_t reweight(uint64_t in) { return in & WEIGHT_INVARIANT & ~COACCESSIBLE; }
// what reweight's passes over the final weights and the arcs leave in the word (reweight.rs:46-49, 84, 101): facts & 2 = some
// final weight went through set_final, facts & 1 = some arc through set_weight_unchecked (their WEIGHTED / UNWEIGHTED
// updates are dropped by reweight() above, which ends the call)
inline uint64_t reweight_marks(uint64_t in, uint32_t facts) {
  uint64_t p = in;
  if (facts & 2u) p = set_final(p, nullptr, nullptr);
  if (facts & 1u) p = p & ARC_RELEVANT;
  return p;
}
// the trinary pairs (fst_properties/utils.rs:4-9 known_properties): a pair is known when either of its bits is set
inline bool knows(uint64_t p, uint64_t pos_bit) { return (p & (pos_bit | (pos_bit << 1))) != 0; }
// compute_and_update_properties(mask) with a mask of DFS bits only (fst_traits/mutable_fst.rs:435-441,
// compute_fst_properties.rs:13-58): the SccVisitor's word replaces the four DFS pairs, nothing else changes
constexpr uint64_t DFS_BITS = ACYCLIC | CYCLIC | INITIAL_ACYCLIC | INITIAL_CYCLIC | ACCESSIBLE | NOT_ACCESSIBLE | COACCESSIBLE |
                              NOT_COACCESSIBLE;
// SccVisitor's bits (visitors/scc_visitors.rs) from four plain facts about the graph: every state reachable from the start,
// every state reaches a final state, some cycle anywhere (the DFS also starts from unreachable states), the start on a cycle
inline uint64_t dfs_bits(bool accessible, bool coaccessible, bool cyclic, bool initial_cyclic) {
  return (accessible ? ACCESSIBLE : NOT_ACCESSIBLE) | (coaccessible ? COACCESSIBLE : NOT_COACCESSIBLE) |
         (cyclic ? CYCLIC : ACYCLIC) | (initial_cyclic ? INITIAL_CYCLIC : INITIAL_ACYCLIC);
}
inline uint64_t merge_dfs(uint64_t in, uint64_t dfs) { return (in & ~DFS_BITS) | (dfs & DFS_BITS); }

// determinize_properties(inprops, has_subsequential_label = false, distinct_psubsequential_labels)
// (mutate_properties.rs:247-279), as determinize_with_config sets it (determinize_static.rs:186-190)
inline uint64_t determinize(uint64_t in, bool distinct_psubsequential_labels) {
  uint64_t out = ACCESSIBLE;
  if ((in & ACCEPTOR) || ((in & NO_I_EPSILONS) && distinct_psubsequential_labels)) out |= I_DETERMINISTIC;
  out |= (ACCEPTOR | ACYCLIC | INITIAL_ACYCLIC | COACCESSIBLE | STRING) & in;
  if ((in & NO_I_EPSILONS) && distinct_psubsequential_labels) out |= NO_EPSILONS & in;
  if (in & ACCESSIBLE) out |= (I_EPSILONS | O_EPSILONS | CYCLIC) & in;
  if (in & ACCEPTOR) out |= (NO_I_EPSILONS | NO_O_EPSILONS) & in;
  return out;
}

// ---- minimize (algorithms/minimize.rs, tr_unique.rs:38-51): arcsort_properties() (properties.rs:351-381) = everything
// but the four label-order bits; delete_arcs_properties() (:300-316)
constexpr uint64_t ARCSORT_MASK = ALL & ~(I_LABEL_SORTED | NOT_I_LABEL_SORTED | O_LABEL_SORTED | NOT_O_LABEL_SORTED);
constexpr uint64_t DELETE_ARCS_MASK = ACCEPTOR | I_DETERMINISTIC | O_DETERMINISTIC | NO_EPSILONS | NO_I_EPSILONS |
                                      NO_O_EPSILONS | I_LABEL_SORTED | O_LABEL_SORTED | UNWEIGHTED | ACYCLIC |
                                      INITIAL_ACYCLIC | TOP_SORTED | NOT_ACCESSIBLE | NOT_COACCESSIBLE | UNWEIGHTED_CYCLES;

// ---- the rational operations (algorithms/{union,concat,closure}), all with delayed = false
// closure_properties (mutate_properties.rs:114-145)
inline uint64_t closure(uint64_t in) {
  uint64_t out = (ACCEPTOR | UNWEIGHTED | ACCESSIBLE) & in;
  if (in & UNWEIGHTED) out |= UNWEIGHTED_CYCLES;
  out |= (COACCESSIBLE | NOT_TOP_SORTED | NOT_STRING) & in;
  out |= (NOT_ACCEPTOR | NOT_I_DETERMINISTIC | NOT_O_DETERMINISTIC | NOT_I_LABEL_SORTED | NOT_O_LABEL_SORTED | WEIGHTED |
          WEIGHTED_CYCLES | NOT_ACCESSIBLE | NOT_COACCESSIBLE) & in;
  if ((in & WEIGHTED) && (in & ACCESSIBLE) && (in & COACCESSIBLE)) out |= WEIGHTED_CYCLES;
  return out;
}
// what both operands hand on unless a condition below says otherwise (mutate_properties.rs:207-220, 717-729)
constexpr uint64_t RATIONAL_NEGATIVE = NOT_ACCEPTOR | NOT_I_DETERMINISTIC | NOT_O_DETERMINISTIC | EPSILONS | I_EPSILONS |
                                       O_EPSILONS | NOT_I_LABEL_SORTED | NOT_O_LABEL_SORTED | WEIGHTED | WEIGHTED_CYCLES |
                                       CYCLIC | NOT_ACCESSIBLE;
// concat_properties (mutate_properties.rs:186-245)
inline uint64_t concat(uint64_t p1, uint64_t p2) {
  uint64_t out = (ACCEPTOR | UNWEIGHTED | UNWEIGHTED_CYCLES | ACYCLIC) & p1 & p2;
  out |= (NOT_TOP_SORTED | NOT_STRING) & p1;
  out |= (NOT_TOP_SORTED | NOT_STRING) & p2;
  out |= (INITIAL_ACYCLIC | INITIAL_CYCLIC) & p1;
  out |= (RATIONAL_NEGATIVE | NOT_COACCESSIBLE) & p1;
  if ((p1 & ACCESSIBLE) && (p1 & COACCESSIBLE)) {
    out |= (ACCESSIBLE | COACCESSIBLE) & p2;
    out |= (RATIONAL_NEGATIVE | NOT_COACCESSIBLE) & p2;
  }
  return out;
}
// union_properties (mutate_properties.rs:692-748)
inline uint64_t union_(uint64_t p1, uint64_t p2) {
  uint64_t out = (ACCEPTOR | UNWEIGHTED | UNWEIGHTED_CYCLES | ACYCLIC | ACCESSIBLE) & p1 & p2;
  out |= INITIAL_ACYCLIC;
  out |= NOT_TOP_SORTED & p1;
  out |= NOT_TOP_SORTED & p2;
  out |= EPSILONS | I_EPSILONS | O_EPSILONS;
  out |= COACCESSIBLE & p1 & p2;
  out |= RATIONAL_NEGATIVE & p1;  // (NOT_COACCESSIBLE of the first operand does not hold: the INITIAL_ACYCLIC branch, :715)
  out |= (RATIONAL_NEGATIVE | NOT_COACCESSIBLE) & p2;
  return out;
}

inline uint64_t compose_result(uint64_t p1, uint64_t p2, bool connected, bool has_start) {
  // start None: LazyFst::compute returns F2::new() untouched (lazy_fst.rs:229-232)
  uint64_t p = has_start ? compose(p1, p2) : NULL_PROPS;
  if (connected) {
    p = delete_states(p);
    p |= ACCESSIBLE | COACCESSIBLE;
  }
  return p;
}

}  // namespace wfst::props
