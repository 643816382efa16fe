// replace.hip — replace (recursive transition networks) on the wide driver of compose_wide.h: a NEW handle, bit for bit
// what rustfst::algorithms::replace (replace/replace_static.rs:44-58) returns for the two-argument options
// ReplaceFstOptions::new(root, epsilon_on_replace) (replace/config.rs:22-36).
//
// ReplaceFst::compute() is LazyFst::compute (lazy/lazy_fst.rs:226-269) over ReplaceFstOp (replace/replace_fst_op.rs): a FIFO
// BFS whose state ids are the first-touch order of StateTable::find_id on tuples (prefix_id, fst_id, fst_state) — the
// numbering the wide driver reproduces.  ReplacePolicy supplies compute_trs (:76-100) and compute_final_weight (:102-113):
//   tuple words  lo = fst_id << 32 | fst_state, hi = prefix_id;
//   item 0       the return arc of compute_final_tr (:258-302), item j the j-th stored arc through compute_tr (:323-370);
//   every item emits 0 or 1 arc, nothing is staged (n_se = 0).
// The call stacks ("prefixes", replace/state_table.rs:10-31) live in a table of the policy's own: a prefix is its parent
// prefix plus one frame (caller fst_id, nextstate), interned by find-or-insert under the key (parent, fst_id, nextstate).
// Its id is its slot + 1; id 0 is the empty stack, which compute_start interns first in the reference as well.  Prefix ids
// never reach the result, which depends only on WHICH stacks are equal.
//
// The reference has no CyclicDependencies check: on a grammar whose expansion reaches a recursive call compute() never
// returns.  A frame names its CALLER, and a callee is entered at its start state whatever the stack, so the expansion is
// infinite iff some stack names one caller twice, and that happens iff a prefix with more frames than there are possible
// callers — the list positions the labels name, a shadowed entry is never entered — is created.  Every
// prefix carries its depth; creating one that deep raises a sticky flag, after which states expand to nothing and the
// search ends within a level.
#include "compose_wide.h"
#include "fst_props.h"

namespace wfst {
namespace {

constexpr uint32_t NO_START = 0xFFFFFFFFu;
enum : uint32_t { RP_CYCLIC = 1u, RP_PREFIX_FULL = 2u };                                                // RpCtl::flags
enum : uint32_t { RP_FLAGS = 0, RP_PREFIXES, RP_DEPTH, RP_CALLS, RP_DROPPED, RP_RETURNS, RP_WORDS = 8 };  // words of RpCtl
constexpr uint32_t RP_MAX_PROBES = 128;  // the table is at most half full: chains of tens at most

struct RpView {  // one entry of the list, by list position
  const wfst_tr* arcs;
  const uint4* srec;  // {arc begin, arc count, final bits, epsilon facts}
  uint32_t start;     // NO_START: no start state
  uint32_t pad;
};

struct RpExpand {
  const wfst_tr* it_arcs;
  const wfst_tr* se_arcs;
  uint32_t n_it, n_se;
  float final_weight;
  uint32_t fst_id, prefix, depth;        // the tuple, and how many frames its stack holds
  uint32_t ret_fst, ret_state, ret_prefix;  // top frame and popped prefix (prefix > 0)
  float fin;                              // Some(final weight) of the FST state, INF = None
  bool dead;                              // a sticky flag is up: the state expands to nothing
  uint32_t seen_to;  // items this lane has evaluated so far: the driver walks them twice, the counters count the first walk
};

// one add per wave for the lanes (of those that are here together) whose `pred` holds
__device__ __forceinline__ void wave_count(uint32_t* ctr, bool pred) {
  const uint64_t m = __ballot(pred);
  if (pred && lanes_below(m) == 0) atomicAdd(ctr, (uint32_t)__popcll(m));
}

struct ReplacePolicy {
  const RpView* views;      // [n]
  const uint32_t* keys;     // [n_keys] the labels of the list, ascending and distinct (nonterminal_set)
  const uint32_t* key_fst;  // [n_keys] the LAST list position with that label (nonterminal_hash.insert overwrites)
  uint32_t n_keys;  // = the FSTs that can ever be entered, and so be callers: the root and whatever a label names last
  uint32_t eps_on_call;  // call arcs are 0:0 (epsilon_on_replace) or ilabel:0
  // prefix table, open addressing: p_lo = parent prefix << 32 | caller fst_id (K_EMPTY: free), p_hi = depth << 32 |
  // nextstate (KHI_UNSET until the slot's winner has written it).  The depth is a function of the key.
  uint64_t* p_lo;
  uint64_t* p_hi;
  uint32_t p_mask;  // slots - 1
  uint32_t* ctl;    // RP_WORDS words
  using Expand = RpExpand;

  __device__ Expand make_expand(uint64_t tlo, uint64_t thi) const {
    Expand x;
    x.se_arcs = nullptr;
    x.n_se = 0;
    x.seen_to = 0;
    x.fst_id = (uint32_t)(tlo >> 32);
    x.prefix = (uint32_t)thi;
    x.depth = 0;
    x.ret_fst = x.ret_state = x.ret_prefix = 0;
    // (a flag raised while this level runs is seen by the next one at the latest: what is emitted meanwhile is valid)
    x.dead = ld_l2(&ctl[RP_FLAGS]) != 0u;
    const uint4 r = views[x.fst_id].srec[(uint32_t)tlo];
    x.it_arcs = views[x.fst_id].arcs + r.x;
    x.n_it = x.dead ? 0u : r.y;
    x.fin = __uint_as_float(r.z);
    x.final_weight = x.prefix == 0u ? x.fin : INF;  // compute_final_weight :102-113: only the root instance is final
    if (x.prefix) {  // (interned by an earlier launch: plain loads)
      const uint64_t lo = p_lo[x.prefix - 1], hi = p_hi[x.prefix - 1];
      x.ret_prefix = (uint32_t)(lo >> 32);
      x.ret_fst = (uint32_t)lo;
      x.ret_state = (uint32_t)hi;
      x.depth = (uint32_t)(hi >> 32);
    }
    return x;
  }

  // find_id of the stack `parent` + (fst, ns) (push_prefix :313-321): slot + 1, or 0 when the table is full (RP_PREFIX_FULL
  // is up then).  Idempotent, and safe when lanes of one wave and of many waves intern one key at once: the loop is uniform
  // over the lanes that are here together, the winner of a slot writes its second word inside the iteration it won in, and
  // a lane that meets a slot whose second word is not there yet tries the same slot again on the next iteration.
  __device__ uint32_t intern(uint32_t parent, uint32_t fst, uint32_t ns, uint32_t depth) const {
    const uint64_t klo = ((uint64_t)parent << 32) | fst, khi = ((uint64_t)depth << 32) | ns;
    uint32_t slot = hash_128(klo, ns) & p_mask, probes = 0, id = 0;
    bool done = false, new_one = false;
    while (__any(!done)) {
      uint64_t prev = 0;
      if (!done) prev = atomicCAS((unsigned long long*)&p_lo[slot], (unsigned long long)K_EMPTY, (unsigned long long)klo);
      const bool won = !done && prev == K_EMPTY;
      if (won) st_l2(&p_hi[slot], khi);
      const bool same_lo = !done && !won && prev == klo;
      uint64_t h = KHI_UNSET;
      if (same_lo) h = ld_l2(&p_hi[slot]);
      if (won || (same_lo && h == khi)) {
        done = true;
        new_one = won;
        id = slot + 1;
      } else if (!done && !(same_lo && h == KHI_UNSET)) {
        slot = (slot + 1) & p_mask;
        if (++probes > min(RP_MAX_PROBES, p_mask)) {
          atomicOr(&ctl[RP_FLAGS], (uint32_t)RP_PREFIX_FULL);
          done = true;
        }
      }
    }
    // (a key is won once in the life of a table, however often its level is emitted: these count prefixes)
    const uint64_t m = __ballot(new_one);
    if (new_one && lanes_below(m) == 0) {
      const uint32_t n_new = (uint32_t)__popcll(m);
      if (atomicAdd(&ctl[RP_PREFIXES], n_new) + n_new > (p_mask + 1) / 2) atomicOr(&ctl[RP_FLAGS], (uint32_t)RP_PREFIX_FULL);
    }
    if (new_one && depth > ld_l2(&ctl[RP_DEPTH])) atomicMax(&ctl[RP_DEPTH], depth);
    return id;
  }

  __device__ bool is_call(uint32_t olabel, uint32_t* callee) const {  // compute_tr :324-334
    if (olabel == 0u || olabel < keys[0] || olabel > keys[n_keys - 1]) return false;
    uint32_t lo = 0, hi = n_keys;
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (keys[mid] < olabel) lo = mid + 1; else hi = mid;
    }
    if (lo == n_keys || keys[lo] != olabel) return false;
    *callee = key_fst[lo];
    return true;
  }

  __device__ uint32_t eval_item(Expand& x, uint32_t j, bool write, uint32_t write_pos, wfst_tr* arcs, uint64_t* a_lo,
                                uint64_t* a_hi, Emitted* first) const {
    if (x.dead) return 0u;
    const bool first_walk = j >= x.seen_to;  // (a lane's items ascend within a walk)
    if (first_walk) x.seen_to = j + 1;
    uint4 arc = make_uint4(0u, 0u, 0u, 0u);
    uint64_t dlo = 0, dhi = 0;
    bool emit = false, call = false, dropped = false;
    if (j == 0) {  // compute_final_tr :258-302: 0:0 / final weight into (popped prefix, top.fst_id, top.nextstate)
      emit = x.prefix != 0u && x.fin != INF;
      arc.z = __float_as_uint(x.fin);
      dlo = ((uint64_t)x.ret_fst << 32) | x.ret_state;
      dhi = x.ret_prefix;
    } else {
      const ArcReg a = load_arc(x.it_arcs + (j - 1));
      uint32_t callee = 0;
      if (!is_call(a.ol, &callee)) {  // copied into the same instance
        emit = true;
        arc = make_uint4(a.il, a.ol, __float_as_uint(a.w), 0u);
        dlo = ((uint64_t)x.fst_id << 32) | a.ns;
        dhi = x.prefix;
      } else if (x.depth + 1 > n_keys) {  // more frames than possible callers: one is there twice, the expansion does not end
        atomicOr(&ctl[RP_FLAGS], (uint32_t)RP_CYCLIC);
      } else {
        const uint32_t id = intern(x.prefix, x.fst_id, a.ns, x.depth + 1);  // the prefix is created before the start is asked for
        const uint32_t start = views[callee].start;
        dropped = id != 0u && start == NO_START;  // (:337-360) no arc, no tuple
        call = emit = id != 0u && start != NO_START;
        arc = make_uint4(eps_on_call ? 0u : a.il, 0u, __float_as_uint(a.w), 0u);
        dlo = ((uint64_t)callee << 32) | start;
        dhi = id;
      }
    }
    wave_count(&ctl[RP_RETURNS], first_walk && emit && j == 0);
    wave_count(&ctl[RP_CALLS], first_walk && call);
    wave_count(&ctl[RP_DROPPED], first_walk && dropped);
    if (!emit) return 0u;
    if (write) {
      *reinterpret_cast<uint4*>(arcs + write_pos) = arc;
      a_lo[write_pos] = dlo;
      a_hi[write_pos] = dhi;
    } else if (first) {
      first->arc = arc;
      first->lo = dlo;
      first->hi = dhi;
    }
    return 1u;
  }
};

// replace_properties of replace_fst_op.rs:120-186 over the STORED words, for ReplaceFstOptions::new(root, eps): the call
// label type is Neither (eps) or Input, the return label type Neither, call_output_label Some(0) (eps) or None — as the
// options give them, before the constructor's overrides (:227-235)
uint64_t replace_word(const uint32_t* labels, const wfst_fst* const* fsts, size_t n, uint32_t root_label, bool eps) {
  using namespace props;
  bool all_ilabel_sorted = true, all_olabel_sorted = true, all_non_empty = true, dense_range = true;
  size_t root = 0;
  for (size_t i = 0; i < n; ++i) {
    if ((uint64_t)labels[i] > (uint64_t)n) dense_range = false;
    if (labels[i] == root_label) root = i;
    if (fsts[i]->start < 0) all_non_empty = false;
    if (!(fsts[i]->props & I_LABEL_SORTED)) all_ilabel_sorted = false;
    if (!(fsts[i]->props & O_LABEL_SORTED)) all_olabel_sorted = false;
  }
  // epsilon_on_input / epsilon_on_output (replace/utils.rs:4-10) of the two label types, replace_transducer (:188-198)
  const bool epsilon_on_call = eps, epsilon_on_return = true, out_epsilon_on_call = true, out_epsilon_on_return = true;
  const bool transducer = !eps;
  const bool all_negative_or_dense = dense_range;  // (labels are unsigned: all_negative is false)
  // mutate_properties.rs:496-620
  uint64_t out = 0;
  uint64_t access = all_non_empty ? (ACCESSIBLE | COACCESSIBLE) : 0;
  for (size_t i = 0; i < n; ++i) access &= fsts[i]->props & (ACCESSIBLE | COACCESSIBLE);
  if (access == (ACCESSIBLE | COACCESSIBLE)) {
    out |= access;
    if (fsts[root]->props & INITIAL_CYCLIC) out |= INITIAL_CYCLIC;
    uint64_t p = 0;
    bool string = true;
    for (size_t i = 0; i < n; ++i) {
      const uint64_t in = fsts[i]->props;
      if (transducer) p |= NOT_ACCEPTOR & in;
      p |= (NOT_I_DETERMINISTIC | NOT_O_DETERMINISTIC | EPSILONS | I_EPSILONS | O_EPSILONS | WEIGHTED | WEIGHTED_CYCLES | CYCLIC |
            NOT_TOP_SORTED | NOT_STRING) & in;
      if (!(in & STRING)) string = false;
    }
    out |= p;
    if (string) out |= STRING;
  }
  bool acceptor = !transducer, ideterministic = !epsilon_on_call && epsilon_on_return;
  bool no_iepsilons = !epsilon_on_call && !epsilon_on_return, acyclic = true, unweighted = true;
  for (size_t i = 0; i < n; ++i) {
    const uint64_t in = fsts[i]->props;
    if (!(in & ACCEPTOR)) acceptor = false;
    if (!(in & I_DETERMINISTIC)) ideterministic = false;
    if (!(in & NO_I_EPSILONS)) no_iepsilons = false;
    if (!(in & ACYCLIC)) acyclic = false;
    if (!(in & UNWEIGHTED)) unweighted = false;
    if (i != root && !(in & NO_I_EPSILONS)) ideterministic = false;
  }
  if (acceptor) out |= ACCEPTOR;
  if (ideterministic) out |= I_DETERMINISTIC;
  if (no_iepsilons) out |= NO_I_EPSILONS;
  if (acyclic) out |= ACYCLIC;
  if (unweighted) out |= UNWEIGHTED;
  if (fsts[root]->props & INITIAL_ACYCLIC) out |= INITIAL_ACYCLIC;
  if (all_ilabel_sorted && epsilon_on_return && (!epsilon_on_call || all_negative_or_dense)) out |= I_LABEL_SORTED;
  if (all_olabel_sorted && out_epsilon_on_return && (!out_epsilon_on_call || all_negative_or_dense)) out |= O_LABEL_SORTED;
  return out;  // set_properties stores the word as it is (vector_fst/mutable_fst.rs:407-409)
}

// WFST_REPLACE_PREFIX_SLOTS (tests): the slots the prefix table starts with, a power of two >= 2
uint32_t prefix_slots_knob() {
  const char* e = std::getenv("WFST_REPLACE_PREFIX_SLOTS");
  if (!e || !*e) return 0;
  char* end = nullptr;
  const long v = std::strtol(e, &end, 10);
  if (*end || v < 2 || v > (1l << 30) || (v & (v - 1))) throw Error("replace: WFST_REPLACE_PREFIX_SLOTS must be a power of two in [2, 2^30]");
  return (uint32_t)v;
}

}  // namespace

wfst_fst* replace_fst(wfst_ctx* ctx, uint32_t root_label, const uint32_t* labels, const wfst_fst* const* fsts, size_t n,
                      bool epsilon_on_replace) {
  ctx->replace = wfst_ctx::ReplaceStats{};
  for (size_t i = 0; i < n; ++i) {
    if (fsts[i]->device != ctx->device) throw Error("replace: item " + std::to_string(i) + " lives on another device");
    if (fsts[i]->ctx != ctx) throw Error("replace: item " + std::to_string(i) + " belongs to another context");
  }
  size_t root = n;
  for (size_t i = 0; i < n; ++i)
    if (labels[i] == root_label) root = i;  // (the last one: nonterminal_hash.insert overwrites, replace_fst_op.rs:237-253)
  if (root == n)
    throw Error("ReplaceFstImpl: No FST corresponding to root label " + std::to_string(root_label) + " in the input tuple vector");
  if (n > 0x7FFFFFFFull) throw Error("replace: more than 2^31 - 1 list entries");
  const uint32_t slots_knob = prefix_slots_knob();
  if (fsts[root]->start < 0) {  // compute_start -> None: LazyFst::compute returns F2::new() untouched (lazy_fst.rs:229-232)
    HostCsr h;
    h.offsets.push_back(0);
    return make_host_fst(ctx, 0, -1, props::NULL_PROPS, std::move(h));
  }
  const uint64_t word = replace_word(labels, fsts, n, root_label, epsilon_on_replace);

  hipStream_t st = ctx->stream;
  std::vector<RpView> views(n);
  uint64_t sum_states = 0, sum_arcs = 0;
  for (size_t i = 0; i < n; ++i) {
    ensure_device(const_cast<wfst_fst*>(fsts[i]));
    views[i] = RpView{fsts[i]->dev.arcs, fsts[i]->dev.srec, fsts[i]->start < 0 ? NO_START : (uint32_t)fsts[i]->start, 0u};
    sum_states += fsts[i]->n_states;
    sum_arcs += fsts[i]->n_arcs;
  }
  std::vector<std::pair<uint32_t, uint32_t>> by_label(n);
  for (size_t i = 0; i < n; ++i) by_label[i] = {labels[i], (uint32_t)i};
  std::sort(by_label.begin(), by_label.end());
  std::vector<uint32_t> keys, key_fst;
  for (size_t i = 0; i < n; ++i) {
    if (i + 1 < n && by_label[i + 1].first == by_label[i].first) continue;  // of equal labels the last list position
    keys.push_back(by_label[i].first);
    key_fst.push_back(by_label[i].second);
  }
  DBuf<RpView> d_views(*ctx->pool, n);
  DBuf<uint32_t> d_keys(*ctx->pool, 2 * keys.size()), d_ctl(*ctx->pool, RP_WORDS);
  HIP_CHECK(hipMemcpyAsync(d_views.p, views.data(), n * sizeof(RpView), hipMemcpyHostToDevice, st));
  HIP_CHECK(hipMemcpyAsync(d_keys.p, keys.data(), keys.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  HIP_CHECK(hipMemcpyAsync(d_keys.p + keys.size(), key_fst.data(), keys.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  HIP_CHECK(hipStreamSynchronize(st));  // (the three host vectors may go)

  // A prefix per call site that is reached: the inputs' arcs bound the call sites of one instance, the instances multiply
  // them.  The table is cleared before every attempt, so it starts small: two slots per input arc (it is kept half full
  // at most: one prefix per arc), 128 k slots at least and 4 M at most (64 MiB, 16 bytes a slot); a table that fills up is
  // doubled and the expansion runs again from the start state.
  uint64_t slots = slots_knob ? slots_knob : wide_next_pow2(std::min<uint64_t>(std::max<uint64_t>(1ull << 17, 2 * sum_arcs), 1ull << 22));
  const double items = 1.0 + (double)sum_arcs / (double)std::max<uint64_t>(sum_states, 1);
  const WideWho who{"replace", "result", &ctx->replace.arena_grows};
  for (;;) {
    DBuf<uint64_t> d_prefix(*ctx->pool, 2 * slots);
    HIP_CHECK(hipMemsetAsync(d_prefix.p, 0xFF, 2 * slots * sizeof(uint64_t), st));  // K_EMPTY, KHI_UNSET
    HIP_CHECK(hipMemsetAsync(d_ctl.p, 0, RP_WORDS * sizeof(uint32_t), st));
    const ReplacePolicy pol{d_views.p, d_keys.p, d_keys.p + keys.size(), (uint32_t)keys.size(), epsilon_on_replace ? 1u : 0u,
                            d_prefix.p, d_prefix.p + slots, (uint32_t)(slots - 1), d_ctl.p};
    WideOutput w;
    run_wide(ctx, pol, ((uint64_t)root << 32) | (uint32_t)fsts[root]->start, 0ull, 2 * sum_states, 0, items, w, who);
    ctx->replace.level_launches += w.n_level_launches;
    uint32_t* hc = (uint32_t*)ctx->pinned.get(RP_WORDS * sizeof(uint32_t));  // (the driver's staging block is free again)
    HIP_CHECK(hipMemcpyAsync(hc, d_ctl.p, RP_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (hc[RP_FLAGS] & RP_CYCLIC)
      throw Error("replace: cyclic dependency between the FSTs: the reference does not terminate on this input");
    if (hc[RP_FLAGS] & RP_PREFIX_FULL) {
      ctx->replace.prefix_reruns++;
      if (slots >= (1ull << 30)) throw Error("replace: more than 2^29 call stacks");
      slots *= 2;
      continue;
    }
    ctx->replace.levels = w.n_levels;
    ctx->replace.states = w.n_states;
    ctx->replace.arcs = w.n_arcs;
    ctx->replace.prefixes = hc[RP_PREFIXES];
    ctx->replace.max_depth = hc[RP_DEPTH];
    ctx->replace.call_arcs = hc[RP_CALLS];
    ctx->replace.dropped_calls = hc[RP_DROPPED];
    ctx->replace.return_arcs = hc[RP_RETURNS];
    return adopt_device(ctx, w.n_states, w.n_arcs, 0, word, w.off, w.arcs, w.fin);
  }
}

}  // namespace wfst
