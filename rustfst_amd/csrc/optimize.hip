// optimize.hip — algorithms::optimize (rustfst/src/algorithms/optimize.rs:11-128) for the tropical semiring (IDEMPOTENT),
// driving the device stages on handles: rm_epsilon, tr_sum, determinize, minimize, and for transducers the label
// encode / decode of encode/encode_static.rs, decode_static.rs, table.rs (EncodeLabels).  Every branch is taken on the STORED
// property word, as the reference does.  Branch table (word after tr_sum; UNWEIGHTED and UNWEIGHTED_CYCLES never survive
// tr_sum's weight_invariant mask, so `intersects(ACYCLIC | UNWEIGHTED | UNWEIGHTED_CYCLES)` is `contains(ACYCLIC)`):
//   I_DETERMINISTIC                      minimize (its KO answers pass through unchanged)
//   no I_DETERMINISTIC, ACYCLIC, acc.    determinize, minimize
//   no I_DETERMINISTIC, ACYCLIC, trans.  encode(EncodeLabels), determinize, minimize, decode
//   no I_DETERMINISTIC, no ACYCLIC       KO (the reference encodes the weights and ends in the cyclic minimizer)
// encode   label = 1 + index of the first occurrence of the arc's (ilabel, olabel) pair in tr_map's scan order, which is
//          the CSR order: a device hash set of the pairs, atomicMin of the arc index per pair (the scheme of
//          minimize.hip's tuple_kernel), first occurrences flagged and scanned into DENSE ids.
// decode   a gather of the pair through the table, then rm_final_epsilon: the machine holds no eps:eps arc (labels >= 1
//          decode to pairs of an epsilon-free FST), so only its closing connect acts.
// The encoded machine is determinized by the ACCEPTOR construction although its word lacks ACCEPTOR and the reference
// takes the gallic one: DESIGN.md §3.10 shows the two results are identical on a label-encoded machine.
// optimize_batch (wfst_optimize_batch) takes the same branches for a list, every stage as one batch call over the sublist
// that needs it; transducers still take encode_deter_mini_decode one by one.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "batch_driver.h"
#include "common.h"
#include "fst_props.h"

namespace wfst {

namespace {

constexpr uint32_t TPB = 256;
constexpr uint64_t EMPTY_KEY = ~0ull;
constexpr float KSHORTESTDELTA = 1e-6f;

// i_label_invariant_properties() & o_label_invariant_properties() (properties.rs:383-432)
constexpr uint64_t LABEL_INVARIANT = props::WEIGHTED | props::UNWEIGHTED | props::CYCLIC | props::ACYCLIC | props::INITIAL_CYCLIC |
                                     props::INITIAL_ACYCLIC | props::TOP_SORTED | props::NOT_TOP_SORTED | props::ACCESSIBLE |
                                     props::NOT_ACCESSIBLE | props::COACCESSIBLE | props::NOT_COACCESSIBLE | props::STRING |
                                     props::NOT_STRING | props::WEIGHTED_CYCLES | props::UNWEIGHTED_CYCLES;

// the pair of arc p into an open-addressing set (EMPTY_KEY = free); minpos[slot] = the first arc that holds the pair
__global__ void __launch_bounds__(TPB) enc_insert_kernel(const wfst_tr* __restrict__ arcs, uint32_t n_arcs,
                                                         unsigned long long* __restrict__ keys, uint32_t mask,
                                                         uint32_t* __restrict__ minpos, uint32_t* __restrict__ slot_of,
                                                         uint32_t* __restrict__ err) {
  for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n_arcs; p += gridDim.x * blockDim.x) {
    const uint64_t key = ((uint64_t)arcs[p].ilabel << 32) | arcs[p].olabel;
    if (key == EMPTY_KEY) {  // the pair (2^32 - 1, 2^32 - 1) is the free mark
      atomicOr(err, 1u);
      slot_of[p] = 0;
      continue;
    }
    uint32_t i = (uint32_t)mix64(key) & mask;
    for (;;) {
      unsigned long long cur = __hip_atomic_load(&keys[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (cur == EMPTY_KEY) cur = atomicCAS(&keys[i], (unsigned long long)EMPTY_KEY, (unsigned long long)key);
      if (cur == EMPTY_KEY || cur == key) break;
      i = (i + 1) & mask;
    }
    atomicMin(&minpos[i], p);
    slot_of[p] = i;
  }
}
// first[p] = arc p is the first occurrence of its pair (first[n_arcs] = 0 closes the scan)
__global__ void enc_first_kernel(const uint32_t* __restrict__ minpos, const uint32_t* __restrict__ slot_of, uint32_t n_arcs,
                                 uint32_t* __restrict__ first) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p <= n_arcs) first[p] = (p < n_arcs && minpos[slot_of[p]] == p) ? 1u : 0u;
}
// both labels become 1 + the rank of the pair's first occurrence; the first occurrence files the pair in the table
__global__ void enc_label_kernel(const wfst_tr* __restrict__ arcs, uint32_t n_arcs, const uint32_t* __restrict__ minpos,
                                 const uint32_t* __restrict__ slot_of, const uint32_t* __restrict__ rank,
                                 wfst_tr* __restrict__ enc, uint2* __restrict__ table) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_arcs) return;
  const wfst_tr a = arcs[p];
  const uint32_t fp = minpos[slot_of[p]];
  const uint32_t id = rank[fp];
  if (fp == p) table[id] = make_uint2(a.ilabel, a.olabel);
  enc[p] = wfst_tr{id + 1u, id + 1u, a.weight, a.nextstate};
}
__global__ void dec_label_kernel(const wfst_tr* __restrict__ arcs, uint32_t n_arcs, const uint2* __restrict__ table,
                                 uint32_t n_pairs, wfst_tr* __restrict__ out, uint32_t* __restrict__ err) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_arcs) return;
  const wfst_tr a = arcs[p];
  if (a.ilabel == 0u || a.ilabel > n_pairs) {  // "Can't decode ilabel" (decode_static.rs:31-37)
    atomicOr(err, 1u);
    out[p] = a;
    return;
  }
  const uint2 t = table[a.ilabel - 1u];
  if (t.x == 0u && t.y == 0u) atomicOr(err, 2u);  // an eps:eps arc survived: the word said NO_EPSILONS and the content did not
  out[p] = wfst_tr{t.x, t.y, a.weight, a.nextstate};
}

// encode(EncodeLabels), determinize, minimize, decode (optimize.rs:36-50) of the transducer x
wfst_fst* encode_deter_mini_decode(wfst_ctx* ctx, const wfst_fst* x) {
  using namespace props;
  hipStream_t st = ctx->stream;
  DevicePool& pool = *ctx->pool;
  const uint32_t n = x->n_states;
  const uint64_t E = x->n_arcs;
  if (E >= (1ull << 31)) throw Error("optimize: input too large");
  const bool mapped = x->start >= 0;  // tr_map returns at once without a start state (tr_map.rs:86-88): no labels, no mask
  DBuf<uint2> table(pool, E);
  uint32_t n_pairs = 0;
  Handle enc;
  if (mapped && E) {
    const uint32_t size = pow2_at_least(2 * E, "optimize");
    DBuf<unsigned long long> keys(pool, size);
    DBuf<uint32_t> minpos(pool, size), slot_of(pool, E), first(pool, E + 1), rank(pool, E + 1), err(pool, 1);
    DBuf<wfst_tr> arcs(pool, E);
    HIP_CHECK(hipMemsetAsync(keys.p, 0xFF, (size_t)size * sizeof(unsigned long long), st));
    HIP_CHECK(hipMemsetAsync(minpos.p, 0xFF, (size_t)size * sizeof(uint32_t), st));
    HIP_CHECK(hipMemsetAsync(err.p, 0, sizeof(uint32_t), st));
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((E + TPB - 1) / TPB, (uint64_t)ctx->n_cus * 32);
    enc_insert_kernel<<<blocks, TPB, 0, st>>>(x->dev.arcs, (uint32_t)E, keys.p, size - 1, minpos.p, slot_of.p, err.p);
    HIP_CHECK(hipGetLastError());
    if (read_u32(ctx, err.p)) throw Error("optimize: the label pair (4294967295, 4294967295) is not supported");
    enc_first_kernel<<<(uint32_t)((E + 1 + TPB - 1) / TPB), TPB, 0, st>>>(minpos.p, slot_of.p, (uint32_t)E, first.p);
    HIP_CHECK(hipGetLastError());
    const DBuf<uint8_t> scan_tmp = exclusive_scan_u32(ctx, first.p, rank.p, (size_t)E + 1);
    enc_label_kernel<<<(uint32_t)((E + TPB - 1) / TPB), TPB, 0, st>>>(x->dev.arcs, (uint32_t)E, minpos.p, slot_of.p, rank.p, arcs.p,
                                                                     table.p);
    HIP_CHECK(hipGetLastError());
    n_pairs = read_u32(ctx, rank.p + E);
    enc.reset(adopt_device(ctx, n, E, x->start, x->props & LABEL_INVARIANT, x->dev.offsets, arcs.p, x->dev.finals));
  } else {
    enc.reset(adopt_device(ctx, n, E, x->start, mapped ? (x->props & LABEL_INVARIANT) : x->props, x->dev.offsets, x->dev.arcs,
                           x->dev.finals));
  }
  // determinize: the acceptor construction with the gallic call's word
  Handle det(determinize_encoded_fst(ctx, enc.get(), KDELTA, /*Functional*/ 0u));
  enc.reset();
  Handle mini(minimize_fst(ctx, det.get(), KSHORTESTDELTA, false));
  det.reset();
  // decode: tr_map(DecodeMapper), then rm_final_epsilon = connect (connect.rs:61-64)
  ensure_device(mini.get());
  const uint64_t M = mini->n_arcs;
  uint64_t p = mini->props;
  if (mini->start >= 0) p &= LABEL_INVARIANT;
  p = (delete_states(p) & ~(ACCESSIBLE | NOT_ACCESSIBLE | COACCESSIBLE | NOT_COACCESSIBLE)) | ACCESSIBLE | COACCESSIBLE;
  DBuf<wfst_tr> dec(pool, M);
  if (mini->start >= 0 && M) {
    DBuf<uint32_t> err(pool, 1);
    HIP_CHECK(hipMemsetAsync(err.p, 0, sizeof(uint32_t), st));
    dec_label_kernel<<<(uint32_t)((M + TPB - 1) / TPB), TPB, 0, st>>>(mini->dev.arcs, (uint32_t)M, table.p, n_pairs, dec.p, err.p);
    HIP_CHECK(hipGetLastError());
    const uint32_t bad = read_u32(ctx, err.p);
    if (bad & 1u) throw Error("optimize: can't decode a label of the minimized machine");
    // rm_final_epsilon would fold such an arc into a final weight; only its closing connect is implemented
    if (bad & 2u) throw Error("optimize: eps:eps arcs under a property word that holds NO_EPSILONS are not supported");
  } else if (M) {
    HIP_CHECK(hipMemcpyAsync(dec.p, mini->dev.arcs, M * sizeof(wfst_tr), hipMemcpyDeviceToDevice, st));
  }
  return connect_and_adopt(ctx, mini->n_states, mini->start, mini->dev.offsets, dec.p, mini->dev.finals, /*all_accessible=*/false, p);
}

}  // namespace

// optimize (optimize.rs:11-128): a NEW handle; every intermediate handle is destroyed on every exit
wfst_fst* optimize_fst(wfst_ctx* ctx, const wfst_fst* f) {
  using namespace props;
  const bool acceptor = (f->props & ACCEPTOR) != 0;  // optimize_acceptor / optimize_transducer (:20-24)
  Handle cur;
  const wfst_fst* x = f;
  if (!(x->props & NO_EPSILONS)) {
    cur.reset(rm_epsilon_fst(ctx, x));
    x = cur.get();
  }
  {
    Handle summed(tr_sum_fst(ctx, x, false));
    cur = std::move(summed);
    x = cur.get();
  }
  if (x->props & I_DETERMINISTIC) return minimize_fst(ctx, x, KSHORTESTDELTA, false);
  if (!(x->props & ACYCLIC))
    throw Error("optimize: inputs whose property word does not hold ACYCLIC are not supported");
  if (!acceptor) return encode_deter_mini_decode(ctx, x);
  Handle det(determinize_fst(ctx, x, KDELTA, /*Functional*/ 0u));
  cur.reset();
  return minimize_fst(ctx, det.get(), KSHORTESTDELTA, false);
}

namespace {

// "item <k>: <rest>", the form in which the batch stages report an item: k and where <rest> begins.  false: the error
// belongs to no item ("split the list", "did not converge", a HIP error)
bool item_error(const char* what, size_t* k, const char** rest) {
  if (std::strncmp(what, "item ", 5) != 0) return false;
  char* end = nullptr;
  const unsigned long long v = std::strtoull(what + 5, &end, 10);
  if (end == what + 5 || end[0] != ':' || end[1] != ' ') return false;
  *k = (size_t)v;
  *rest = end + 2;
  return true;
}

}  // namespace

// optimize of n FSTs: the branches of optimize_fst, each stage as ONE batch call over the sublist that takes it (DESIGN.md
// §3.10).  cur[i] is item i's intermediate handle (none yet: the input itself); every one is destroyed on every exit.
void optimize_batch(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, wfst_fst** outs, uint8_t* in_kernel) {
  using namespace props;
  ctx->opt_batch = {};
  check_items_owned(ctx, fsts, n, "optimize_batch");
  OptimizeBatchStats& stats = ctx->opt_batch;
  std::vector<Handle> cur(n);
  std::vector<uint8_t> flag(n, 1);
  auto at = [&](size_t i) -> const wfst_fst* { return cur[i] ? cur[i].get() : fsts[i]; };
  // An item error at index i.  The stages run on sublists, so an item below i may fail in a LATER stage, and the loop of
  // single calls would report that one: the intermediates go, optimize_fst replays items 0..i in index order and the first
  // error met is thrown with its index in front.  A cold path.
  auto replay = [&](size_t i, const std::string& message) {
    for (Handle& h : cur) h.reset();
    for (size_t j = 0; j <= i; ++j) {
      try {
        Handle again(optimize_fst(ctx, fsts[j]));
      } catch (const std::exception& e) {
        throw Error("item " + std::to_string(j) + ": " + e.what());
      }
    }
    throw Error("item " + std::to_string(i) + ": " + message);  // (the replay found nothing: the stage's own message)
  };
  // one stage over the sublist `sub`: its results replace the items' intermediates, its flags join theirs
  auto stage = [&](const std::vector<size_t>& sub, int which, const BatchStats& inner, auto&& call) {
    if (sub.empty()) return;
    const size_t m = sub.size();
    std::vector<const wfst_fst*> in(m);
    std::vector<wfst_fst*> got(m, nullptr);
    std::vector<uint8_t> fl(m, 0);
    for (size_t k = 0; k < m; ++k) in[k] = at(sub[k]);
    try {
      call(in.data(), m, got.data(), fl.data());
    } catch (const std::exception& e) {
      stats.launches[which] = inner.launches;
      size_t k = 0;
      const char* rest = nullptr;
      if (!item_error(e.what(), &k, &rest) || k >= m) throw;
      replay(sub[k], rest);
    }
    stats.launches[which] = inner.launches;
    for (size_t k = 0; k < m; ++k) {
      cur[sub[k]].reset(got[k]);
      flag[sub[k]] &= fl[k];
    }
  };
  std::vector<size_t> sub;
  // 1. rm_epsilon unless the word holds NO_EPSILONS
  for (size_t i = 0; i < n; ++i)
    if (!(fsts[i]->props & NO_EPSILONS)) sub.push_back(i);
  stage(sub, 0, ctx->rm_batch, [&](const wfst_fst* const* in, size_t m, wfst_fst** got, uint8_t* fl) { rm_epsilon_batch(ctx, in, m, got, fl); });
  // 2. tr_sum of every item
  sub.resize(n);
  for (size_t i = 0; i < n; ++i) sub[i] = i;
  stage(sub, 1, ctx->trsum_batch, [&](const wfst_fst* const* in, size_t m, wfst_fst** got, uint8_t* fl) { tr_sum_batch(ctx, in, m, false, got, fl); });
  // 3. on the word after tr_sum (optimize_fst's branch table)
  std::vector<size_t> det, mini, trans;
  for (size_t i = 0; i < n; ++i) {
    const uint64_t p = cur[i]->props;
    if (p & I_DETERMINISTIC) {
      mini.push_back(i);
    } else if (!(p & ACYCLIC)) {
      replay(i, "optimize: inputs whose property word does not hold ACYCLIC are not supported");
    } else if (fsts[i]->props & ACCEPTOR) {
      det.push_back(i);
      mini.push_back(i);
    } else {
      trans.push_back(i);
    }
  }
  stage(det, 2, ctx->det_batch, [&](const wfst_fst* const* in, size_t m, wfst_fst** got, uint8_t* fl) {
    determinize_batch(ctx, in, m, KDELTA, /*Functional*/ 0u, got, fl);
  });
  // 4. minimize
  stage(mini, 3, ctx->min_batch, [&](const wfst_fst* const* in, size_t m, wfst_fst** got, uint8_t* fl) {
    minimize_batch(ctx, in, m, KSHORTESTDELTA, false, got, fl);
  });
  // transducers: no batch form of the label encoding; each on its own
  for (size_t i : trans) {
    try {
      cur[i].reset(encode_deter_mini_decode(ctx, cur[i].get()));
    } catch (const std::exception& e) {
      const std::string message = e.what();
      replay(i, message);
    }
    flag[i] = 0;
    stats.items_transducer += 1;
  }
  for (size_t i = 0; i < n; ++i) {
    (flag[i] ? stats.items_in_kernel : stats.items_single) += 1;
    outs[i] = cur[i].release();
  }
  if (in_kernel) std::copy(flag.begin(), flag.end(), in_kernel);
}

}  // namespace wfst
