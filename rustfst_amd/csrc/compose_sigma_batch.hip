// compose_sigma_batch.hip — the fused batch with a sigma matcher on T: for every acceptor a_i of a batch,
// shortest_path(compose_with_config(a_i, T, config with matcher configs)), bit for bit what the caller's loop over
// wfst_compose_with_matchers + wfst_shortest_path returns, property word included.
//
// The decoding case runs in ONE launch of string_sigma_sp_kernel, one wavefront per utterance: a_i a linear, epsilon-free
// acceptor (wfst_fst::is_string), T known ilabel-sorted and without input epsilons, a SigmaMatcher on T alone, the Sequence
// filter.  The kernel has the shape of compose.hip's string_compose_sp_kernel — BFS level `pos` = the composed states (pos, q),
// the frontier in lane registers, parents / olabels / weights in the wave's slice of LDS, no hash table — as a plain level
// loop: no chase runs, no scalar rows, no tickets, no zero-copy results.  What the sigma matcher adds per level, with the
// string's label l (wave-uniform) and lane k holding (pos, q_k); the reference's lines are those of compose_sigma.hip's head:
//   bad label      l == sigma is Err "SigmaMatcher::Find: bad label (sigma)" (sigma_matcher.rs:199-201) as soon as a composed
//                  state is expanded whose item carries it.  The string's arc is an item wherever the string is iterated:
//                  in BOTH mode that is every state whose q_k has arcs (match_input, compose_fst_op.rs:199-219: q_k requires, or
//                  1 <= n2; a q_k without arcs is iterated itself and the string is searched by a plain SortedMatcher), in INPUT
//                  mode (the string's word does not say olabel-sorted) every state.  A position that no state reaches never raises.
//   exact first    the run of q_k's arcs with ilabel l, in arc order (blocks of more than 64 arcs: chunk by chunk).  Where it is
//                  not empty it is the whole answer: no fall-through to the sigma arcs (:206-208, DESIGN.md 3.15 rule 4).
//   sigma          only where the run is empty: q_k's sigma range (sigma_ranges.h, one launch per call), if the allowed set is
//                  empty or holds l (searched by the whole wave, once per level, only when a state needs it).  Each sigma arc's
//                  olabel becomes l iff rewrite_both and it equals sigma (value_openfst, :246-266; the ilabel of the composed
//                  arc is the string's).
//   numbering      emission order = frontier order, then T's arc order; a destination new to the level gets the next id
//                  (StateTable::find_id); its parent is the first strict improvement in emission order — the canonical parent
//                  of string_compose_sp_kernel, which is what shortest_path returns on the layered lattice.
// A level of more than 64 states, more composed states than the slice holds, or a label 0xFFFFFFFF in the string end the item
// as "not a string case": the host redoes it on the loop route.  Everything else — a matcher on side 1, another filter, T with
// input epsilons or not known sorted, a non-linear acceptor, wfst_ctx_set_tie_order — never reaches the kernel: those
// items go one by one through compose_sigma + shortest_path_n1 on the same context, in item order.
#include "sigma_ranges.h"
#include "string_placement.h"

namespace wfst {
namespace {

constexpr uint32_t SSB_MAXS = 2048;  // states of an acceptor, and composed states of an item, at most (compose.hip: STR_MAXS)
constexpr uint32_t SSB_NONE = 0xFFFFFFFFu;
static_assert(SSB_MAXS * 16u * 2u <= STRING_LDS_BYTES, "string_placement.h: two of the largest slices per workgroup");
constexpr unsigned long long SSB_KEY_INF = ~0ull;
enum : uint32_t { SSB_OK = 0, SSB_NOT_A_STRING_CASE = 1, SSB_BAD_LABEL = 2 };

struct SsbDesc {
  const wfst_tr* arcs;  // the string's arcs: arc i leaves state i
  const uint4* srec;    // its state records (the final weight of state L)
  uint32_t L;           // number of arcs
  uint32_t path_off;    // this item's slice of the path buffer: L arcs
  uint32_t iterate_always;  // INPUT mode: the string is iterated in every composed state
  uint32_t pad;
};
struct SsbGrammar {
  const wfst_tr* arcs;
  const uint4* srec;        // {arc begin, arc count, final bits, epsilon facts}
  const uint2* anext;       // per arc: {arc begin, arc count} of its destination (wfst_fst::anext)
  const uint2* sig;         // per state: {first sigma arc within its block, how many}; null: sigma == NO_LABEL
  const uint32_t* allowed;  // ascending and distinct
  uint32_t n_allowed;       // 0: no restriction
  uint32_t sigma, rewrite_both, start;
};
struct SsbResult {
  uint32_t status;
  uint32_t n_states, n_arcs;  // of the composition, before trimming
  uint32_t has_path;          // hops == L
  float final_weight;
  uint32_t facts;  // OR of props::path_arc_facts over the path
  uint32_t exact_items, sigma_items, sigma_arcs, refused_items, max_level_width;
  uint32_t pad;
};

// is_match_label_allowed (sigma_matcher.rs:172-181) by the whole wave: each round the lanes probe 64 evenly spaced entries
// of [lo, hi) and the range shrinks to the stride that holds `label`; the last round compares 64 neighbours
__device__ bool ssb_allowed(const uint32_t* __restrict__ allowed, uint32_t n, uint32_t label, uint32_t lane) {
  uint32_t lo = 0, hi = n;
  for (;;) {
    const uint32_t step = (hi - lo + 63u) / 64u;
    const uint32_t idx = lo + lane * step;
    const bool in = idx < hi;
    const uint32_t v = in ? allowed[idx] : 0u;
    if (step <= 1u) return __ballot(in && v == label) != 0ull;
    const uint64_t le = __ballot(in && v <= label);  // (a prefix of the lanes: the set ascends)
    if (le == 0ull) return false;
    lo += ((uint32_t)__popcll(le) - 1u) * step;
    hi = min(lo + step, hi);
  }
}

// One wave = one item; a workgroup holds blockDim.x / 64 of them, each with its own `maxs`-state slice of the dynamic LDS.
__global__ void __launch_bounds__(512) string_sigma_sp_kernel(const SsbDesc* __restrict__ descs, SsbGrammar g,
                                                              SsbResult* __restrict__ results, wfst_tr* __restrict__ path_buf,
                                                              uint32_t n_problems, uint32_t maxs) {
  extern __shared__ __attribute__((aligned(16))) uint32_t s_dyn[];
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t p = blockIdx.x * (blockDim.x >> 6) + wave;
  if (p >= n_problems) return;
  uint32_t* const s_par = s_dyn + (size_t)wave * 4u * maxs;  // predecessor on the best way into the state (SSB_NONE: unreached)
  uint32_t* const s_ol = s_par + maxs;                        // olabel of the arc taken from it
  float* const s_w = reinterpret_cast<float*>(s_ol + maxs);   // its weight (w1 (x) w2)
  uint32_t* const s_pth = s_ol + 2u * maxs;                   // states of the best path, from the final one backwards
  const uint32_t lane = threadIdx.x & 63u;
  const SsbDesc D = descs[p];
  const uint32_t L = D.L;
  SsbResult res;
  res.status = SSB_OK;
  res.n_states = res.n_arcs = res.has_path = 0;
  res.final_weight = INF;
  res.facts = 0;
  res.exact_items = res.sigma_items = res.sigma_arcs = res.refused_items = 0;
  res.max_level_width = 1;
  res.pad = 0;
  // the frontier: lane k < F holds composed state lo + k = (pos, q) with q's arc block [nb, nb + nc) and distance d
  uint32_t q = 0, nb = 0, nc = 0;
  float d = INF;
  if (lane == 0) {
    q = g.start;
    d = 0.0f;  // Weight::one()
    const uint4 r = g.srec[q];
    nb = r.x;
    nc = r.y;
    s_par[0] = SSB_NONE;
  }
  uint32_t lo = 0, hi = 1, F = 1, n_arcs = 0, level = 0;
  uint4 ch = make_uint4(0, 0, 0, 0);  // 64 arcs of the string, one per lane
  const bool sigma_real = g.sigma != NO_LABEL;
  for (uint32_t pos = 0; pos < L && F; ++pos) {
    if ((pos & 63u) == 0u) {
      ch = make_uint4(0, 0, 0, 0);
      if (pos + lane < L) ch = *reinterpret_cast<const uint4*>(D.arcs + pos + lane);
    }
    const uint32_t label = rl(ch.x, pos & 63u);
    const float w1 = __uint_as_float(rl(ch.z, pos & 63u));
    if (label == NO_LABEL) {  // (the sorted matcher looks for epsilons then: not this kernel's case)
      res.status = SSB_NOT_A_STRING_CASE;
      break;
    }
    uint2 sg = make_uint2(0, 0);
    if (g.sig && lane < F) sg = g.sig[q];
    if (sigma_real && label == g.sigma && (D.iterate_always || __ballot(lane < F && nc != 0u) != 0ull)) {
      res.status = SSB_BAD_LABEL;
      break;
    }
    int allowed_l = g.n_allowed == 0u ? 1 : -1;  // (-1: not asked yet)
    uint32_t nq = 0, nnb = 0, nnc = 0, n_new = 0;  // the next level: lane k holds state hi + k
    float nd = INF;
    bool ok = true;
    // one emitted arc (f -> qd, output label ol, weight w2, the destination's arc block [xb, xb + xc))
    auto on_match = [&](uint32_t f, float fd, uint32_t qd, uint32_t ol, uint32_t xb, uint32_t xc, float w2) -> bool {
      const float wsum = wtimes(w1, w2);  // add_tr, compose_fst_op.rs:267-285
      float c = INF;
      if (fd < INF) c = (fd + wsum) + 0.0f;  // +inf never relaxes (shortest_path.rs:226)
      const uint64_t ex = __ballot(lane < n_new && nq == qd);  // StateTable::find_id inside the level
      uint32_t idx;
      if (ex == 0ull) {
        idx = n_new;
        if (idx >= 64u || hi + idx >= maxs) return false;
        if (lane == idx) {
          nq = qd;
          nnb = xb;
          nnc = xc;
          nd = INF;
        }
        if (lane == 0) s_par[hi + idx] = SSB_NONE;
        n_new += 1;
      } else {
        idx = (uint32_t)__ffsll((unsigned long long)ex) - 1u;
      }
      const float cur = rlf(nd, idx);
      if (c < cur) {  // strict: on ties the earlier (source id, arc position) stays
        if (lane == idx) nd = c;
        if (lane == 0) {
          s_par[hi + idx] = lo + f;
          s_ol[hi + idx] = ol;
          s_w[hi + idx] = wsum;
        }
      }
      return true;
    };
    // the arcs of `m`'s lanes, in lane order; by_sigma: rewritten (value_openfst)
    auto emit = [&](uint64_t m, uint32_t f, float fd, const uint4& a, const uint2& nx, bool by_sigma) -> bool {
      n_arcs += (uint32_t)__popcll(m);
      while (m) {
        const uint32_t l = (uint32_t)__ffsll((unsigned long long)m) - 1u;
        m &= m - 1ull;
        uint32_t ol = rl(a.y, l);
        if (by_sigma && g.rewrite_both && ol == g.sigma) ol = label;
        if (!on_match(f, fd, rl(a.w, l), ol, rl(nx.x, l), rl(nx.y, l), __uint_as_float(rl(a.z, l)))) return false;
      }
      return true;
    };
    for (uint32_t f = 0; f < F && ok; ++f) {
      const uint32_t fb = rl(nb, f), fc = rl(nc, f), fsl = rl(sg.x, f), fsn = rl(sg.y, f);
      const float fd = rlf(d, f);
      if (fc == 0u) continue;  // (T's state is the iterated side: it has nothing to iterate)
      uint32_t found = 0;
      uint4 a = make_uint4(0, 0, 0, 0);
      uint2 nx = make_uint2(0, 0);
      for (uint32_t base = 0; base < fc && ok; base += 64u) {
        const bool have = base + lane < fc;
        if (have) {
          a = *reinterpret_cast<const uint4*>(g.arcs + fb + base + lane);
          nx = g.anext[fb + base + lane];
        }
        const uint64_t m = __ballot(have && a.x == label);  // the label-equal run of the sorted block, in arc order
        found += (uint32_t)__popcll(m);
        ok = emit(m, f, fd, a, nx, false);
      }
      if (!ok) break;
      if (found) {
        res.exact_items += sigma_real ? 1u : 0u;
        continue;
      }
      if (fsn == 0u) continue;
      if (allowed_l < 0) allowed_l = ssb_allowed(g.allowed, g.n_allowed, label, lane) ? 1 : 0;
      if (!allowed_l) {
        res.refused_items += 1u;
        continue;
      }
      res.sigma_items += 1u;
      res.sigma_arcs += fsn;
      if (fc <= 64u) {  // the lanes still hold the whole block: its sigma arcs are lanes [fsl, fsl + fsn)
        ok = emit(__ballot(lane >= fsl && lane < fsl + fsn), f, fd, a, nx, true);
      } else {
        for (uint32_t base = 0; base < fsn && ok; base += 64u) {
          const bool have = base + lane < fsn;
          if (have) {
            a = *reinterpret_cast<const uint4*>(g.arcs + fb + fsl + base + lane);
            nx = g.anext[fb + fsl + base + lane];
          }
          ok = emit(__ballot(have), f, fd, a, nx, true);
        }
      }
    }
    if (!ok) {
      res.status = SSB_NOT_A_STRING_CASE;
      break;
    }
    lo = hi;
    hi += n_new;
    F = n_new;
    q = nq;
    nb = nnb;
    nc = nnc;
    d = nd;
    if (F) level = pos + 1u;
    res.max_level_width = max(res.max_level_width, n_new);
  }
  if (res.status != SSB_OK) {
    if (lane == 0) results[p] = res;
    return;
  }
  res.n_states = hi;
  res.n_arcs = n_arcs;
  // final states: only level L can be final (the string's single final state); rho = rho1 (x) rho2 (compose_fst_op.rs:420-449)
  unsigned long long best = SSB_KEY_INF;
  float my_fin = INF;
  if (F && level == L) {
    const float fin1 = __uint_as_float(D.srec[L].z);
    if (lane < F) {
      const float fin2 = __uint_as_float(g.srec[q].z);
      if (fin1 != INF && fin2 != INF) my_fin = wtimes(fin1, fin2);
      if (d < INF && my_fin < INF) {
        const float tot = (d + my_fin) + 0.0f;
        if (tot < INF) best = ((unsigned long long)f32_key(tot) << 32) | (lo + lane);
      }
    }
  }
  best = wave_min_u64(best);  // the smallest (total, state id)
  if (best != SSB_KEY_INF) {
    const uint32_t fp = (uint32_t)best;
    res.has_path = 1;
    res.final_weight = rlf(my_fin, fp - lo);
    lds_handoff();
    if (lane == 0) {  // the parents back to state 0: exactly L arcs (every arc climbs one level)
      uint32_t st = fp;
      for (uint32_t k = 0; k < L; ++k) {
        s_pth[k] = st;
        st = s_par[st];
      }
    }
    lds_handoff();
    uint32_t facts = 0;
    for (uint32_t k = lane; k < L; k += 64u) {  // arc k enters the k-th state the backtrace creates (shortest_path.rs:257-272)
      const uint32_t st = s_pth[k];
      const uint32_t il = D.arcs[L - 1u - k].ilabel;
      const uint32_t ol = s_ol[st];
      const float w = s_w[st];
      *reinterpret_cast<uint4*>(path_buf + D.path_off + k) = make_uint4(il, ol, __float_as_uint(w), k);
      facts |= props::path_arc_facts(il, ol, w);
    }
    for (int o = 32; o >= 1; o >>= 1) facts |= (uint32_t)__shfl_xor((int)facts, o);
    res.facts = facts;
  }
  if (lane == 0) results[p] = res;
}

}  // namespace

void compose_sigma_sp_batch(wfst_ctx* ctx, const wfst_fst* const* accs, size_t n, const wfst_fst* t, bool connect, uint32_t filter,
                            const SigmaSpec* m1, const SigmaSpec* m2, wfst_fst** outs, uint64_t* composed_arcs) {
  using namespace props;
  ctx->sigma_batch = wfst_ctx::SigmaBatchCounters{};
  ctx->string_placement = {};
  wfst_ctx::SigmaBatchCounters& cnt = ctx->sigma_batch;
  if (composed_arcs) *composed_arcs = 0;
  if (n == 0) return;
  const EnvSnap env = EnvSnap::take();  // the WFST_* variables as the call found them
  // the set-up errors of every item, in item order, before anything is launched
  std::vector<uint32_t> mode(n);
  for (size_t i = 0; i < n; ++i) {
    if (!accs[i]) throw Error("null acceptor in batch");
    mode[i] = sigma_setup_mode(accs[i], t, filter, m1, m2);
  }
  // which items are the kernel's?
  bool kernel_ok = filter == 3u && !m1 && m2 && !ctx->tie_reference && t->start >= 0 && t->n_arcs > 0 && t->n_arcs < 0xFFFFFFFFull &&
                   (t->props & I_LABEL_SORTED);
  if (kernel_ok) {
    bool any = false;
    for (size_t i = 0; i < n && !any; ++i) any = accs[i]->is_string && accs[i]->n_states <= SSB_MAXS;
    kernel_ok = any;
  }
  const uint2* anext = nullptr;
  if (kernel_ok) {
    ensure_device(const_cast<wfst_fst*>(t));
    kernel_ok = !has_input_epsilons(ctx, t);
    if (kernel_ok) anext = ensure_anext(ctx, t);
    kernel_ok = anext != nullptr;
  }
  std::vector<size_t> items;       // the kernel's items, ascending
  std::vector<int64_t> slot(n, -1);  // item -> its position in `items`
  std::vector<SsbDesc> descs;
  uint64_t n_path = 0;
  uint32_t max_states = 0;
  if (kernel_ok)
    for (size_t i = 0; i < n; ++i) {
      const wfst_fst* a = accs[i];
      if (!a->is_string || a->n_states > SSB_MAXS || a->n_states == 0 || a->start != 0) continue;
      ensure_device(const_cast<wfst_fst*>(a));
      slot[i] = (int64_t)items.size();
      items.push_back(i);
      descs.push_back(SsbDesc{a->dev.arcs, a->dev.srec, a->n_states - 1u, (uint32_t)n_path, mode[i] == 1u ? 1u : 0u, 0u});
      n_path += a->n_states - 1u;
      max_states = std::max(max_states, a->n_states);
    }
  cnt.items_loop = n - items.size();
  const size_t k = items.size();
  hipStream_t st = ctx->stream;
  // staging: descriptors, results and path arcs of this call in one pinned block of its own (the loop route below uses the
  // context's staging buffers)
  const size_t off_res = (k * sizeof(SsbDesc) + 255) & ~(size_t)255, off_path = (off_res + k * sizeof(SsbResult) + 255) & ~(size_t)255;
  std::shared_ptr<PinnedBlock> block;
  DBuf<SsbDesc> d_desc;
  DBuf<SsbResult> d_res;
  DBuf<wfst_tr> d_path;
  SigmaTables tabs;
  const SsbResult* h_res = nullptr;
  const wfst_tr* h_path = nullptr;
  uint64_t tot_arcs = 0;
  for (size_t i = 0; i < n; ++i) outs[i] = nullptr;
  try {
    if (k) {
      block = ctx->pinned_ring->take(off_path + n_path * sizeof(wfst_tr) + 256);
      char* pin = (char*)block->p;
      std::memcpy(pin, descs.data(), k * sizeof(SsbDesc));
      d_desc = DBuf<SsbDesc>(*ctx->pool, k);
      d_res = DBuf<SsbResult>(*ctx->pool, k);
      d_path = DBuf<wfst_tr>(*ctx->pool, n_path);
      HIP_CHECK(hipMemcpyAsync(d_desc.p, pin, k * sizeof(SsbDesc), hipMemcpyHostToDevice, st));
      sigma_tables(ctx, t, m2, /*by_ilabel=*/true, tabs);  // sigma_ranges.h: one launch per call
      const SsbGrammar g{t->dev.arcs, t->dev.srec, anext, tabs.sig.p, tabs.allowed.p, tabs.n_allowed, tabs.sigma, tabs.rewrite_both,
                         (uint32_t)t->start};
      // states per slice: a string of L arcs against an input-deterministic-ish T composes to a little more than L states; an
      // item that outgrows its slice is handed back.  Waves per workgroup: string_placement.h
      // (WFST_STRING_UNPACKED, as in compose.hip: one wave per workgroup and the largest slice, whatever WFST_STRING_WPB says)
      const bool unpacked = env.has("WFST_STRING_UNPACKED");
      const uint64_t need = 2ull * max_states + 64;
      const uint32_t maxs = unpacked ? SSB_MAXS : (need <= 512 ? 512u : (need <= 1024 ? 1024u : SSB_MAXS));
      const StringPlacement pl = string_placement(k, maxs, (uint32_t)std::max(ctx->n_cus, 1), resident_grid_at_work(ctx->device),
                                                  unpacked ? 1u : string_forced_wpb(env.get("WFST_STRING_WPB")));
      ctx->string_placement = {pl.wpb, maxs, pl.workgroups, pl.packed_for_resident ? 1u : 0u, pl.forced ? 1u : 0u};
      string_sigma_sp_kernel<<<pl.workgroups, 64 * pl.wpb, (size_t)pl.wpb * 16u * maxs, st>>>(d_desc.p, g, d_res.p, d_path.p, (uint32_t)k, maxs);
      HIP_CHECK(hipGetLastError());
      cnt.launches += 1;
      HIP_CHECK(hipMemcpyAsync(pin + off_res, d_res.p, k * sizeof(SsbResult), hipMemcpyDeviceToHost, st));
      if (n_path) HIP_CHECK(hipMemcpyAsync(pin + off_path, d_path.p, n_path * sizeof(wfst_tr), hipMemcpyDeviceToHost, st));
      HIP_CHECK(hipStreamSynchronize(st));
      h_res = (const SsbResult*)(pin + off_res);
      h_path = (const wfst_tr*)(pin + off_path);
    }
    // the kernel's answers; the lowest item it ended in an error is where the caller's loop would have stopped
    size_t first_bad = n;
    for (size_t j = 0; j < k; ++j) {
      const SsbResult& r = h_res[j];
      if (r.status == SSB_BAD_LABEL) {
        first_bad = std::min(first_bad, items[j]);
      } else if (r.status == SSB_NOT_A_STRING_CASE) {
        cnt.items_handed_back += 1;
        slot[items[j]] = -1;
      } else {
        cnt.items_in_kernel += 1;
        cnt.exact_items += r.exact_items;
        cnt.sigma_items += r.sigma_items;
        cnt.sigma_arcs += r.sigma_arcs;
        cnt.refused_items += r.refused_items;
        cnt.max_level_width = std::max<uint64_t>(cnt.max_level_width, r.max_level_width);
        tot_arcs += r.n_arcs;
        const uint32_t hops = descs[j].L;
        outs[items[j]] = batch_path_fst(ctx, r.has_path != 0, hops, r.final_weight, r.has_path ? r.facts : PATH_FACTS_NONE,
                                        r.has_path && hops ? h_path + descs[j].path_off : nullptr);
      }
    }
    // the loop route, in item order up to the first error
    for (size_t i = 0; i < n; ++i) {
      if (i == first_bad) throw Error("SigmaMatcher::Find: bad label (sigma)");
      if (slot[i] >= 0) continue;
      Handle c(compose_sigma(ctx, accs[i], t, connect, filter, m1, m2));
      tot_arcs += ctx->compose_sigma.arcs;
      outs[i] = shortest_path_n1(ctx, c.get());
    }
  } catch (...) {
    (void)hipStreamSynchronize(st);  // (the kernel may still be writing this call's buffers)
    for (size_t i = 0; i < n; ++i) {
      delete outs[i];
      outs[i] = nullptr;
    }
    throw;
  }
  ctx->stats.compose_arcs = tot_arcs;
  if (composed_arcs) *composed_arcs = tot_arcs;
}

}  // namespace wfst
