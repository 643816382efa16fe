// sigma_ranges.h — what a sigma matcher's side needs on the device, shared by compose_sigma.hip (the wide driver's
// SigmaPolicy) and compose_sigma_batch.hip (the wave-per-utterance kernel): has_sigma of every state of a sigma operand
// (sigma_matcher.rs:33-45: matcher.iter(state, sigma).next().is_some()) as the range the sorted matcher would walk, the
// allowed set in searchable form, and the rewrite decision.  Like compose_wide.h, everything here sits in an anonymous
// namespace: each translation unit that includes it gets its own copy of the kernel.
#pragma once
#include <algorithm>

#include "compose_match.h"
#include "fst_props.h"

namespace wfst {
namespace {

// sig[s] = {first sigma arc within the state's arcs, how many}: one thread per state
__global__ void __launch_bounds__(256) sigma_ranges(const wfst_tr* __restrict__ arcs, const uint4* __restrict__ srec, uint32_t n_states,
                                                    bool by_ilabel, uint32_t sigma, uint2* __restrict__ sig) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_states) return;
  const uint4 r = srec[s];
  uint32_t lo = 0, cnt = 0;
  equal_range(arcs + r.x, r.y, by_ilabel, sigma, &lo, &cnt);
  sig[s] = make_uint2(lo, cnt);
}

// One side's tables.  Without a config, or with sigma_label == NO_LABEL (has_sigma is false everywhere then,
// sigma_matcher.rs:40-44), everything stays empty and sigma stays NO_LABEL.
struct SigmaTables {
  DBuf<uint2> sig;              // [n_states]
  DBuf<uint32_t> allowed;       // ascending and distinct
  std::vector<uint32_t> h_allowed;  // (the upload's source)
  uint32_t n_allowed = 0;       // 0: no restriction
  uint32_t sigma = WFST_NO_LABEL;
  uint32_t rewrite_both = 0;    // sigma_matcher.rs:67-75
};
// Queues the pre-pass and the allowed set's upload on ctx's stream; `b` must outlive the stream's next synchronisation.
inline void sigma_tables(wfst_ctx* ctx, const wfst_fst* f, const SigmaSpec* m, bool by_ilabel, SigmaTables& b) {
  if (!m || m->sigma_label == WFST_NO_LABEL) return;
  hipStream_t st = ctx->stream;
  b.sigma = m->sigma_label;
  b.rewrite_both = m->rewrite_mode == 1u || (m->rewrite_mode == 0u && (f->props & props::ACCEPTOR)) ? 1u : 0u;
  b.sig = DBuf<uint2>(*ctx->pool, std::max<uint32_t>(f->n_states, 1));
  if (f->n_states)
    sigma_ranges<<<(f->n_states + 255) / 256, 256, 0, st>>>(f->dev.arcs, f->dev.srec, f->n_states, by_ilabel, b.sigma, b.sig.p);
  HIP_CHECK(hipGetLastError());
  if (m->n_allowed) {  // a HashSet in the reference (compose_static.rs:101-103): order and duplicates do not matter
    b.h_allowed.assign(m->allowed, m->allowed + m->n_allowed);
    std::sort(b.h_allowed.begin(), b.h_allowed.end());
    b.h_allowed.erase(std::unique(b.h_allowed.begin(), b.h_allowed.end()), b.h_allowed.end());
    b.allowed = DBuf<uint32_t>(*ctx->pool, b.h_allowed.size());
    HIP_CHECK(hipMemcpyAsync(b.allowed.p, b.h_allowed.data(), b.h_allowed.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    b.n_allowed = (uint32_t)b.h_allowed.size();
  }
}

}  // namespace
}  // namespace wfst
