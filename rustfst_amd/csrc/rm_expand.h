// rm_expand.h — RmEpsilonState::expand (algorithms/rm_epsilon/rm_epsilon_state.rs:44-119) of ONE state by ONE thread: the
// closure distances, the depth-first walk, the combining of equal (ilabel, olabel, nextstate) at the first occurrence and
// the final reversal.  They define the arc order of rm_epsilon's result, so they exist once: rm_expand (rm_epsilon.hip,
// one launch per epsilon depth) and rm_epsilon_batch_kernel (rm_epsilon_batch.hip, one workgroup per FST) both call this.
#pragma once
#include "common.h"

namespace wfst {

struct RmCaps {
  uint32_t C;  // closure states
  uint32_t K;  // depth-first stack entries
  uint32_t A;  // arcs of the rewritten state
};
__host__ __device__ inline size_t rm_arcs_offset(const RmCaps& c) { return ((size_t)c.C * 12 + (size_t)c.K * 4 + 15) & ~(size_t)15; }
__host__ __device__ inline size_t rm_slice_bytes(const RmCaps& c) { return rm_arcs_offset(c) + (size_t)c.A * 16; }

__device__ __forceinline__ bool is_eps(const wfst_tr& t) { return t.ilabel == 0u && t.olabel == 0u; }  // EpsilonTrFilter

struct RmView {  // the FST as the reference's loop sees it at this moment
  const uint32_t* offsets;
  const wfst_tr* arcs;
  const uint32_t* done;                 // state already rewritten
  const uint32_t* cnt;                  // its new arc count
  const unsigned long long* arc_ptr;    // and where its new arcs are
  __device__ const wfst_tr* trs(uint32_t q, uint32_t* n) const {
    if (done[q]) {
      *n = cnt[q];
      return (const wfst_tr*)arc_ptr[q];
    }
    *n = offsets[q + 1] - offsets[q];
    return arcs + offsets[q];
  }
};

// the rewrite of state s inside `slice` (rm_slice_bytes(caps) bytes, 16-byte aligned): false when the slice is too small;
// else the new arcs are the *n_arcs arcs at slice + rm_arcs_offset(caps) and *final_weight the new final weight.  Nothing
// but the slice is written.
__device__ inline bool rm_expand_state(const RmView& v, uint32_t s, const RmCaps& caps, char* __restrict__ slice,
                                       const float* __restrict__ fin, uint32_t* n_arcs, float* final_weight) {
  uint32_t* cl = (uint32_t*)slice;  // closure states, in discovery order
  float* dist = (float*)(slice + (size_t)caps.C * 4);
  uint32_t* vis = (uint32_t*)(slice + (size_t)caps.C * 8);
  uint32_t* stack = (uint32_t*)(slice + (size_t)caps.C * 12);
  wfst_tr* out = (wfst_tr*)(slice + rm_arcs_offset(caps));
  // 1. closure and distances over the epsilon arcs as they are now
  uint32_t nc = 1;
  cl[0] = s;
  dist[0] = 0.0f;
  for (uint32_t iter = 0;; ++iter) {
    bool changed = false;
    for (uint32_t k = 0; k < nc; ++k) {
      const float dk = dist[k];
      uint32_t nq;
      const wfst_tr* tq = v.trs(cl[k], &nq);
      for (uint32_t a = 0; a < nq; ++a) {
        const wfst_tr tr = tq[a];
        if (!is_eps(tr)) continue;
        uint32_t j = 0;
        while (j < nc && cl[j] != tr.nextstate) ++j;
        if (j == nc) {
          if (nc == caps.C) return false;
          cl[nc] = tr.nextstate;
          dist[nc] = INF;
          ++nc;
          changed = true;
        }
        const float cand = wtimes(dk, tr.weight);
        if (cand < dist[j]) {
          dist[j] = cand;
          changed = true;
        }
      }
    }
    if (!changed) break;
    if (iter > nc + 1u) break;  // a negative epsilon cycle: the reference would not terminate either; stop improving
  }
  // 2. the depth-first walk of the closure: arcs and the final weight in visiting order
  for (uint32_t k = 0; k < nc; ++k) vis[k] = 0u;
  uint32_t sp = 0, na = 0;
  stack[sp++] = 0u;  // (indices into cl)
  float final_w = INF;
  while (sp) {
    const uint32_t k = stack[--sp];
    if (vis[k]) continue;
    vis[k] = 1u;
    const uint32_t q = cl[k];
    const float dq = dist[k];
    uint32_t nq;
    const wfst_tr* tq = v.trs(q, &nq);
    for (uint32_t a = 0; a < nq; ++a) {
      wfst_tr tr = tq[a];
      tr.weight = wtimes(dq, tr.weight);
      if (is_eps(tr)) {
        uint32_t j = 0;
        while (cl[j] != tr.nextstate) ++j;  // (in the closure since step 1)
        if (!vis[j]) {
          if (sp == caps.K) return false;
          stack[sp++] = j;
        }
      } else {
        uint32_t j = 0;
        while (j < na && !(out[j].ilabel == tr.ilabel && out[j].olabel == tr.olabel && out[j].nextstate == tr.nextstate)) ++j;
        if (j < na) {
          if (tr.weight < out[j].weight) out[j].weight = tr.weight;  // plus_assign at the first occurrence
        } else {
          if (na == caps.A) return false;
          out[na++] = tr;
        }
      }
    }
    const float f = wtimes(dq, fin[q]);
    final_w = f < final_w ? f : final_w;
  }
  for (uint32_t a = 0; a < na / 2; ++a) {  // trs.into_iter().rev() (rm_epsilon_static.rs:125)
    const wfst_tr t = out[a];
    out[a] = out[na - 1 - a];
    out[na - 1 - a] = t;
  }
  *n_arcs = na;
  *final_weight = final_w;
  return true;
}

}  // namespace wfst
