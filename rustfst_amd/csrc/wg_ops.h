// wg_ops.h — passes of ONE workgroup of MB_TPB threads over arrays in global memory, separated by barriers: fill, exclusive
// scan, transpose of a CSR, frontier search.  What the one-workgroup-per-item batch kernels (minimize_batch_kernel in
// minimize.hip, rm_epsilon_batch_kernel in rm_epsilon_batch.hip) are made of; their host side is batch_driver.h.
#pragma once
#include "common.h"

namespace wfst {
namespace {

constexpr uint32_t MB_TPB = 256;            // 4 waves: small lattices leave no more lanes busy, and 8 workgroups fit a compute unit
// words that other lanes of the SAME launch wrote (narrow regime: level after level in one workgroup): device-scope
// accesses, which do not stay in a compute unit's vector L1
__device__ inline uint32_t ld(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void stg(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// transpose of a CSR: thread `tid` of `nth`, 16 lanes per state; cursor zeroed by the caller
__device__ void transpose_fill(const uint32_t* __restrict__ off, const wfst_tr* __restrict__ arcs, uint32_t n,
                               const uint32_t* __restrict__ roff, uint32_t* __restrict__ cursor, uint32_t* __restrict__ rsrc,
                               uint32_t tid, uint32_t nth) {
  const uint32_t lane = tid & 15u;
  for (uint32_t s = tid >> 4; s < n; s += nth >> 4)
    for (uint32_t i = off[s] + lane; i < off[s + 1]; i += 16) {
      const uint32_t t = arcs[i].nextstate;
      rsrc[roff[t] + atomicAdd(&cursor[t], 1u)] = s;
    }
}
// every thread of the workgroup: what was written before is visible after
__device__ inline void wg_bar() {
  __threadfence();
  __syncthreads();
}
__device__ inline void wg_fill(uint32_t* p, uint32_t count, uint32_t v) {
  for (uint32_t i = threadIdx.x; i < count; i += MB_TPB) p[i] = v;
}
__device__ inline void wg_fill64(unsigned long long* p, uint32_t count, unsigned long long v) {
  for (uint32_t i = threadIdx.x; i < count; i += MB_TPB) p[i] = v;
}
// out[i] = in[0] + .. + in[i - 1] for i < count (in == out allowed); returns the sum of all.  part: MB_TPB + 1 words of LDS
__device__ uint32_t wg_exclusive_scan(const uint32_t* in, uint32_t* out, uint32_t count, uint32_t* part) {
  const uint32_t tid = threadIdx.x;
  const uint32_t chunk = (count + MB_TPB - 1) / MB_TPB;
  const uint32_t b = min(count, tid * chunk), e = min(count, b + chunk);
  uint32_t sum = 0;
  for (uint32_t i = b; i < e; ++i) sum += ld(&in[i]);
  part[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    uint32_t run = 0;
    for (uint32_t t = 0; t < MB_TPB; ++t) {
      const uint32_t v = part[t];
      part[t] = run;
      run += v;
    }
    part[MB_TPB] = run;
  }
  __syncthreads();
  uint32_t run = part[tid];
  for (uint32_t i = b; i < e; ++i) {
    const uint32_t v = ld(&in[i]);
    stg(&out[i], run);
    run += v;
  }
  const uint32_t total = part[MB_TPB];
  wg_bar();
  return total;
}
// transpose of (off, arcs) with n states into (roff, rsrc); rcnt: n + 1 words of scratch
__device__ void wg_transpose(const uint32_t* off, const wfst_tr* arcs, uint32_t n, uint32_t E, uint32_t* roff, uint32_t* rcnt,
                             uint32_t* rsrc, uint32_t* part) {
  wg_fill(rcnt, n + 1, 0u);
  wg_bar();
  for (uint32_t i = threadIdx.x; i < E; i += MB_TPB) atomicAdd(&rcnt[arcs[i].nextstate], 1u);
  wg_bar();
  wg_exclusive_scan(rcnt, roff, n + 1, part);
  wg_fill(rcnt, n + 1, 0u);
  wg_bar();
  transpose_fill(off, arcs, n, roff, rcnt, rsrc, threadIdx.x, MB_TPB);
  wg_bar();
}
// frontier search: queue[0 .. q[2]) holds the marked seeds; every state reached over the adjacency (off, arcs' nextstate)
// or, with arcs == nullptr, (off, src) is marked and queued once.  q: three words of LDS (level begin, level end, tail).
__device__ void wg_search(const uint32_t* off, const wfst_tr* arcs, const uint32_t* src, uint32_t* mark, uint32_t* queue,
                          uint32_t* q) {
  const uint32_t tid = threadIdx.x, lane = tid & 15u;
  if (tid == 0) {
    q[0] = 0;
    q[1] = q[2];
  }
  __syncthreads();
  for (;;) {
    const uint32_t lo = q[0], hi = q[1];
    if (lo == hi) break;
    for (uint32_t k = lo + (tid >> 4); k < hi; k += MB_TPB >> 4) {
      const uint32_t s = ld(&queue[k]);
      for (uint32_t i = off[s] + lane; i < off[s + 1]; i += 16) {
        const uint32_t t = arcs ? arcs[i].nextstate : src[i];
        if (ld(&mark[t]) == 0u && atomicExch(&mark[t], 1u) == 0u) stg(&queue[atomicAdd(&q[2], 1u)], t);
      }
    }
    wg_bar();
    if (tid == 0) {
      q[0] = hi;
      q[1] = q[2];
    }
    __syncthreads();
  }
}

}  // namespace
}  // namespace wfst
