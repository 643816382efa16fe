// device_ops.hip — host-side plumbing shared by the device operations (declared in common.h): the rocPRIM exclusive
// scan, one-word read-back, in-degree counting, hash-table sizing.  Everything runs on ctx->stream.
#include <algorithm>

#include <rocprim/device/device_scan.hpp>

#include "common.h"

namespace wfst {

namespace {

__global__ void indegree_kernel(const wfst_tr* __restrict__ arcs, uint64_t n_arcs, uint32_t* __restrict__ indeg) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_arcs; i += (uint64_t)gridDim.x * blockDim.x)
    atomicAdd(&indeg[arcs[i].nextstate], 1u);
}

}  // namespace

DBuf<uint8_t> exclusive_scan_u32(wfst_ctx* ctx, const uint32_t* in, uint32_t* out, size_t count) {
  size_t temp_bytes = 0;
  HIP_CHECK(rocprim::exclusive_scan(nullptr, temp_bytes, in, out, 0u, count, rocprim::plus<uint32_t>(), ctx->stream));
  DBuf<uint8_t> temp(*ctx->pool, temp_bytes);
  HIP_CHECK(rocprim::exclusive_scan(temp.p, temp_bytes, in, out, 0u, count, rocprim::plus<uint32_t>(), ctx->stream));
  return temp;
}

uint32_t read_u32(wfst_ctx* ctx, const uint32_t* d) {
  uint32_t v = 0;
  HIP_CHECK(hipMemcpyAsync(&v, d, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return v;
}

void count_indegrees(wfst_ctx* ctx, const wfst_tr* arcs, uint64_t n_arcs, uint32_t* indeg) {
  if (!n_arcs) return;
  const uint32_t blocks = (uint32_t)std::min<uint64_t>((n_arcs + 255) / 256, (uint64_t)ctx->n_cus * 8);
  indegree_kernel<<<blocks, 256, 0, ctx->stream>>>(arcs, n_arcs, indeg);
  HIP_CHECK(hipGetLastError());
}

uint32_t pow2_at_least(uint64_t v, const char* what) {
  uint64_t p = 64;
  while (p < v) p <<= 1;
  if (p > (1ull << 31)) throw Error(std::string(what) + ": input too large (a hash table beyond 2^31 entries)");
  return (uint32_t)p;
}

}  // namespace wfst
