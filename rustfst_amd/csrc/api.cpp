// api.cpp — the extern "C" surface declared in include/wfst.h (conventions: rustfst-ffi/src/lib.rs:29-97).
#include <cmath>
#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "lookahead.h"
#include "fst_props.h"

namespace wfst {

static thread_local std::string t_last_error;  // LAST_ERROR, rustfst-ffi/src/lib.rs:39-41
static thread_local bool t_has_error = false;
void set_last_error(const std::string& msg) {
  t_last_error = msg;
  t_has_error = true;
  if (std::getenv("WFST_FFI_ERROR_STDERR")) std::fprintf(stderr, "%s\n", msg.c_str());  // cf. lib.rs:48-50
}

// ---------------------------------------------------------------- DevicePool
size_t DevicePool::bucket(size_t bytes) {
  if (bytes < 256) return 256;
  // round up to a multiple of 1/8 of the enclosing power of two: <= 12.5 % slack, few distinct sizes
  size_t p = 256;
  while (p < bytes) p <<= 1;
  size_t step = p >> 3;
  return (bytes + step - 1) / step * step;
}
void* DevicePool::alloc(size_t bytes) {
  std::lock_guard<std::mutex> lk(mu_);
  size_t b = bucket(bytes);
  // LIFO inside a bucket: the block freed LAST is handed out first.  A solve frees its buffers in the reverse order of their
  // allocation, so every buffer of the next solve gets the block it had in the last one — two buffers of one bucket (the
  // mailbox kernels' two message arrays are both 160 MB for the benched T) otherwise SWAP blocks from solve to solve, and a
  // resident launch whose region headers sit where the other array was last time finds none of them in the Infinity Cache:
  // 280 -> 265 us per solve of C3 (LAB_NOTEBOOK.md, round 5).
  auto range = free_.equal_range(b);
  if (range.first != range.second) {
    auto it = std::prev(range.second);
    void* p = it->second;
    free_.erase(it);
    live_[p] = b;
    return p;
  }
  // A LARGE request (>= 64 MB) with no block of its own bucket takes the smallest cached block of up to twice its size instead
  // of a fresh hipMalloc (0.1-0.7 s for the multi-GB arenas of the wide compose driver: its second call asks for "last result
  // + 1/8" while the pool holds the first call's grown arena, a little larger — profiles/r06d_wide_lookahead.md).  Small
  // requests keep the exact-bucket rule above: their placement is what the relaxation's launches are tuned on.
  if (b >= (64u << 20)) {
    auto it = free_.upper_bound(b);
    if (it != free_.end() && it->first <= 2 * b) {
      void* p = it->second;
      const size_t real = it->first;
      free_.erase(it);
      live_[p] = real;
      return p;
    }
  }
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, b);
  if (e != hipSuccess) {
    trim_locked();
    HIP_CHECK(hipMalloc(&p, b));
  }
  live_[p] = b;
  return p;
}
void DevicePool::free(void* p) {
  if (!p) return;
  std::lock_guard<std::mutex> lk(mu_);
  auto it = live_.find(p);
  if (it == live_.end()) return;
  free_.emplace(it->second, p);
  live_.erase(it);
}
void DevicePool::park(void* const* ps, size_t count) {
  std::lock_guard<std::mutex> lk(mu_);
  for (size_t i = 0; i < count; ++i) {
    auto it = ps[i] ? live_.find(ps[i]) : live_.end();
    if (it == live_.end()) continue;
    parked_.emplace(it->first, it->second);
    live_.erase(it);
  }
}
bool DevicePool::unpark(void* const* ps, size_t count) {
  std::lock_guard<std::mutex> lk(mu_);
  for (size_t i = 0; i < count; ++i)
    if (ps[i] && parked_.find(ps[i]) == parked_.end()) return false;  // (trim takes all of them at once)
  for (size_t i = 0; i < count; ++i) {
    if (!ps[i]) continue;
    auto it = parked_.find(ps[i]);
    live_.emplace(it->first, it->second);
    parked_.erase(it);
  }
  return true;
}
void DevicePool::trim_locked() {
  for (auto& kv : free_) (void)hipFree(kv.second);
  free_.clear();
  for (auto& kv : parked_) (void)hipFree(kv.first);
  parked_.clear();
}
void DevicePool::trim() {
  std::lock_guard<std::mutex> lk(mu_);
  trim_locked();
}
DevicePool::~DevicePool() {
  trim();
  for (auto& kv : live_) (void)hipFree(kv.first);
}

void rearm_drop(wfst_ctx* ctx) {
  RearmRecord& r = ctx->rearm;
  if (!r.plan) return;
  (void)hipStreamSynchronize(ctx->stream);
  if (ctx->pool && ctx->pool->unpark(r.blk, RearmRecord::BLOCKS))
    for (void* b : r.blk) ctx->pool->free(b);
  r.clear();
  ctx->rearm_stats.dropped += 1;
}

void* PinnedBuf::get(size_t bytes) {
  if (bytes > cap) {
    if (p) (void)hipHostFree(p);
    size_t ncap = std::max<size_t>(bytes, cap * 2);
    ncap = std::max<size_t>(ncap, 4096);
    HIP_CHECK(hipHostMalloc(&p, ncap, hipHostMallocDefault));
    cap = ncap;
  }
  return p;
}
PinnedBuf::~PinnedBuf() {
  if (p) (void)hipHostFree(p);
}

std::shared_ptr<PinnedBlock> PinnedRing::take(size_t bytes) {
  PinnedBlock* blk = nullptr;
  {
    std::lock_guard<std::mutex> lk(mu_);
    size_t best = free_.size();
    for (size_t i = 0; i < free_.size(); ++i)
      if (free_[i]->cap >= bytes && (best == free_.size() || free_[i]->cap < free_[best]->cap)) best = i;
    if (best != free_.size()) {
      blk = free_[best];
      free_.erase(free_.begin() + (std::ptrdiff_t)best);
    }
  }
  if (!blk) {
    auto fresh = std::make_unique<PinnedBlock>();
    fresh->cap = (std::max<size_t>(bytes, 4096) + 65535) & ~(size_t)65535;
    HIP_CHECK(hipHostMalloc(&fresh->p, fresh->cap, hipHostMallocDefault));
    blk = fresh.release();
  }
  std::weak_ptr<PinnedRing> ring = weak_from_this();
  return std::shared_ptr<PinnedBlock>(blk, [ring](PinnedBlock* b) {
    if (auto r = ring.lock()) {
      std::lock_guard<std::mutex> lk(r->mu_);
      if (r->free_.size() < 8) {
        r->free_.push_back(b);
        return;
      }
    }
    (void)hipHostFree(b->p);
    delete b;
  });
}
PinnedRing::~PinnedRing() {
  for (PinnedBlock* b : free_) {
    (void)hipHostFree(b->p);
    delete b;
  }
}

}  // namespace wfst

DeviceArena::~DeviceArena() {
  if (base && pool) pool->free(base);
}

using namespace wfst;

static wfst_ctx* ctx_create(int device, void* stream, bool own, const uint32_t* cu_mask = nullptr, uint32_t mask_words = 0) {
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count == 0)
    throw Error("libwfst_amd: no HIP device available (this engine has no CPU fallback)");
  if (device < 0 || device >= count) throw Error("libwfst_amd: device index out of range");
  HIP_CHECK(hipSetDevice(device));
  auto ctx = std::make_unique<wfst_ctx>();
  ctx->device = device;
  if (own && cu_mask && mask_words) {
    HIP_CHECK(hipExtStreamCreateWithCUMask(&ctx->stream, mask_words, cu_mask));
    ctx->owns_stream = true;
  } else if (own) {
    HIP_CHECK(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    ctx->owns_stream = true;
  } else {
    ctx->stream = (hipStream_t)stream;
  }
  ctx->pool = std::make_shared<DevicePool>(device);
  HIP_CHECK(hipEventCreate(&ctx->ev0));
  HIP_CHECK(hipEventCreate(&ctx->ev1));
  hipDeviceProp_t prop;
  HIP_CHECK(hipGetDeviceProperties(&prop, device));
  ctx->n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  if (cu_mask && mask_words) {  // grids are sized for the CUs this context's stream may use
    int bits = 0;
    for (uint32_t w = 0; w < mask_words; ++w) bits += __builtin_popcount(cu_mask[w]);
    if (bits <= 0) throw Error("empty CU mask");
    ctx->n_cus = std::min(ctx->n_cus, bits);
  }
  return ctx.release();
}

// The body of a wfst_ctx_get_*_stats getter: counter i of `family` (common.h: fields in the order of the getter's
// parameters) goes through out[i] where that is not null.
template <class F, size_t N>
static wfst_status get_counters(wfst_ctx* ctx, F wfst_ctx::*family, uint64_t* const (&out)[N]) {
  static_assert(std::is_trivially_copyable_v<F> && sizeof(F) == N * sizeof(uint64_t));
  return wrap([&] {
    if (!ctx) throw Error("null pointer");
    uint64_t v[N];
    std::memcpy(v, &(ctx->*family), sizeof v);
    for (size_t i = 0; i < N; ++i)
      if (out[i]) *out[i] = v[i];
  });
}
// wfst_shortest_path / wfst_shortest_path_batch begin: the n1_* counters are those of this call's last sp1_wave_kernel launch
static void small_path_begin(wfst_ctx* ctx) {
  ctx->small_path.n1_in_kernel = ctx->small_path.n1_staged = ctx->small_path.n1_handed_back = 0;
}

extern "C" {

uint32_t wfst_abi_version(void) { return WFST_ABI_VERSION; }

wfst_status wfst_last_error(char** msg) {
  return wrap([&] {
    if (!msg) throw Error("null out pointer");
    std::string s = t_has_error ? t_last_error : std::string("No error message");
    t_has_error = false;
    char* out = (char*)std::malloc(s.size() + 1);
    if (!out) throw Error("out of memory");
    std::memcpy(out, s.c_str(), s.size() + 1);
    *msg = out;
  });
}
wfst_status wfst_string_destroy(char* msg) {
  std::free(msg);
  return WFST_OK;
}
wfst_status wfst_bytes_destroy(uint8_t* data) {
  std::free(data);
  return WFST_OK;
}

wfst_status wfst_ctx_create(int device, wfst_ctx** out) {
  return wrap([&] {
    if (!out) throw Error("null out pointer");
    *out = ctx_create(device, nullptr, true);
  });
}
wfst_status wfst_ctx_create_on_stream(int device, void* hip_stream, wfst_ctx** out) {
  return wrap([&] {
    if (!out) throw Error("null out pointer");
    *out = ctx_create(device, hip_stream, false);
  });
}
wfst_status wfst_ctx_create_with_cu_mask(int device, const uint32_t* cu_mask, uint32_t mask_words, wfst_ctx** out) {
  return wrap([&] {
    if (!out || !cu_mask || !mask_words) throw Error("null pointer");
    *out = ctx_create(device, nullptr, true, cu_mask, mask_words);
  });
}
wfst_status wfst_ctx_destroy(wfst_ctx* ctx) {
  return wrap([&] {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    for (hipEvent_t e : ctx->ev_chain)
      if (e) (void)hipEventDestroy(e);
    rearm_drop(ctx);  // (the pool may outlive the context: handles share it)
    ctx->solo_log.reset();
    sp_host_timing_report(ctx);
    ctx->pool.reset();
    if (ctx->owns_stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
  });
}
wfst_status wfst_ctx_synchronize(wfst_ctx* ctx) {
  return wrap([&] {
    if (!ctx) throw Error("null ctx");
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
  });
}
wfst_status wfst_ctx_stream(wfst_ctx* ctx, void** hip_stream) {
  return wrap([&] {
    if (!ctx || !hip_stream) throw Error("null pointer");
    *hip_stream = (void*)ctx->stream;
  });
}

wfst_status wfst_fst_upload(wfst_ctx* ctx, uint32_t n_states, int64_t start, const uint32_t* offsets,
                            const wfst_tr* arcs, const float* finals, uint64_t props, wfst_fst** out) {
  return wrap([&] {
    if (!ctx || !out) throw Error("null pointer");
    if (n_states && (!offsets || !finals)) throw Error("null array");
    *out = upload_from_host(ctx, n_states, start, offsets, arcs, finals, props);
  });
}
wfst_status wfst_fst_upload_device(wfst_ctx* ctx, uint32_t n_states, int64_t start, const uint32_t* d_offsets,
                                   const wfst_tr* d_arcs, const float* d_finals, uint64_t props, wfst_fst** out) {
  return wrap([&] {
    if (!ctx || !out) throw Error("null pointer");
    *out = upload_from_device(ctx, n_states, start, d_offsets, d_arcs, d_finals, props);
  });
}
wfst_status wfst_fst_upload_many(wfst_ctx* ctx, size_t n, const uint32_t* n_states, const int64_t* starts,
                                 const uint32_t* offsets_cat, const wfst_tr* arcs_cat, const float* finals_cat,
                                 const uint64_t* props, wfst_fst** outs) {
  return wrap([&] {
    if (!ctx || !outs) throw Error("null pointer");
    upload_many(ctx, n, n_states, starts, offsets_cat, arcs_cat, finals_cat, props, outs);
  });
}
wfst_status wfst_fst_from_openfst_bytes(wfst_ctx* ctx, const uint8_t* data, size_t len, wfst_fst** out) {
  return wrap([&] {
    if (!ctx || !out || !data) throw Error("null pointer");
    *out = fst_from_openfst_bytes(ctx, data, len);
  });
}
wfst_status wfst_fst_to_openfst_bytes(const wfst_fst* fst, uint8_t** data, size_t* len) {
  return wrap([&] {
    if (!fst || !data || !len) throw Error("null pointer");
    std::vector<uint8_t> buf;
    fst_to_openfst_bytes(fst, buf);
    uint8_t* p = (uint8_t*)std::malloc(buf.size() ? buf.size() : 1);
    if (!p) throw Error("out of memory");
    std::memcpy(p, buf.data(), buf.size());
    *data = p;
    *len = buf.size();
  });
}
wfst_status wfst_fst_to_openfst_const_bytes(const wfst_fst* fst, uint8_t** data, size_t* len) {
  return wrap([&] {
    if (!fst || !data || !len) throw Error("null pointer");
    std::vector<uint8_t> buf;
    fst_to_openfst_const_bytes(fst, buf);
    uint8_t* p = (uint8_t*)std::malloc(buf.size() ? buf.size() : 1);
    if (!p) throw Error("out of memory");
    std::memcpy(p, buf.data(), buf.size());
    *data = p;
    *len = buf.size();
  });
}
wfst_status wfst_fst_info(const wfst_fst* fst, uint32_t* n_states, uint64_t* n_arcs, int64_t* start, uint64_t* props) {
  return wrap([&] {
    if (!fst) throw Error("null fst");
    if (n_states) *n_states = fst->n_states;
    if (n_arcs) *n_arcs = fst->n_arcs;
    if (start) *start = fst->start;
    if (props) *props = fst->props;
  });
}
wfst_status wfst_fst_download(const wfst_fst* fst, uint32_t* offsets, wfst_tr* arcs, float* finals) {
  return wrap([&] {
    if (!fst) throw Error("null fst");
    ensure_host(fst);
    const HostCsr& h = fst->host;
    if (offsets) std::memcpy(offsets, h.offsets.data(), h.offsets.size() * sizeof(uint32_t));
    if (arcs && !h.arcs.empty()) std::memcpy(arcs, h.arcs.data(), h.arcs.size() * sizeof(wfst_tr));
    if (finals && !h.finals.empty()) std::memcpy(finals, h.finals.data(), h.finals.size() * sizeof(float));
  });
}
wfst_status wfst_fst_destroy(wfst_fst* fst) {
  return wrap([&] {
    if (!fst) return;
    (void)hipSetDevice(fst->device);
    delete fst;
  });
}

wfst_status wfst_fst_destroy_many(wfst_fst* const* fsts, size_t n) {
  return wrap([&] {
    if (n && !fsts) throw Error("null pointer");
    for (size_t i = 0; i < n; ++i) delete fsts[i];
  });
}

wfst_status wfst_compose(wfst_ctx* ctx, const wfst_fst* fst1, const wfst_fst* fst2, const wfst_compose_config* cfg,
                         wfst_fst** out) {
  return wrap([&] {
    if (!ctx || !fst1 || !fst2 || !out) throw Error("null pointer");
    wfst_compose_config c = cfg ? *cfg : wfst_compose_config{0, 1};  // ComposeConfig::default(), compose_static.rs:56-65
    if (c.compose_filter > 6) throw Error("unknown compose_filter " + std::to_string(c.compose_filter));  // compose.rs:20-33
    HIP_CHECK(hipSetDevice(ctx->device));
    *out = compose(ctx, fst1, fst2, c.connect != 0, c.compose_filter);
  });
}

// compose of n = max(n1, n2) pairs in one call; every argument is checked before anything is launched
wfst_status wfst_compose_batch(wfst_ctx* ctx, const wfst_fst* const* fst1s, size_t n1, const wfst_fst* const* fst2s, size_t n2,
                               const wfst_compose_config* cfg, wfst_fst** outs, uint8_t* in_kernel) {
  return wrap([&] {
    const size_t n = std::max(n1, n2);
    if (outs)
      for (size_t i = 0; i < n; ++i) outs[i] = nullptr;
    if (!ctx || !fst1s || !fst2s || !outs) throw Error("null pointer");
    if ((n1 != n && n1 != 1) || (n2 != n && n2 != 1))
      throw Error("compose_batch: the lists hold " + std::to_string(n1) + " and " + std::to_string(n2) +
                  " FSTs (equal lengths, or one of them 1)");
    const wfst_compose_config c = cfg ? *cfg : wfst_compose_config{0, 1};
    if (c.compose_filter > 6) throw Error("unknown compose_filter");
    if (n == 0) return;
    for (size_t i = 0; i < n1; ++i)
      if (!fst1s[i]) throw Error("item " + std::to_string(i) + ": null FST in batch");
    for (size_t i = 0; i < n2; ++i)
      if (!fst2s[i]) throw Error("item " + std::to_string(i) + ": null FST in batch");
    HIP_CHECK(hipSetDevice(ctx->device));
    compose_batch(ctx, fst1s, n1, fst2s, n2, c.connect != 0, c.compose_filter, outs, in_kernel);
  });
}
wfst_status wfst_ctx_get_compose_batch_counters(wfst_ctx* ctx, uint64_t* launches, uint64_t* items_in_kernel,
                                                uint64_t* items_single, uint64_t* items_no_start, uint64_t* regrown_states,
                                                uint64_t* regrown_arcs, uint64_t* regrown_hash) {
  return get_counters(ctx, &wfst_ctx::compose_batch, {launches, items_in_kernel, items_single, items_no_start, regrown_states,
                                                      regrown_arcs, regrown_hash});
}

// compose_with_config with matcher configs (compose_static.rs:166-266; rustfst-ffi/src/algorithms/compose.rs:199-211: an empty
// allowed list is None); without any it is wfst_compose
wfst_status wfst_compose_with_matchers(wfst_ctx* ctx, const wfst_fst* fst1, const wfst_fst* fst2, const wfst_compose_config* cfg,
                                       const wfst_matcher_config* m1, const wfst_matcher_config* m2, wfst_fst** out) {
  if (!m1 && !m2) return wfst_compose(ctx, fst1, fst2, cfg, out);
  return wrap([&] {
    if (out) *out = nullptr;
    if (!ctx || !fst1 || !fst2 || !out) throw Error("null pointer");
    wfst_compose_config c = cfg ? *cfg : wfst_compose_config{0, 1};
    if (c.compose_filter > 6) throw Error("unknown compose_filter " + std::to_string(c.compose_filter));
    SigmaSpec specs[2];
    const wfst_matcher_config* ms[2] = {m1, m2};
    for (int i = 0; i < 2; ++i) {
      if (!ms[i]) continue;
      if (ms[i]->rewrite_mode > 2) throw Error("unknown rewrite_mode " + std::to_string(ms[i]->rewrite_mode));
      if (ms[i]->n_allowed && !ms[i]->sigma_allowed_matches) throw Error("null pointer");
      specs[i] = SigmaSpec{ms[i]->sigma_label, ms[i]->rewrite_mode, ms[i]->sigma_allowed_matches, ms[i]->n_allowed};
    }
    HIP_CHECK(hipSetDevice(ctx->device));
    *out = compose_sigma(ctx, fst1, fst2, c.connect != 0, c.compose_filter, m1 ? &specs[0] : nullptr, m2 ? &specs[1] : nullptr);
  });
}
wfst_status wfst_ctx_get_compose_sigma_counters(wfst_ctx* ctx, uint64_t* levels, uint64_t* states, uint64_t* arcs,
                                             uint64_t* require1_states, uint64_t* require2_states, uint64_t* exact_items,
                                             uint64_t* sigma_items, uint64_t* sigma_arcs, uint64_t* refused_items,
                                             uint64_t* arena_grows, uint64_t* level_launches) {
  return get_counters(ctx, &wfst_ctx::compose_sigma, {levels, states, arcs, require1_states, require2_states, exact_items,
                                                      sigma_items, sigma_arcs, refused_items, arena_grows, level_launches});
}

wfst_status wfst_shortest_path(wfst_ctx* ctx, const wfst_fst* fst, const wfst_shortest_path_config* cfg,
                               wfst_fst** out) {
  return wrap([&] {
    if (!ctx || !fst || !out) throw Error("null pointer");
    wfst_shortest_path_config c = cfg ? *cfg : wfst_shortest_path_config{1e-6f, 1, 0};  // shortest_path.rs:31-39
    HIP_CHECK(hipSetDevice(ctx->device));
    small_path_begin(ctx);
    if (c.nshortest == 0) {  // shortest_path.rs:118-120: FO::new()
      HostCsr h;
      h.offsets.push_back(0);
      *out = make_host_fst(ctx, 0, -1, props::NULL_PROPS, std::move(h));
      return;
    }
    // nshortest == 1 returns before `unique` is looked at (shortest_path.rs:122-133)
    if (c.nshortest == 1) {
      *out = shortest_path_n1(ctx, fst);
      return;
    }
    // unique: the reversed FST is determinized on the host first (shortest_path.rs:157-165); acceptors only, as there
    *out = shortest_path_nbest(ctx, fst, c.nshortest, c.delta, c.unique != 0);
  });
}

wfst_status wfst_shortest_path_batch(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, const wfst_shortest_path_config* cfg,
                                     wfst_fst** outs) {
  return wrap([&] {
    if (!ctx || (n && (!fsts || !outs))) throw Error("null pointer");
    for (size_t i = 0; i < n; ++i) {
      if (!fsts[i]) throw Error("null FST in batch");
      outs[i] = nullptr;
    }
    wfst_shortest_path_config c = cfg ? *cfg : wfst_shortest_path_config{1e-6f, 1, 0};
    HIP_CHECK(hipSetDevice(ctx->device));
    small_path_begin(ctx);
    try {
      if (c.nshortest >= 2 && !c.unique) {
        shortest_path_nbest_batch(ctx, fsts, n, c.nshortest, c.delta, outs);
        return;
      }
      if (c.nshortest == 1) {  // small inputs in one launch (one wavefront each), the others one after the other
        shortest_path_n1_batch(ctx, fsts, n, outs);
        return;
      }
      if (c.nshortest >= 2 && c.unique) {  // small inputs: one launch for distances + arrays, the host stages on threads
        shortest_path_nbest_unique_batch(ctx, fsts, n, c.nshortest, c.delta, outs);
        return;
      }
      for (size_t i = 0; i < n; ++i) {
        if (c.nshortest == 0) {
          HostCsr h;
          h.offsets.push_back(0);
          outs[i] = make_host_fst(ctx, 0, -1, props::NULL_PROPS, std::move(h));
        } else if (c.nshortest == 1) {
          outs[i] = shortest_path_n1(ctx, fsts[i]);
        } else {
          outs[i] = shortest_path_nbest(ctx, fsts[i], c.nshortest, c.delta, true);  // unique: one after the other
        }
      }
    } catch (...) {
      for (size_t i = 0; i < n; ++i) {
        delete outs[i];
        outs[i] = nullptr;
      }
      throw;
    }
  });
}

wfst_status wfst_shortest_distance(wfst_ctx* ctx, const wfst_fst* fst, float* distance, uint32_t* hops) {
  return wrap([&] {
    if (!ctx || !fst || !distance) throw Error("null pointer");
    HIP_CHECK(hipSetDevice(ctx->device));
    shortest_distance(ctx, fst, distance, hops);
  });
}

// shortest_distance_with_config (shortest_distance.rs:313-336); ShortestDistanceConfig::default() when cfg == NULL
wfst_status wfst_shortest_distance_with_config(wfst_ctx* ctx, const wfst_fst* fst, const wfst_shortest_distance_config* cfg,
                                               float* distance, uint32_t* len) {
  return wrap([&] {
    if (ctx) ctx->push_stats = {};  // (before any argument is looked at: common.h)
    const wfst_shortest_distance_config c = cfg ? *cfg : wfst_shortest_distance_config{0u, 1e-6f};
    if (!(c.delta >= 0.0f) || !std::isfinite(c.delta)) throw Error("shortest_distance: delta must be finite and >= 0");
    (void)push_max_blocks_knob();
    if (!ctx || !fst || !distance) throw Error("null pointer");
    HIP_CHECK(hipSetDevice(ctx->device));
    shortest_distance_ex(ctx, fst, c.reverse != 0, distance, len);
  });
}

// push_weights_with_config (push.rs:89-118); PushWeightsConfig::default() = {KDELTA, false} when cfg == NULL
wfst_status wfst_push_weights(wfst_ctx* ctx, const wfst_fst* fst, uint32_t reweight_type, const wfst_push_weights_config* cfg,
                              wfst_fst** out) {
  return wrap([&] {
    if (out) *out = nullptr;
    if (ctx) ctx->push_stats = {};  // (before any argument is looked at: common.h)
    const wfst_push_weights_config c = cfg ? *cfg : wfst_push_weights_config{1.0f / 1024.0f, 0u};
    if (reweight_type > 1) throw Error("push_weights: unknown reweight_type " + std::to_string(reweight_type));
    if (!(c.delta >= 0.0f) || !std::isfinite(c.delta)) throw Error("push_weights: delta must be finite and >= 0");
    (void)push_max_blocks_knob();
    if (!ctx || !fst || !out) throw Error("null pointer");
    HIP_CHECK(hipSetDevice(ctx->device));
    *out = push_weights_fst(ctx, fst, reweight_type, c.remove_total_weight != 0);
  });
}

// reweight (reweight.rs:29-154) with caller-given potentials
wfst_status wfst_reweight(wfst_ctx* ctx, const wfst_fst* fst, const float* potentials, uint64_t n_potentials,
                          uint32_t reweight_type, wfst_fst** out) {
  return wrap([&] {
    if (out) *out = nullptr;
    if (ctx) ctx->push_stats = {};  // (before any argument is looked at: common.h)
    if (reweight_type > 1) throw Error("reweight: unknown reweight_type " + std::to_string(reweight_type));
    if (!potentials && n_potentials) throw Error("reweight: potentials is NULL but n_potentials > 0");
    (void)push_max_blocks_knob();
    if (!ctx || !fst || !out) throw Error("null pointer");
    HIP_CHECK(hipSetDevice(ctx->device));
    *out = reweight_fst(ctx, fst, potentials, n_potentials, reweight_type);
  });
}

// determinize_with_config (determinize_static.rs:176-190); DeterminizeConfig::default() = {KDELTA, Functional} when cfg == NULL
wfst_status wfst_determinize(wfst_ctx* ctx, const wfst_fst* fst, const wfst_determinize_config* cfg, wfst_fst** out) {
  return wrap([&] {
    if (out) *out = nullptr;
    const wfst_determinize_config c = cfg ? *cfg : wfst_determinize_config{1.0f / 1024.0f, 0u};
    if (c.det_type > 2) throw Error("determinize: unknown det_type " + std::to_string(c.det_type));
    if (!(c.delta > 0.0f) || !std::isfinite(c.delta)) throw Error("determinize: delta must be finite and > 0");
    if (!ctx || !fst || !out) throw Error("null pointer");
    HIP_CHECK(hipSetDevice(ctx->device));
    *out = determinize_fst(ctx, fst, c.delta, c.det_type);
  });
}

// determinize_with_config of n acceptors (one workgroup each); every argument is checked before anything is launched
static void null_outs(wfst_fst** outs, size_t n) {
  if (outs)
    for (size_t i = 0; i < n; ++i) outs[i] = nullptr;
}
static void check_batch_args(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, wfst_fst** outs) {  // (behind null_outs)
  if (!ctx || !fsts || !outs) throw Error("null pointer");
  for (size_t i = 0; i < n; ++i)
    if (!fsts[i]) throw Error("item " + std::to_string(i) + ": null FST in batch");
}
// The preamble of the one-workgroup-per-item batch calls, behind null_outs and the op's own config checks: the counters of
// the last call go, then the arguments are checked.  false: an empty list, nothing to do.
extern "C++" template <class Stats>  // (BatchStats, and OptimizeBatchStats of wfst_optimize_batch)
static bool begin_batch_call(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, wfst_fst** outs, Stats wfst_ctx::*stats) {
  if (ctx) ctx->*stats = {};
  if (n == 0) return false;
  check_batch_args(ctx, fsts, n, outs);
  HIP_CHECK(hipSetDevice(ctx->device));
  return true;
}
wfst_status wfst_determinize_batch(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, const wfst_determinize_config* cfg,
                                   wfst_fst** outs, uint8_t* in_kernel) {
  return wrap([&] {
    null_outs(outs, n);
    const wfst_determinize_config c = cfg ? *cfg : wfst_determinize_config{1.0f / 1024.0f, 0u};
    if (c.det_type > 2) throw Error("determinize: unknown det_type " + std::to_string(c.det_type));
    if (!(c.delta > 0.0f) || !std::isfinite(c.delta)) throw Error("determinize: delta must be finite and > 0");
    if (!begin_batch_call(ctx, fsts, n, outs, &wfst_ctx::det_batch)) return;
    determinize_batch(ctx, fsts, n, c.delta, c.det_type, outs, in_kernel);
  });
}

static float* to_malloc(const std::vector<float>& v) {  // released with wfst_bytes_destroy
  float* p = (float*)std::malloc(std::max<size_t>(v.size(), 1) * sizeof(float));
  if (!p) throw Error("out of memory");
  if (!v.empty()) std::memcpy(p, v.data(), v.size() * sizeof(float));
  return p;
}
// determinize_with_distance (determinize_static.rs:24-39)
wfst_status wfst_determinize_with_distance(wfst_ctx* ctx, const wfst_fst* fst, const float* in_dist, uint64_t n_in_dist,
                                           float delta, wfst_fst** out, float** out_dist, uint64_t* n_out_dist) {
  return wrap([&] {
    if (out) *out = nullptr;
    if (out_dist) *out_dist = nullptr;
    if (n_out_dist) *n_out_dist = 0;
    if (!(delta > 0.0f) || !std::isfinite(delta)) throw Error("determinize: delta must be finite and > 0");
    if (!in_dist && n_in_dist) throw Error("determinize_with_distance: in_dist is NULL but n_in_dist > 0");
    if (!ctx || !fst || !out || !out_dist || !n_out_dist) throw Error("null pointer");
    HIP_CHECK(hipSetDevice(ctx->device));
    std::vector<float> d;
    std::unique_ptr<wfst_fst> r(determinize_with_distance_fst(ctx, fst, in_dist, n_in_dist, delta, d));
    *out_dist = to_malloc(d);
    *n_out_dist = d.size();
    *out = r.release();
  });
}
wfst_status wfst_determinize_with_distance_batch(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n,
                                                 const float* const* in_dists, const uint64_t* n_in_dists, float delta,
                                                 wfst_fst** outs, float** out_dist, uint64_t* out_offsets, uint8_t* in_kernel) {
  return wrap([&] {
    null_outs(outs, n);
    if (out_dist) *out_dist = nullptr;
    if (!(delta > 0.0f) || !std::isfinite(delta)) throw Error("determinize: delta must be finite and > 0");
    if (ctx) ctx->det_batch = {};  // (begin_batch_call's steps, with this call's own checks between them)
    if (!out_dist || !out_offsets) throw Error("null pointer");
    out_offsets[0] = 0;
    if (n == 0) {
      *out_dist = to_malloc({});
      return;
    }
    if (!in_dists || !n_in_dists) throw Error("null pointer");
    for (size_t i = 0; i < n; ++i)
      if (!in_dists[i] && n_in_dists[i])
        throw Error("item " + std::to_string(i) + ": determinize_with_distance: in_dist is NULL but n_in_dist > 0");
    check_batch_args(ctx, fsts, n, outs);
    HIP_CHECK(hipSetDevice(ctx->device));
    std::vector<float> d;
    std::vector<uint64_t> off;
    determinize_batch(ctx, fsts, n, delta, 0, outs, in_kernel, in_dists, n_in_dists, &d, &off);
    try {
      *out_dist = to_malloc(d);
    } catch (...) {
      for (size_t i = 0; i < n; ++i) {
        delete outs[i];
        outs[i] = nullptr;
      }
      throw;
    }
    std::memcpy(out_offsets, off.data(), (n + 1) * sizeof(uint64_t));
  });
}
wfst_status wfst_ctx_get_determinize_batch_stats(wfst_ctx* ctx, uint64_t* launches, uint64_t* items_in_kernel,
                                                 uint64_t* items_single) {
  return get_counters(ctx, &wfst_ctx::det_batch, {launches, items_in_kernel, items_single});
}

// minimize_with_config (minimize.rs:92-176); MinimizeConfig::default() = {KSHORTESTDELTA, false} when cfg == NULL
wfst_status wfst_minimize(wfst_ctx* ctx, const wfst_fst* fst, const wfst_minimize_config* cfg, wfst_fst** out) {
  return wrap([&] {
    if (out) *out = nullptr;
    if (ctx) ctx->min_stats = {};  // (before any argument is looked at: common.h)
    const wfst_minimize_config c = cfg ? *cfg : wfst_minimize_config{1e-6f, 0u};
    if (!(c.delta > 0.0f) || !std::isfinite(c.delta)) throw Error("minimize: delta must be finite and > 0");
    if (!ctx || !fst || !out) throw Error("null pointer");
    HIP_CHECK(hipSetDevice(ctx->device));
    *out = minimize_fst(ctx, fst, c.delta, c.allow_nondet != 0);
  });
}
// minimize_with_config of n acceptors (one workgroup each, one launch); every argument is checked before anything is launched
wfst_status wfst_minimize_batch(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, const wfst_minimize_config* cfg,
                                wfst_fst** outs, uint8_t* in_kernel) {
  return wrap([&] {
    null_outs(outs, n);
    const wfst_minimize_config c = cfg ? *cfg : wfst_minimize_config{1e-6f, 0u};
    if (!(c.delta > 0.0f) || !std::isfinite(c.delta)) throw Error("minimize: delta must be finite and > 0");
    if (!begin_batch_call(ctx, fsts, n, outs, &wfst_ctx::min_batch)) return;
    minimize_batch(ctx, fsts, n, c.delta, c.allow_nondet != 0, outs, in_kernel);
  });
}
wfst_status wfst_ctx_get_minimize_batch_stats(wfst_ctx* ctx, uint64_t* launches, uint64_t* items_in_kernel,
                                              uint64_t* items_single) {
  return get_counters(ctx, &wfst_ctx::min_batch, {launches, items_in_kernel, items_single});
}

// tr_sum (tr_sum.rs:7-22) / tr_unique (tr_unique.rs:38-51)
wfst_status wfst_tr_sum(wfst_ctx* ctx, const wfst_fst* fst, wfst_fst** out) {
  return wrap([&] {
    if (out) *out = nullptr;
    if (!ctx || !fst || !out) throw Error("null pointer");
    HIP_CHECK(hipSetDevice(ctx->device));
    *out = tr_sum_fst(ctx, fst, false);
  });
}

wfst_status wfst_tr_unique(wfst_ctx* ctx, const wfst_fst* fst, wfst_fst** out) {
  return wrap([&] {
    if (out) *out = nullptr;
    if (!ctx || !fst || !out) throw Error("null pointer");
    HIP_CHECK(hipSetDevice(ctx->device));
    *out = tr_sum_fst(ctx, fst, true);
  });
}

// tr_sum / tr_unique of n FSTs (one workgroup each, one launch); every argument is checked before anything is launched
wfst_status wfst_tr_sum_batch(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, wfst_fst** outs, uint8_t* in_kernel) {
  return wrap([&] {
    null_outs(outs, n);
    if (!begin_batch_call(ctx, fsts, n, outs, &wfst_ctx::trsum_batch)) return;
    tr_sum_batch(ctx, fsts, n, false, outs, in_kernel);
  });
}
wfst_status wfst_tr_unique_batch(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, wfst_fst** outs, uint8_t* in_kernel) {
  return wrap([&] {
    null_outs(outs, n);
    if (!begin_batch_call(ctx, fsts, n, outs, &wfst_ctx::trsum_batch)) return;
    tr_sum_batch(ctx, fsts, n, true, outs, in_kernel);
  });
}
wfst_status wfst_ctx_get_tr_sum_batch_stats(wfst_ctx* ctx, uint64_t* launches, uint64_t* items_in_kernel, uint64_t* items_single) {
  return get_counters(ctx, &wfst_ctx::trsum_batch, {launches, items_in_kernel, items_single});
}

// optimize (optimize.rs:11-128), tropical semiring
wfst_status wfst_optimize(wfst_ctx* ctx, const wfst_fst* fst, wfst_fst** out) {
  return wrap([&] {
    if (out) *out = nullptr;
    if (!ctx || !fst || !out) throw Error("null pointer");
    HIP_CHECK(hipSetDevice(ctx->device));
    *out = optimize_fst(ctx, fst);
  });
}
// optimize of n FSTs over the four batch stages; every argument is checked before anything is launched
wfst_status wfst_optimize_batch(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, wfst_fst** outs, uint8_t* in_kernel) {
  return wrap([&] {
    null_outs(outs, n);
    if (!begin_batch_call(ctx, fsts, n, outs, &wfst_ctx::opt_batch)) return;
    optimize_batch(ctx, fsts, n, outs, in_kernel);
  });
}
wfst_status wfst_ctx_get_optimize_batch_stats(wfst_ctx* ctx, uint64_t* launches, uint64_t* items_in_kernel, uint64_t* items_single,
                                              uint64_t* items_transducer) {
  return wrap([&] {
    if (!ctx) throw Error("null pointer");
    if (launches) std::copy(ctx->opt_batch.launches, ctx->opt_batch.launches + 4, launches);
    if (items_in_kernel) *items_in_kernel = ctx->opt_batch.items_in_kernel;
    if (items_single) *items_single = ctx->opt_batch.items_single;
    if (items_transducer) *items_transducer = ctx->opt_batch.items_transducer;
  });
}

// union / concat / closure (union_static.rs:55-118, concat_static.rs:53-109, closure_static.rs:25-73) and the list forms
// (rustfst-python union_list / concat_list): every argument is checked before anything is launched
wfst_status wfst_union(wfst_ctx* ctx, const wfst_fst* a, const wfst_fst* b, wfst_fst** out) {
  return wrap([&] {
    if (out) *out = nullptr;
    if (!ctx || !a || !b || !out) throw Error("null pointer");
    HIP_CHECK(hipSetDevice(ctx->device));
    *out = union_fst(ctx, a, b);
  });
}
wfst_status wfst_concat(wfst_ctx* ctx, const wfst_fst* a, const wfst_fst* b, wfst_fst** out) {
  return wrap([&] {
    if (out) *out = nullptr;
    if (!ctx || !a || !b || !out) throw Error("null pointer");
    HIP_CHECK(hipSetDevice(ctx->device));
    *out = concat_fst(ctx, a, b);
  });
}
wfst_status wfst_closure(wfst_ctx* ctx, const wfst_fst* f, uint32_t closure_type, wfst_fst** out) {
  return wrap([&] {
    if (out) *out = nullptr;
    if (closure_type > 1) throw Error("closure: unknown closure_type " + std::to_string(closure_type));  // closure/mod.rs:9-12
    if (!ctx || !f || !out) throw Error("null pointer");
    HIP_CHECK(hipSetDevice(ctx->device));
    *out = closure_fst(ctx, f, closure_type == 0);
  });
}
static void check_list_args(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, wfst_fst** out) {
  if (out) *out = nullptr;
  if (n == 0) throw Error("fsts must be at least of len 1");  // rustfst-python/rustfst/algorithms/union.py, concat.py
  if (!ctx || !fsts || !out) throw Error("null pointer");
  for (size_t i = 0; i < n; ++i)
    if (!fsts[i]) throw Error("item " + std::to_string(i) + ": null FST in list");
}
wfst_status wfst_union_list(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, wfst_fst** out) {
  return wrap([&] {
    check_list_args(ctx, fsts, n, out);
    HIP_CHECK(hipSetDevice(ctx->device));
    *out = union_list_fst(ctx, fsts, n);
  });
}
wfst_status wfst_concat_list(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, wfst_fst** out) {
  return wrap([&] {
    check_list_args(ctx, fsts, n, out);
    HIP_CHECK(hipSetDevice(ctx->device));
    *out = concat_list_fst(ctx, fsts, n);
  });
}
// replace (replace/replace_static.rs:44-58, rustfst-ffi/src/algorithms/replace.rs): every argument is checked before anything
// is launched
wfst_status wfst_replace(wfst_ctx* ctx, uint32_t root, const wfst_label_fst_pair* pairs, size_t n, uint32_t epsilon_on_replace,
                         wfst_fst** out) {
  return wrap([&] {
    if (out) *out = nullptr;
    if (!ctx || !out || (n && !pairs)) throw Error("null pointer");
    std::vector<uint32_t> labels(n);
    std::vector<const wfst_fst*> fsts(n);
    for (size_t i = 0; i < n; ++i) {
      if (!pairs[i].fst) throw Error("item " + std::to_string(i) + ": null FST in list");
      labels[i] = pairs[i].label;
      fsts[i] = pairs[i].fst;
    }
    HIP_CHECK(hipSetDevice(ctx->device));
    *out = replace_fst(ctx, root, labels.data(), fsts.data(), n, epsilon_on_replace != 0);
  });
}
wfst_status wfst_ctx_get_replace_stats(wfst_ctx* ctx, uint64_t* levels, uint64_t* states, uint64_t* arcs, uint64_t* prefixes,
                                       uint64_t* max_depth, uint64_t* call_arcs, uint64_t* dropped_calls, uint64_t* return_arcs,
                                       uint64_t* arena_grows, uint64_t* prefix_reruns, uint64_t* level_launches) {
  return get_counters(ctx, &wfst_ctx::replace, {levels, states, arcs, prefixes, max_depth, call_arcs, dropped_calls,
                                                return_arcs, arena_grows, prefix_reruns, level_launches});
}
wfst_status wfst_rational_check_sizes(uint32_t op, const uint64_t* n_states, const uint64_t* n_arcs, size_t n) {
  return wrap([&] { rational_check_sizes(op, n_states, n_arcs, n); });
}

// state_sort (state_sort.rs:16-78) and top_sort (top_sort.rs:76-94): new handles
wfst_status wfst_state_sort(wfst_ctx* ctx, const wfst_fst* fst, const uint32_t* order, size_t n_order, wfst_fst** out) {
  return wrap([&] {
    if (out) *out = nullptr;
    if (!ctx || !fst || !out) throw Error("null pointer");
    HIP_CHECK(hipSetDevice(ctx->device));
    *out = state_sort_fst(ctx, fst, order, n_order);
  });
}
wfst_status wfst_top_sort(wfst_ctx* ctx, const wfst_fst* fst, wfst_fst** out) {
  return wrap([&] {
    if (out) *out = nullptr;
    if (!ctx || !fst || !out) throw Error("null pointer");
    HIP_CHECK(hipSetDevice(ctx->device));
    *out = top_sort_fst(ctx, fst);
  });
}
wfst_status wfst_ctx_get_top_sort_stats(wfst_ctx* ctx, uint64_t* levels, uint64_t* narrow_launches, uint64_t* wide_launches,
                                        uint64_t* narrow_levels, uint64_t* max_level_width, uint64_t* max_tree_depth,
                                        uint64_t* lift_rows, uint64_t* states_compared, uint64_t* wave_states, uint64_t* cyclic) {
  return get_counters(ctx, &wfst_ctx::top_sort, {levels, narrow_launches, wide_launches, narrow_levels, max_level_width,
                                                 max_tree_depth, lift_rows, states_compared, wave_states, cyclic});
}
// top_sort of n FSTs (one workgroup each, one launch); every argument is checked before anything is launched
wfst_status wfst_top_sort_batch(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, wfst_fst** outs, uint8_t* in_kernel) {
  return wrap([&] {
    null_outs(outs, n);
    if (!begin_batch_call(ctx, fsts, n, outs, &wfst_ctx::top_sort_batch)) return;
    top_sort_batch(ctx, fsts, n, outs, in_kernel);
  });
}
wfst_status wfst_ctx_get_top_sort_batch_counters(wfst_ctx* ctx, uint64_t* launches, uint64_t* items_in_kernel, uint64_t* items_single) {
  return get_counters(ctx, &wfst_ctx::top_sort_batch, {launches, items_in_kernel, items_single});
}

wfst_status wfst_reverse(wfst_ctx* ctx, const wfst_fst* fst, wfst_fst** out) {
  return wrap([&] {
    if (!ctx || !fst || !out) throw Error("null pointer");
    HIP_CHECK(hipSetDevice(ctx->device));
    *out = reverse_fst(ctx, fst);
  });
}

wfst_status wfst_fst_tr_sort(wfst_ctx* ctx, wfst_fst* fst, int ilabel_cmp) {
  return wrap([&] {
    if (!ctx || !fst) throw Error("null pointer");
    tr_sort_device(ctx, fst, ilabel_cmp != 0);
  });
}

wfst_status wfst_fst_set_start(wfst_ctx* ctx, wfst_fst* fst, uint32_t state) {  // mutable_fst.rs:35-44
  return wrap([&] {
    if (!ctx || !fst) throw Error("null pointer");
    if (state >= fst->n_states) throw Error("The state " + std::to_string(state) + " doesn't exist");
    std::lock_guard<std::mutex> lk(fst->cache_mu);
    if (fst->start != (int64_t)state) fst->is_string = false;  // (the string o T kernel's input is linear FROM its start state)
    fst->start = (int64_t)state;
    fst->props = props::set_start(fst->props);
    fst->rev_host.reset();  // reverse(fst) marks the old start state final (reverse.rs:80-86)
    fst->stable_sweeps.store(0, std::memory_order_relaxed);  // (the next queries are queued with a spare launch again)
    fst->bounded_streak.store(0, std::memory_order_relaxed);  // (... and with the chain of a full solve: the head may not stop from here)
    // (what a solve learned about the launch pattern of the LAST source says little about this one: the first query predicts
    // from it all the same, and a solve that outruns its prediction is continued)
  });
}

wfst_status wfst_compose_shortest_path_batch(wfst_ctx* ctx, const wfst_fst* const* acceptors, size_t n,
                                             const wfst_fst* t, const wfst_compose_config* ccfg,
                                             const wfst_shortest_path_config* scfg, wfst_fst** outs,
                                             uint64_t* composed_arcs) {
  return wrap([&] {
    if (!ctx || !t || !outs || (n && !acceptors)) throw Error("null pointer");
    wfst_compose_config c = ccfg ? *ccfg : wfst_compose_config{0, 1};
    wfst_shortest_path_config s = scfg ? *scfg : wfst_shortest_path_config{1e-6f, 1, 0};
    if (c.compose_filter > 6) throw Error("unknown compose_filter");
    if (s.nshortest != 1) throw Error("unsupported: nshortest != 1 in the fused batch");
    HIP_CHECK(hipSetDevice(ctx->device));
    compose_shortest_path_batch(ctx, acceptors, n, t, c.connect != 0, outs, composed_arcs, c.compose_filter);
  });
}

// the fused batch with matcher configs (compose_sigma_batch.hip); without any it is wfst_compose_shortest_path_batch
wfst_status wfst_compose_shortest_path_batch_with_matchers(wfst_ctx* ctx, const wfst_fst* const* acceptors, size_t n, const wfst_fst* t,
                                                           const wfst_compose_config* ccfg, const wfst_matcher_config* m1,
                                                           const wfst_matcher_config* m2, const wfst_shortest_path_config* scfg,
                                                           wfst_fst** outs, uint64_t* composed_arcs) {
  if (!m1 && !m2) return wfst_compose_shortest_path_batch(ctx, acceptors, n, t, ccfg, scfg, outs, composed_arcs);
  return wrap([&] {
    null_outs(outs, n);
    if (!ctx || !t || !outs || (n && !acceptors)) throw Error("null pointer");
    wfst_compose_config c = ccfg ? *ccfg : wfst_compose_config{0, 1};
    wfst_shortest_path_config s = scfg ? *scfg : wfst_shortest_path_config{1e-6f, 1, 0};
    if (c.compose_filter > 6) throw Error("unknown compose_filter");
    if (s.nshortest != 1) throw Error("unsupported: nshortest != 1 in the fused batch");
    SigmaSpec specs[2];
    const wfst_matcher_config* ms[2] = {m1, m2};
    for (int i = 0; i < 2; ++i) {
      if (!ms[i]) continue;
      if (ms[i]->rewrite_mode > 2) throw Error("unknown rewrite_mode " + std::to_string(ms[i]->rewrite_mode));
      if (ms[i]->n_allowed && !ms[i]->sigma_allowed_matches) throw Error("null pointer");
      specs[i] = SigmaSpec{ms[i]->sigma_label, ms[i]->rewrite_mode, ms[i]->sigma_allowed_matches, ms[i]->n_allowed};
    }
    HIP_CHECK(hipSetDevice(ctx->device));
    compose_sigma_sp_batch(ctx, acceptors, n, t, c.connect != 0, c.compose_filter, m1 ? &specs[0] : nullptr, m2 ? &specs[1] : nullptr, outs,
                           composed_arcs);
  });
}
wfst_status wfst_ctx_get_sigma_batch_counters(wfst_ctx* ctx, uint64_t* launches, uint64_t* items_in_kernel, uint64_t* items_handed_back,
                                              uint64_t* items_loop, uint64_t* exact_items, uint64_t* sigma_items, uint64_t* sigma_arcs,
                                              uint64_t* refused_items, uint64_t* max_level_width) {
  return get_counters(ctx, &wfst_ctx::sigma_batch, {launches, items_in_kernel, items_handed_back, items_loop, exact_items, sigma_items,
                                                    sigma_arcs, refused_items, max_level_width});
}

wfst_status wfst_rm_epsilon(wfst_ctx* ctx, const wfst_fst* fst, wfst_fst** out) {
  return wrap([&] {
    if (!ctx || !fst || !out) throw Error("null pointer");
    *out = nullptr;
    HIP_CHECK(hipSetDevice(ctx->device));
    *out = rm_epsilon_fst(ctx, fst);
  });
}

// rm_epsilon of n FSTs (one workgroup each); every argument is checked before anything is launched
wfst_status wfst_rm_epsilon_batch(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, wfst_fst** outs, uint8_t* in_kernel) {
  return wrap([&] {
    null_outs(outs, n);
    if (!begin_batch_call(ctx, fsts, n, outs, &wfst_ctx::rm_batch)) return;
    rm_epsilon_batch(ctx, fsts, n, outs, in_kernel);
  });
}
wfst_status wfst_ctx_get_rm_epsilon_batch_stats(wfst_ctx* ctx, uint64_t* launches, uint64_t* items_in_kernel,
                                                uint64_t* items_single) {
  return get_counters(ctx, &wfst_ctx::rm_batch, {launches, items_in_kernel, items_single});
}

wfst_status wfst_ctx_get_small_path_stats(wfst_ctx* ctx, uint64_t* n1_in_kernel, uint64_t* n1_staged, uint64_t* n1_handed_back,
                                          uint64_t* nbest_in_kernel, uint64_t* nbest_tree_full, uint64_t* nbest_out_full,
                                          uint64_t* nbest_tree_capacity) {
  return get_counters(ctx, &wfst_ctx::small_path, {n1_in_kernel, n1_staged, n1_handed_back, nbest_in_kernel, nbest_tree_full,
                                                   nbest_out_full, nbest_tree_capacity});
}

wfst_status wfst_ctx_get_compose_path_stats(wfst_ctx* ctx, uint64_t* string_answered, uint64_t* string_handed_back,
                                            uint64_t* wave_first, uint64_t* relaunch_states, uint64_t* relaunch_arcs,
                                            uint64_t* relaunch_hash, uint64_t* relaunch_path, uint64_t* switched_wide,
                                            uint64_t* two_step, uint64_t* caps_states, uint64_t* caps_arcs, uint64_t* caps_hash) {
  return get_counters(ctx, &wfst_ctx::compose_path, {string_answered, string_handed_back, wave_first, relaunch_states,
                                                     relaunch_arcs, relaunch_hash, relaunch_path, switched_wide, two_step,
                                                     caps_states, caps_arcs, caps_hash});
}

wfst_status wfst_ctx_get_string_run_stats(wfst_ctx* ctx, uint64_t* run_levels, uint64_t* runs) {
  return get_counters(ctx, &wfst_ctx::string_run, {run_levels, runs});
}

wfst_status wfst_ctx_get_determinize_stats(wfst_ctx* ctx, uint64_t* levels, uint64_t* wide_levels, uint64_t*
                                           narrow_launches, uint64_t* exit_wide_states, uint64_t* exit_wide_cands,
                                           uint64_t* exit_budget, uint64_t* exit_need, uint64_t* exit_done, uint64_t*
                                           wide_need, uint64_t* grow_states, uint64_t* grow_elts, uint64_t* grow_arcs,
                                           uint64_t* grow_cands, uint64_t* rehashes, uint64_t* cap_states, uint64_t*
                                           cap_elts, uint64_t* cap_arcs, uint64_t* cap_cands, uint64_t* rounds_max) {
  return get_counters(ctx, &wfst_ctx::det_stats, {levels, wide_levels, narrow_launches, exit_wide_states, exit_wide_cands,
                                                  exit_budget, exit_need, exit_done, wide_need, grow_states, grow_elts,
                                                  grow_arcs, grow_cands, rehashes, cap_states, cap_elts, cap_arcs, cap_cands,
                                                  rounds_max});
}

wfst_status wfst_ctx_get_minimize_stats(wfst_ctx* ctx, uint64_t* check_levels, uint64_t* check_wide_levels,
                                        uint64_t* check_narrow_launches, uint64_t* check_exit_wide, uint64_t* check_exit_done,
                                        uint64_t* levels, uint64_t* wide_levels, uint64_t* narrow_launches, uint64_t* exit_wide,
                                        uint64_t* exit_done, uint64_t* branch, uint64_t* wave_states,
                                        uint64_t* unequal_compares) {
  return get_counters(ctx, &wfst_ctx::min_stats, {check_levels, check_wide_levels, check_narrow_launches, check_exit_wide,
                                                  check_exit_done, levels, wide_levels, narrow_launches, exit_wide, exit_done,
                                                  branch, wave_states, unequal_compares});
}

wfst_status wfst_ctx_get_push_stats(wfst_ctx* ctx, uint64_t* searches, uint64_t* rounds, uint64_t* reads, uint64_t* rounds_max,
                                    uint64_t* bfs_blocks, uint64_t* arcs_blocks, uint64_t* total_blocks, uint64_t* structural,
                                    uint64_t* start_branch, uint64_t* removed) {
  return get_counters(ctx, &wfst_ctx::push_stats, {searches, rounds, reads, rounds_max, bfs_blocks, arcs_blocks, total_blocks,
                                                   structural, start_branch, removed});
}

wfst_status wfst_ctx_get_rm_epsilon_stats(wfst_ctx* ctx, uint64_t* batches, uint64_t* thread_launches, uint64_t* wave_launches,
                                          uint64_t* states_thread, uint64_t* states_wave, uint64_t* max_closure_cap) {
  return get_counters(ctx, &wfst_ctx::rm_eps, {batches, thread_launches, wave_launches, states_thread, states_wave,
                                               max_closure_cap});
}

wfst_status wfst_ctx_get_rearm_stats(wfst_ctx* ctx, uint64_t* armed, uint64_t* adopted, uint64_t* dropped) {
  return get_counters(ctx, &wfst_ctx::rearm_stats, {armed, adopted, dropped});
}
wfst_status wfst_ctx_get_bounded_stats(wfst_ctx* ctx, uint64_t* stops, uint64_t* full_solves, const char** last_reason) {
  return wrap([&] {
    if (!ctx) throw Error("null pointer");
    if (stops) *stops = ctx->bounded.stops;
    if (full_solves) *full_solves = ctx->bounded.full_solves;
    if (last_reason) *last_reason = ctx->bounded_last_refusal;
  });
}
wfst_status wfst_ctx_trim_pool(wfst_ctx* ctx) {
  return wrap([&] {
    if (!ctx || !ctx->pool) throw Error("null pointer");
    HIP_CHECK(hipSetDevice(ctx->device));
    ctx->pool->trim();
  });
}

wfst_status wfst_connect(wfst_ctx* ctx, const wfst_fst* fst, wfst_fst** out) {
  return wrap([&] {
    if (!ctx || !fst || !out) throw Error("null pointer");
    *out = nullptr;
    HIP_CHECK(hipSetDevice(ctx->device));
    *out = connect_fst(ctx, fst);
  });
}

wfst_status wfst_fst_project(wfst_ctx* ctx, wfst_fst* fst, int project_output) {
  return wrap([&] {
    if (!ctx || !fst) throw Error("null pointer");
    project_device(ctx, fst, project_output != 0);
  });
}

// invert (inversion.rs:32-48) in place, and isomorphic_with_config (isomorphic.rs:134-158, 200-212)
wfst_status wfst_fst_invert(wfst_ctx* ctx, wfst_fst* fst) {
  return wrap([&] {
    if (!ctx || !fst) throw Error("null pointer");
    invert_device(ctx, fst);
  });
}
wfst_status wfst_isomorphic(wfst_ctx* ctx, const wfst_fst* fst1, const wfst_fst* fst2, const wfst_isomorphic_config* cfg,
                            int* is_isomorphic) {
  return wrap([&] {
    if (!ctx || !fst1 || !fst2 || !is_isomorphic) throw Error("null pointer");
    *is_isomorphic = 0;
    HIP_CHECK(hipSetDevice(ctx->device));
    *is_isomorphic = isomorphic_fsts(ctx, fst1, fst2, cfg ? cfg->delta : KDELTA) ? 1 : 0;
  });
}
wfst_status wfst_ctx_get_isomorphic_counters(wfst_ctx* ctx, uint64_t* levels, uint64_t* narrow_launches, uint64_t* wide_launches,
                                             uint64_t* narrow_levels, uint64_t* max_level_width, uint64_t* pairs, uint64_t* events,
                                             uint64_t* wave_pairs, uint64_t* big_states_sorted, uint64_t* nondet_marks) {
  return get_counters(ctx, &wfst_ctx::isomorphic, {levels, narrow_launches, wide_launches, narrow_levels, max_level_width, pairs,
                                                   events, wave_pairs, big_states_sorted, nondet_marks});
}

// paths_iter (paths_iterator.rs:24-62) as a table in HBM: one handle, a list of handles, the count alone
wfst_status wfst_fst_count_paths(wfst_ctx* ctx, const wfst_fst* fst, uint64_t* count) {
  return wrap([&] {
    if (ctx) ctx->paths = {};
    if (!ctx || !fst || !count) throw Error("null pointer");
    HIP_CHECK(hipSetDevice(ctx->device));
    *count = count_paths_fst(ctx, fst);
  });
}
wfst_status wfst_fst_paths(wfst_ctx* ctx, const wfst_fst* fst, uint64_t max_paths, wfst_paths** out) {
  return wrap([&] {
    if (ctx) ctx->paths = {};
    if (!ctx || !fst || !out) throw Error("null pointer");
    HIP_CHECK(hipSetDevice(ctx->device));
    *out = paths_fst(ctx, fst, max_paths);
  });
}
wfst_status wfst_fst_paths_batch(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, uint64_t max_paths, wfst_paths** out,
                                 uint8_t* in_kernel) {
  return wrap([&] {
    if (ctx) ctx->paths = {};
    if (!ctx || !out || (n && !fsts)) throw Error("null pointer");
    for (size_t i = 0; i < n; ++i)
      if (!fsts[i]) throw Error("item " + std::to_string(i) + ": null FST in batch");
    HIP_CHECK(hipSetDevice(ctx->device));
    *out = paths_batch(ctx, fsts, n, max_paths, in_kernel);
  });
}
wfst_status wfst_paths_info(const wfst_paths* paths, uint64_t* n_items, uint64_t* n_paths, uint64_t* n_ilabels, uint64_t* n_olabels) {
  return wrap([&] {
    if (!paths) throw Error("null pointer");
    if (n_items) *n_items = paths->item_off.size() - 1;
    if (n_paths) *n_paths = paths->n_paths;
    if (n_ilabels) *n_ilabels = paths->n_il;
    if (n_olabels) *n_olabels = paths->n_ol;
  });
}
wfst_status wfst_paths_download(wfst_ctx* ctx, const wfst_paths* paths, uint64_t* item_off, float* weights, uint64_t* ilabel_off,
                                uint32_t* ilabels, uint64_t* olabel_off, uint32_t* olabels) {
  return wrap([&] {
    if (!ctx || !paths) throw Error("null pointer");
    HIP_CHECK(hipSetDevice(ctx->device));
    paths_download(ctx, paths, item_off, weights, ilabel_off, ilabels, olabel_off, olabels);
  });
}
wfst_status wfst_paths_destroy(wfst_paths* paths) {
  return wrap([&] {
    if (!paths) return;
    (void)hipSetDevice(paths->device);
    delete paths;
  });
}
wfst_status wfst_ctx_get_paths_counters(wfst_ctx* ctx, uint64_t* launches, uint64_t* items_in_kernel, uint64_t* items_single,
                                        uint64_t* levels, uint64_t* paths, uint64_t* max_path_arcs, uint64_t* saturated) {
  return get_counters(ctx, &wfst_ctx::paths, {launches, items_in_kernel, items_single, levels, paths, max_path_arcs, saturated});
}

wfst_status wfst_lookahead_create(wfst_ctx* ctx, const wfst_fst* fst1, wfst_lookahead** out) {
  return wrap([&] {
    if (!ctx || !fst1 || !out) throw Error("null pointer");
    *out = nullptr;
    HIP_CHECK(hipSetDevice(ctx->device));
    *out = lookahead_create(ctx, fst1);
  });
}

wfst_status wfst_lookahead_relabel(wfst_lookahead* la, const wfst_fst* fst2, wfst_fst** out) {
  return wrap([&] {
    if (!la || !fst2 || !out) throw Error("null pointer");
    *out = nullptr;
    if (!la->ctx) throw Error("host-only look-ahead handle");
    HIP_CHECK(hipSetDevice(la->ctx->device));
    *out = lookahead_relabel(la, fst2);
  });
}

wfst_status wfst_lookahead_fst1(const wfst_lookahead* la, const wfst_fst** out) {
  return wrap([&] {
    if (!la || !out) throw Error("null pointer");
    if (!la->fst1) throw Error("host-only look-ahead handle");
    *out = la->fst1;
  });
}

wfst_status wfst_compose_lookahead(wfst_ctx* ctx, const wfst_lookahead* la, const wfst_fst* relabeled_fst2, wfst_fst** out) {
  return wrap([&] {
    if (!ctx || !la || !relabeled_fst2 || !out) throw Error("null pointer");
    *out = nullptr;
    HIP_CHECK(hipSetDevice(ctx->device));
    *out = compose_lookahead(ctx, la, relabeled_fst2);
  });
}

wfst_status wfst_compose_lookahead_batch(wfst_ctx* ctx, const wfst_lookahead* la, const wfst_fst* const* relabeled_fst2s,
                                         size_t n, wfst_fst** outs) {
  return wrap([&] {
    if (!ctx || !la || (n && (!relabeled_fst2s || !outs))) throw Error("null pointer");
    HIP_CHECK(hipSetDevice(ctx->device));
    compose_lookahead_batch(ctx, la, relabeled_fst2s, n, outs);
  });
}
wfst_status wfst_ctx_get_lookahead_stats(wfst_ctx* ctx, uint64_t* items, uint64_t* items_no_start, uint64_t* wave_answered,
                                         uint64_t* handed_over_states, uint64_t* handed_over_width, uint64_t* overflow_arcs,
                                         uint64_t* overflow_states, uint64_t* wide_items, uint64_t* wave_regrows,
                                         uint64_t* wide_grows, uint64_t* wide_hinted, uint64_t* hint_fallbacks,
                                         uint64_t* one_limits) {
  return get_counters(ctx, &wfst_ctx::lookahead, {items, items_no_start, wave_answered, handed_over_states, handed_over_width,
                                                  overflow_arcs, overflow_states, wide_items, wave_regrows, wide_grows,
                                                  wide_hinted, hint_fallbacks, one_limits});
}

wfst_status wfst_lookahead_destroy(wfst_lookahead* la) {
  return wrap([&] {
    if (!la) return;
    if (la->ctx) (void)hipSetDevice(la->ctx->device);
    delete la;
  });
}

wfst_status wfst_lookahead_info(const wfst_lookahead* la, uint32_t* n_states, uint64_t* n_intervals, uint32_t* n_labels,
                                uint32_t* final_label) {
  return wrap([&] {
    if (!la) throw Error("null pointer");
    if (n_states) *n_states = (uint32_t)(la->data.iv_off.size() - 1);
    if (n_intervals) *n_intervals = la->data.iv.size() / 2;
    if (n_labels) *n_labels = (uint32_t)la->data.label2index.size();
    if (final_label) *final_label = la->data.final_label;
  });
}

wfst_status wfst_lookahead_download(const wfst_lookahead* la, uint32_t* interval_offsets, uint32_t* intervals,
                                    uint32_t* labels, uint32_t* indices) {
  return wrap([&] {
    if (!la) throw Error("null pointer");
    if (interval_offsets) std::copy(la->data.iv_off.begin(), la->data.iv_off.end(), interval_offsets);
    if (intervals) std::copy(la->data.iv.begin(), la->data.iv.end(), intervals);
    if (labels || indices) {
      std::vector<std::pair<uint32_t, uint32_t>> v(la->data.label2index.begin(), la->data.label2index.end());
      std::sort(v.begin(), v.end());
      for (size_t i = 0; i < v.size(); ++i) {
        if (labels) labels[i] = v[i].first;
        if (indices) indices[i] = v[i].second;
      }
    }
  });
}

wfst_status wfst_label_reachable_compute(uint32_t n_states, const uint32_t* offsets, const wfst_tr* arcs, const float* finals,
                                         int reach_input, wfst_lookahead** out) {
  return wrap([&] {
    if (!offsets || !out || (n_states && !finals) || (offsets[n_states] && !arcs)) throw Error("null pointer");
    *out = nullptr;
    for (uint32_t s = 0; s < n_states; ++s) {
      if (offsets[s] > offsets[s + 1]) throw Error("offsets are not monotone");
      for (uint32_t k = offsets[s]; k < offsets[s + 1]; ++k)
        if (arcs[k].nextstate >= n_states) throw Error("arc to a state that does not exist");
    }
    std::unique_ptr<wfst_lookahead> la(new wfst_lookahead());
    la->data.compute(n_states, offsets, arcs, finals, reach_input != 0);
    *out = la.release();
  });
}

wfst_status wfst_shortest_path_begin(wfst_ctx* ctx, const wfst_fst* fst, const wfst_shortest_path_config* cfg,
                                     wfst_sp_job** job) {
  return wrap([&] {
    if (!ctx || !fst || !job) throw Error("null pointer");
    *job = nullptr;
    wfst_shortest_path_config c = cfg ? *cfg : wfst_shortest_path_config{1e-6f, 1, 0};
    if (c.nshortest != 1) throw Error("unsupported: nshortest != 1 in the asynchronous shortest_path");
    if (ctx->sp_in_flight) throw Error("a shortest_path job is already in flight on this context");
    HIP_CHECK(hipSetDevice(ctx->device));
    *job = shortest_path_n1_begin(ctx, fst);
    ctx->sp_in_flight = true;
  });
}

wfst_status wfst_shortest_path_end(wfst_sp_job* job, wfst_fst** out) {
  return wrap([&] {
    if (!job) throw Error("null job");
    wfst_ctx* ctx = sp_job_ctx(job);
    ctx->sp_in_flight = false;
    if (!out) {
      shortest_path_n1_abandon(job);
      throw Error("null pointer");
    }
    *out = nullptr;
    HIP_CHECK(hipSetDevice(ctx->device));
    *out = shortest_path_n1_end(job);
  });
}

wfst_status wfst_compose_shortest_path_batch_begin(wfst_ctx* ctx, const wfst_fst* const* acceptors, size_t n,
                                                   const wfst_fst* t, const wfst_compose_config* ccfg,
                                                   const wfst_shortest_path_config* scfg, wfst_batch_job** job) {
  return wrap([&] {
    if (!ctx || !t || !job || (n && !acceptors)) throw Error("null pointer");
    *job = nullptr;
    wfst_compose_config c = ccfg ? *ccfg : wfst_compose_config{0, 1};
    wfst_shortest_path_config s = scfg ? *scfg : wfst_shortest_path_config{1e-6f, 1, 0};
    if (c.compose_filter > 6) throw Error("unknown compose_filter");
    if (s.nshortest != 1) throw Error("unsupported: nshortest != 1 in the fused batch");
    if (ctx->batch_in_flight) throw Error("a fused batch is already in flight on this context");
    HIP_CHECK(hipSetDevice(ctx->device));
    *job = compose_shortest_path_batch_begin(ctx, acceptors, n, t, c.compose_filter);
    ctx->batch_in_flight = true;
  });
}

wfst_status wfst_compose_shortest_path_batch_end(wfst_batch_job* job, wfst_fst** outs, uint64_t* composed_arcs) {
  return wrap([&] {
    if (!job) throw Error("null job");
    wfst_ctx* ctx = batch_job_ctx(job);
    ctx->batch_in_flight = false;
    if (!outs) {
      compose_shortest_path_batch_abandon(job);
      throw Error("null pointer");
    }
    HIP_CHECK(hipSetDevice(ctx->device));
    compose_shortest_path_batch_end(job, outs, composed_arcs);
  });
}

wfst_status wfst_fst_pack_paths(const wfst_fst* const* paths, size_t n, uint32_t max_arcs, uint32_t* out) {
  return wrap([&] {
    if ((n && !paths) || !out) throw Error("null pointer");
    const size_t rec = 4 + 4 * (size_t)max_arcs;
    for (size_t i = 0; i < n; ++i) {
      if (!paths[i]) throw Error("null path in batch");
      pack_path_record(out + i * rec, max_arcs, paths[i]);
    }
  });
}

wfst_status wfst_compose_shortest_path_batch_packed(wfst_ctx* ctx, const wfst_fst* const* acceptors, size_t n, const wfst_fst* t,
                                                    const wfst_compose_config* ccfg, const wfst_shortest_path_config* scfg,
                                                    uint32_t max_arcs, uint32_t* out, uint64_t* composed_arcs) {
  return wrap([&] {
    if (!ctx || !t || (n && (!acceptors || !out))) throw Error("null pointer");
    wfst_compose_config c = ccfg ? *ccfg : wfst_compose_config{0, 1};
    wfst_shortest_path_config s = scfg ? *scfg : wfst_shortest_path_config{1e-6f, 1, 0};
    if (c.compose_filter > 6) throw Error("unknown compose_filter");
    if (s.nshortest != 1) throw Error("unsupported: nshortest != 1 in the fused batch");
    if (ctx->batch_in_flight) throw Error("a batch is in flight on this context");
    HIP_CHECK(hipSetDevice(ctx->device));
    const PackedSink sink{max_arcs, out};
    compose_shortest_path_batch_end(compose_shortest_path_batch_begin(ctx, acceptors, n, t, c.compose_filter), nullptr, composed_arcs,
                                    &sink);
  });
}

wfst_status wfst_ctx_set_tie_order(wfst_ctx* ctx, int reference_order) {
  return wrap([&] {
    if (!ctx) throw Error("null ctx");
    ctx->tie_reference = reference_order != 0;
  });
}
wfst_status wfst_ctx_set_resident_share(wfst_ctx* ctx, uint32_t share) {
  return wrap([&] {
    if (!ctx) throw Error("null ctx");
    if (share > 1) throw Error("wfst_ctx_set_resident_share: 0 (whole device) or 1 (half)");
    ctx->resident_share = share;
  });
}
wfst_status wfst_ctx_set_profiling(wfst_ctx* ctx, int on) {
  return wrap([&] {
    if (!ctx) throw Error("null ctx");
    ctx->profiling = on == 1;
    ctx->chain_timing = on == 2;
    if (ctx->chain_timing && !ctx->ev_chain[0]) {
      HIP_CHECK(hipEventCreate(&ctx->ev_chain[0]));
      HIP_CHECK(hipEventCreate(&ctx->ev_chain[1]));
    }
  });
}
wfst_status wfst_ctx_get_stats(wfst_ctx* ctx, wfst_stats* out) {
  return wrap([&] {
    if (!ctx || !out) throw Error("null pointer");
    *out = ctx->stats;
  });
}
wfst_status wfst_ctx_get_sweep_trace(wfst_ctx* ctx, double* ms, uint64_t* arcs, uint64_t* states, size_t cap, size_t* n) {
  return wrap([&] {
    if (!ctx || !n) throw Error("null pointer");
    *n = ctx->sweep_trace.size();
    for (size_t i = 0; i < std::min(cap, *n); ++i) {
      if (ms) ms[i] = ctx->sweep_trace[i].ms;
      if (arcs) arcs[i] = ctx->sweep_trace[i].arcs;
      if (states) states[i] = ctx->sweep_trace[i].states;
    }
  });
}
wfst_status wfst_ctx_get_sweep_modes(wfst_ctx* ctx, uint32_t* modes, size_t cap, size_t* n) {
  return wrap([&] {
    if (!ctx || !n) throw Error("null pointer");
    *n = ctx->sweep_trace.size();
    for (size_t i = 0; i < std::min(cap, *n); ++i)
      if (modes) modes[i] = ctx->sweep_trace[i].mode;
  });
}
wfst_status wfst_ctx_reset_stats(wfst_ctx* ctx) {
  return wrap([&] {
    if (!ctx) throw Error("null ctx");
    ctx->stats = wfst_stats{};
  });
}

}  // extern "C"
