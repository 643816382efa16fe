// sssp_solo.h — the solo query: a repeated bounded single-shortest-path query answered in ONE launch of ONE workgroup.
//
// Included by sssp.hip inside namespace wfst { namespace { ... } } behind sssp_tail_kernel (it calls the tail's search and walk).
//
// Where the host would queue "the bounded head and nothing behind it" on re-armed scratch (shortest_path_n1_begin), this kernel
// does the whole query on the parked key[] as the re-arm launch left it — every word KEY_INF:
//   seed    the start state's key and list entry (mbox_narrow's own seeding);
//   search  mbox_narrow<12, true, true>: the bounded head's level loop, dropping what it cannot settle (the argument stands
//           above that function);
//   path    on a stop, the tail's search over the handle's whole list of final states and the walk, by this workgroup: no
//           hand-over between workgroups, and TailOut written as sssp_tail_kernel writes it;
//   clean   stop or abort: key[s] = KEY_INF for every state the search wrote (the log), so the scratch is armed again — no
//           other word of the scratch, and nothing of the control block, is touched;
//   ticket  TailOut::solo says stopped or aborted (SOLO_*), then the fence, then TailOut::done.
// It waits for no other workgroup; its loops are bounded by NW_MAX_LEVELS, the list sizes, the log and the path buffer.
// A log that overflows cannot say which keys to put back: every key is cleaned instead (n stores by one workgroup, on the way
// to an ordinary solve of the same query).

constexpr uint32_t SOLO_ANSWERED = 1, SOLO_ABORT_BAND = 2, SOLO_ABORT_GREW = 3, SOLO_ABORT_LOG = 4, SOLO_ABORT_OTHER = 5;  // TailOut::solo
constexpr uint32_t SOLO_LOG_CAP = 8192;  // entries of the log (wfst_ctx::solo_log); WFST_SSSP_SOLO_LOG caps it further

__global__ void __launch_bounds__(MB_THREADS) sssp_solo_kernel(const uint32_t* __restrict__ offsets, const uint2* __restrict__ wn,
                                                               uint64_t* __restrict__ key, uint32_t n, uint32_t start, float tau0,
                                                               const float* __restrict__ finals, const uint2* __restrict__ fin_list,
                                                               uint32_t n_fin, const wfst_tr* __restrict__ arcs,
                                                               const uint32_t* __restrict__ rev_off, const uint4* __restrict__ rev_arc,
                                                               wfst_tr* __restrict__ out, uint32_t out_cap, TailOut* __restrict__ hout,
                                                               uint32_t* __restrict__ log, uint32_t log_cap, uint32_t done_ticket) {
  __shared__ uint4 s_wl[2 * NW_CAP];
  __shared__ uint32_t s_n[16];
  __shared__ unsigned long long s_best[MB_THREADS / 64];
  __shared__ uint2 s_walk[WALK_LDS];
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  uint32_t seed_off = 0;
  if (tid < 2) seed_off = offsets[start + tid];  // (lanes 0 and 1 of the first wave, as mbox_narrow reads them)
  if (tid == 0) {  // (mbox_narrow writes words 0..11 and has a barrier in front of its first level)
    s_n[12] = 0;
    s_n[13] = 1;  // the start state is entry 0
    s_n[14] = log_cap;
    s_n[15] = BOUNDED_WHY_OTHER;
  }
  MboxView mb{};
  mb.nb = 1;
  mbox_narrow<MB_LOG, true, true>(offsets, wn, key, mb, nullptr, nullptr, 0u, tau0, 0u, 0u, 0u, 1u, false, 0u, s_wl, s_n, 0u, nullptr,
                                  nullptr, nullptr, start + 1u, seed_off, finals, log);
  __syncthreads();
  const uint32_t why = s_n[15], logged = s_n[13], hop_pad = s_n[12] ? 1u : 0u;
  const bool full = logged > log_cap;  // (uniform, like `stop`)
  const bool stop = why == 0u && !full;
  if (stop) {  // every key at or below B is exact, every other key is above B or KEY_INF: the tail's search and walk
    unsigned long long best = KEY_INF;
    bool tie = false;
    tail_search_list(key, fin_list, n_fin, tid, MB_THREADS, best, tie);
    tail_wave_reduce(best, tie);
    if (lane == 0) s_best[tid >> 6] = tail_pack(best, tie);
    __syncthreads();
    if (tid < 64) {
      best = KEY_INF;
      tie = false;
      if (lane < MB_THREADS / 64) tail_merge_packed(best, tie, s_best[lane]);
      tail_wave_reduce(best, tie);
      (void)tail_walk_publish(best, tie, hop_pad, finals, key, offsets, arcs, rev_off, rev_arc, out, out_cap, hout, nullptr, s_walk);
    }
  }
  __syncthreads();  // the walk has read its last key
  if (full) {
    for (uint32_t i = tid; i < n; i += MB_THREADS) key[i] = KEY_INF;
  } else {
    // (the log was written by other waves of this workgroup: read past the L1)
    for (uint32_t i = tid; i < logged; i += MB_THREADS) key[__hip_atomic_load(&log[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)] = KEY_INF;
  }
  __syncthreads();  // every key is KEY_INF again
  if (tid >= 64) return;
  if (lane == 0) {
    if (!stop) {
      hout->has_path = 0u;
      hout->hops = 0u;
      hout->pad = hop_pad;
      hout->f_parent = 0u;
      hout->final_weight = INF;
      hout->total = INF;
      hout->ties = 0u;
    }
    hout->early = EARLY_UNCHECKED;
    hout->early_src = 0u;
    hout->rearmed = 1u;  // (the scratch is armed: it never stopped being parked)
    hout->bounded_why = stop ? 0u : full ? BOUNDED_WHY_OTHER : why;
    hout->solo = stop                       ? SOLO_ANSWERED
                 : full                     ? SOLO_ABORT_LOG
                 : why == BOUNDED_WHY_BAND ? SOLO_ABORT_BAND
                 : why == BOUNDED_WHY_GREW ? SOLO_ABORT_GREW
                                           : SOLO_ABORT_OTHER;
    hout->solo_cleaned = full ? n : logged;
  }
  host_stores_done();
  if (lane == 0) __hip_atomic_store(&hout->done, done_ticket, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// wfst_ctx_parked_key_check: the words of a parked key[] that are not KEY_INF (a test's view of "the scratch is armed")
__global__ void __launch_bounds__(256) sssp_key_check_kernel(const uint64_t* __restrict__ key, uint32_t n,
                                                            unsigned long long* __restrict__ not_inf) {
  unsigned long long c = 0;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) c += key[i] != KEY_INF ? 1ull : 0ull;
  for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d);
  if ((threadIdx.x & 63u) == 0 && c) atomicAdd(not_inf, c);
}
