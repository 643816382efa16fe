// sssp.hip — n=1 shortest path on an HBM-resident CSR: frontier-synchronous tropical relaxation.
//
// Replaces rustfst::algorithms::shortest_path for nshortest == 1:
//   single_shortest_path            rustfst/src/algorithms/shortest_path.rs:173-239
//   single_shortest_path_backtrace  rustfst/src/algorithms/shortest_path.rs:241-282
// The reference relaxes states one at a time in AutoQueue order (queues/auto_queue.rs:23-99: top order
// on lattices, FIFO inside cyclic SCCs).  Here every frontier state of a sweep is relaxed at once:
//   key[t] = (order-preserving f32 bits of d[t]) << 32 | hops[t]      one u64 per state
//   relax arc (s,w,t):  cand = (enc(d[s] + w) << 32) | (hops[s] + 1);  atomicMin(&key[t], cand)
// The least fixed point of that recurrence is unique (f32 + is monotone), so the result does not depend
// on scheduling.  Ties are resolved canonically (DESIGN.md §Shortest path): fewest arcs, then the
// smallest (source state, arc position) predecessor, then the smallest final state id.
// No MFMA: this is sparse DP; the bound is HBM / L2-atomic traffic (20 B per arc relaxed by the
// SURVEY §8(d) accounting; this layout actually streams 8 B of arc + one 8-B atomic).
#include <cstdlib>
#include <cerrno>
#include <cstdio>
#include <sys/stat.h>
#include <sys/types.h>
#include <cstddef>
#include <chrono>
#include <cstring>
#include <initializer_list>
#include <optional>

#include <fcntl.h>
#include <sys/file.h>
#include <unistd.h>

#include "common.h"
#include "fst_props.h"

namespace wfst {

namespace {

constexpr uint64_t KEY_INF = ~0ull;
constexpr uint32_t GROUP = 16;  // lanes cooperating on one frontier state (average fan-out ~10)

// What the tail writes for the host is in host memory before a ticket stored after this is.  (Waiting for the stores'
// acknowledgements alone — `s_waitcnt vmcnt(0)`, without the L2 write-back of the system-scope fence — is NOT enough even
// for fine-grained pinned memory: measured, a 512-problem batch read results that had not landed.  The fence costs the
// tail kernel ~2 us.)
__device__ __forceinline__ void host_stores_done() { __threadfence_system(); }

// Near-far schedule (a Delta-stepping relative that needs no buckets): sweep k only relaxes active states
// with d <= tau_k; the others stay in the frontier.  When a sweep activates nothing near, tau advances by
// delta (doubling on consecutive empty sweeps so that gaps are crossed in log time).  All of it is decided on
// the device from a few words per sweep kept in a ring, so sweeps still launch back-to-back without a host
// round trip.  When the near set is too small to fill the GPU (< near_low activations: such a sweep costs the
// launch floor whatever it does) and shrinking — the tail of a band — the band is widened by delta at once
// instead of draining through half a dozen near-empty sweeps.  Activations are counted with ONE atomicAdd per workgroup on a
// counter sharded 16 ways (same-address atomics serialise at ~12 ns each).
constexpr uint32_t RING = 256;
constexpr uint32_t NEAR_SHARDS = 16;
constexpr uint32_t NEAR_RING = 4;     // sweep k writes slot k % 4, reads k-1 and k-2, recycles k+1
constexpr uint32_t NEAR_STRIDE = 32;  // one shard per 128-B line: atomics on one LINE serialise like one address
constexpr uint32_t PROF_STRIDE = 16;  // u64 counters: one shard per 128-B line
constexpr uint32_t NF_STRIDE = 16;
constexpr uint32_t PROF_SHARDS = 64;
constexpr uint32_t IMP_RING = 512;  // per-sweep "something happened" flags, indexed by sweep % IMP_RING

struct Ctl {
  uint32_t base;          // first sweep index of the batch being replayed (its launches add their static offsets)
  float tau0;             // threshold of sweep 0 (a multiple of delta)
  uint32_t tau[RING];     // f32 bits of the threshold used by sweep k (written by sweep k, read by sweep k+1)
  // number of activations with d <= tau_k made by sweep k: counter sharded 16 ways, shard j at [j * NEAR_STRIDE]
  uint32_t near[NEAR_RING][NEAR_SHARDS * NEAR_STRIDE];
  // atomic sweeps / binned levels: states left in the frontier BEYOND the threshold by sweep k (re-flagged far states and
  // far activations; an upper bound — a state may be counted twice), sharded like `near`.  With `near` it predicts the
  // next level's frontier, which decides the kernel that relaxes it (sssp_binned.h)
  uint32_t far[NEAR_RING][NEAR_SHARDS * NEAR_STRIDE];
  uint32_t streak[RING];  // consecutive sweeps before k that activated nothing near
  // mailbox sweeps: the mode launch k ran in (MODE_*), and the number of states waiting beyond the threshold (sharded like
  // `near`; a block adds the change of its own count, unsigned wrap-around)
  uint32_t mode[RING];
  // mailbox sweeps: what launch k counted, sharded like `near`, one u64 per shard: low word = near activations (the
  // states it expanded), high word = states left waiting beyond the threshold (every block reports its own, asleep or not)
  unsigned long long nf[NEAR_RING][NEAR_SHARDS * NF_STRIDE];
  // arcs / states relaxed so far (profiling only): sharded like `near`, shard j at [j * PROF_STRIDE]
  unsigned long long arcs[PROF_SHARDS * PROF_STRIDE];
  unsigned long long states[PROF_SHARDS * PROF_STRIDE];
  unsigned long long best;    // enc(total) << 32 | final state
  // backtrace header
  uint32_t f_parent, hops;
  float final_weight, total;
  uint32_t has_path, pad;
  // fused tail (sssp_tail_kernel): per-workgroup best final state, and the ticket that tells the last workgroup it is last
  unsigned long long tail_best[128];
  uint32_t tail_ticket, tail_pad;
  // early tail (sssp_early_tail): the least enc(d) a NARROW launch k wrote into key[] (all ones: it lowered nothing), and
  // what the extra workgroup of such a launch found while the others were still relaxing — (best | TIE_BIT) as in tail_best,
  // and the launch it ran in (0 = none: launch 0 never runs it).  sssp_tail_kernel decides whether that result stands.
  uint32_t narrow_low[RING];
  unsigned long long early_best;
  uint32_t early_sweep;
  // the resident launch that left every block's best final state in MboxView::blk_best on its COLLECT exit (0 = none: a
  // resident launch that hands over is never launch 0); the early tail of launch blk_best_sweep + 1 merges those words
  uint32_t blk_best_sweep;
  // the fused tail's verdict for the re-arm launch queued behind it (sssp_mbox_rearm_kernel): 1 = the solve reached its fixed
  // point inside the batch and the host will not read the keys again — clean the scratch for the next solve.  Written by every
  // fused tail that has such a launch behind it; the cleaning itself leaves the word alone.
  uint32_t rearm;
  // the bounded head (mbox_narrow<LOG, true>): launch + 1 of the head that ended the search once the best final state was
  // settled (0 = none), and enc(B), the best total it had seen.  Every later launch of the chain reads the first word with its
  // schedule words (mbox_sched_load) and leaves at entry.  bounded_why: why a bounded head that ran did NOT stop (BOUNDED_WHY_*).
  uint32_t bounded_launch, bounded_b, bounded_why;
};
constexpr uint32_t BOUNDED_WHY_BAND = 1, BOUNDED_WHY_GREW = 2, BOUNDED_WHY_OTHER = 3;
constexpr uint32_t TAIL_BLOCKS = 128;
constexpr uint32_t TAIL_LIST_BLOCKS = 16;  // ... over the handle's list of final states (RevCsr::fin), 4096 entries each
// what the host needs from the tail of a solve, written straight into pinned memory by sssp_tail_kernel
struct TailOut {
  uint32_t has_path, hops, pad, f_parent;
  float final_weight, total;
  uint32_t done;  // the launch's ticket, written last (after a system-scope fence): the host waits for this word instead of
                  // a HIP event (an event / stream wait retires the stream's finished launches first: ~15 us when ten of them
                  // are waiting, on the critical path of every query)
  uint32_t ties;  // states of the returned path with more than one optimal predecessor (the start state: with any), + 1 when
                  // several final states attain the optimum: 0 = the optimum is unique (wfst_stats.tied_choices)
  uint32_t early;  // EARLY_*: what sssp_tail_kernel made of the early tail's result
  uint32_t early_src;  // EARLY_SRC_*: where the early tail that published last took the best final state from
  uint32_t rearmed;    // Ctl::rearm as this launch wrote it (0 from a tail without a re-arm launch behind it): the host parks the scratch
  uint32_t bounded_why;  // Ctl::bounded_why: why the bounded head of this solve did not end it (0: it did, or there was none)
  uint32_t solo;         // SOLO_* (sssp_solo.h): the solo query's verdict; never written by another kernel
  uint32_t solo_cleaned;  // ... and the keys it put back to KEY_INF (n: every key, behind a log that overflowed)
};
constexpr uint32_t EARLY_UNCHECKED = 0, EARLY_USED = 1, EARLY_ABSENT = 2, EARLY_REFUTED = 3;
constexpr uint32_t EARLY_SRC_LIST = 1, EARLY_SRC_BLOCKS = 2;
// what the extra workgroup of a mailbox launch needs for the tail's work (sssp_early_tail); by value, last kernel argument
struct EarlyTail {
  const uint2* fin_list;  // RevCsr::fin
  const float* finals;
  const wfst_tr* arcs;
  const uint32_t* rev_off;
  const uint4* rev_arc;
  wfst_tr* out;   // pinned host memory
  TailOut* hout;  // pinned host memory
  uint32_t n_fin, out_cap;
  uint32_t blk_best_on;  // the resident launches of this solve leave the blocks' best final states (mbox_blk_best)
  uint32_t seed;  // launch 0 on re-armed scratch: start state + 1 — the owner of its block seeds it (0: a set-up launch did)
};
__device__ __forceinline__ void sssp_early_tail(const EarlyTail& et, const uint32_t* __restrict__ offsets, const uint64_t* __restrict__ key,
                                Ctl* __restrict__ ctl, uint32_t prev_flag, uint32_t sweep, unsigned long long* lds, bool merged,
                                unsigned long long best, bool tie);

// threshold of sweep k from what sweep k-1 left in the ring (every thread computes the same value)
// Called by one full wave (all 64 lanes): lanes 0..15 fetch the shards of sweep-1's counter, lanes 16..31 those of
// sweep-2's, so the whole decision costs one load latency.
__device__ __forceinline__ float sweep_tau(const Ctl* ctl, uint32_t sweep, float delta, uint32_t near_low,
                                           uint32_t* streak, uint32_t* prev_near, uint32_t* frontier_est = nullptr) {
  *streak = 0;
  *prev_near = 0;
  if (frontier_est) *frontier_est = 1u;
  if (sweep == 0) return ctl->tau0;
  const uint32_t p = (sweep - 1) % RING;
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t mine = 0;
  if (lane < NEAR_SHARDS) mine = ctl->near[(sweep - 1) % NEAR_RING][lane * NEAR_STRIDE];
  else if (lane < 2 * NEAR_SHARDS && sweep >= 2) mine = ctl->near[(sweep - 2) % NEAR_RING][(lane - NEAR_SHARDS) * NEAR_STRIDE];
  else if (lane >= 2 * NEAR_SHARDS && lane < 3 * NEAR_SHARDS && frontier_est) mine = ctl->far[(sweep - 1) % NEAR_RING][(lane - 2 * NEAR_SHARDS) * NEAR_STRIDE];
  const float prev = __uint_as_float(ctl->tau[p]);
  const uint32_t prev_streak = ctl->streak[p];
  for (int d = 8; d >= 1; d >>= 1) mine += __shfl_xor(mine, d);  // sums inside each group of 16 lanes
  const uint32_t cnt = __shfl(mine, 0), before = __shfl(mine, 16), far = __shfl(mine, 32);
  *prev_near = cnt;
  float t = prev;
  if (cnt >= near_low) {
    t = prev;
  } else if (cnt) {
    // a near set that cannot fill the GPU AND is shrinking (the tail of a band, not its growing head):
    // widen the band by delta and keep relaxing
    t = cnt < before ? prev + delta : prev;
  } else {
    const uint32_t st = min(prev_streak + 1u, 30u);
    *streak = st;
    t = prev + delta * (float)(1u << (st - 1u));
  }
  // the states this sweep will find near: what the last one activated below the threshold, plus — when the threshold moves —
  // at most everything that waits beyond it
  if (frontier_est) *frontier_est = cnt + (t != prev ? far : 0u);
  return t;
}

// ---- what sssp_tail_kernel, the early tail (sssp_early_tail) and the resident launch's epilogue share: the arg-min over final states.
// (enc(total) << 32 | final state) and whether ANOTHER final state attains the same total: merged pairwise; where the pair
// travels as one word the flag sits in bit 31 of the state word (state ids have 31 bits)
constexpr unsigned long long TIE_BIT = 1ull << 31;
__device__ __forceinline__ void tail_merge(unsigned long long& best, bool& tie, unsigned long long o, bool o_tie) {
  if (o == KEY_INF) return;
  if ((o >> 32) == (best >> 32)) {
    tie = true;
    best = o < best ? o : best;
  } else if (o < best) {
    best = o;
    tie = o_tie;
  }
}
__device__ __forceinline__ unsigned long long tail_pack(unsigned long long best, bool tie) {
  return best == KEY_INF ? best : (best | (tie ? TIE_BIT : 0ull));
}
__device__ __forceinline__ void tail_merge_packed(unsigned long long& best, bool& tie, unsigned long long o) {
  tail_merge(best, tie, o == KEY_INF ? o : (o & ~TIE_BIT), o != KEY_INF && (o & TIE_BIT) != 0ull);
}
__device__ __forceinline__ void tail_wave_reduce(unsigned long long& best, bool& tie) {
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long o = __shfl_xor(best, d);
    const bool ot = __shfl_xor((int)tie, d) != 0;
    tail_merge(best, tie, o, ot);
  }
}
__device__ __forceinline__ void tail_candidate(uint64_t k /* key[s] */, uint32_t s, float f, unsigned long long& best, bool& tie) {
  if (k == KEY_INF) return;
  const float tot = (key_f32((uint32_t)(k >> 32)) + f) + 0.0f;  // d[s] (x) rho(s), shortest_path.rs:214-220
  if (!(tot < INF)) return;
  tail_merge(best, tie, ((unsigned long long)f32_key(tot) << 32) | s, false);
}

#include "sssp_mailbox.h"
#include "sssp_resident.h"
#include "sssp_binned.h"

// Initial state of a solve in ONE launch (five memsets + an init kernel cost five more launch gaps): every key and shadow
// +inf except the start state (d = 1-bar, 0 hops: shortest_path.rs:204), both flag buffers clear except the start state's
// flag in buffer 0, the activity ring and the control block zeroed.
__global__ void __launch_bounds__(256) sssp_setup_kernel(uint64_t* __restrict__ key, uint32_t* __restrict__ shadow,
                                                         uint32_t* __restrict__ flag_words, uint32_t n_flag_words,
                                                         uint32_t* __restrict__ improved, Ctl* __restrict__ ctl, uint32_t n,
                                                         uint32_t start, float tau0) {
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x, nt = gridDim.x * blockDim.x;
  for (uint32_t i = tid; i < n; i += nt) {
    const bool is_start = i == start;
    key[i] = is_start ? (uint64_t)f32_key(0.0f) << 32 : KEY_INF;
    shadow[i] = is_start ? f32_key(0.0f) : 0xFFFFFFFFu;
  }
  for (uint32_t i = tid; i < n_flag_words; i += nt) flag_words[i] = i == (start >> 2) ? 1u << (8u * (start & 3u)) : 0u;
  for (uint32_t i = tid; i < IMP_RING; i += nt) improved[i] = 0;
  // control block: rings, counters and header zero, except the first threshold and the best-final key (+inf)
  uint32_t* cw = (uint32_t*)ctl;
  constexpr uint32_t W_TAU0 = offsetof(Ctl, tau0) / 4, W_BEST = offsetof(Ctl, best) / 4;
  for (uint32_t i = tid; i < (uint32_t)(sizeof(Ctl) / 4); i += nt)
    cw[i] = i == W_TAU0 ? __float_as_uint(tau0) : (i == W_BEST || i == W_BEST + 1) ? 0xFFFFFFFFu : 0u;
}

// One sweep: relax every arc leaving the current frontier.
// The frontier is a byte flag per state (idempotent plain stores: no queue, no dedupe atomics); a wave
// scans 64 flags with one coalesced load + ballot, then GROUP lanes share each active state so its arcs
// (contiguous 8-B {w,next} records) are read by consecutive lanes.  The only atomic is the atomicMin of
// relaxations that pass the plain pre-check.
//
// Chasing: a relaxation that improves a target to a NEAR distance does not flag it for the next sweep but puts it on a
// small list private to the wave (LDS); after its flagged states the wave relaxes the listed ones too, up to
// `chase_rounds` states per launch (narrow frontiers are followed deep, growing ones are cut off), spilling to the flags
// whatever does not fit (`chase_cap` entries) or is left over — only in sweeps that follow one with fewer than
// `chase_low` near activations, and only by waves that had at most CHASE_OWN_MAX flagged states of their own.  A sweep
// costs a launch plus a chain of dependent memory trips (~7 us) however small its frontier is, and half of the sweeps
// of a solve are that small (the head and the tail of every band): chasing walks several levels of such a frontier
// inside one launch.  The fixed point does not depend on the order of relaxations, so results are unchanged; an entry
// whose key has been improved again since it was listed is dropped (the improver listed or flagged the state itself).
constexpr uint32_t CHASE_MAX = 128;  // list entries per wave (ring)
constexpr uint32_t CHASE_OWN_MAX = 4;

__global__ void __launch_bounds__(256) sssp_relax_kernel(const uint32_t* __restrict__ offsets,
                                                         const uint2* __restrict__ wn, uint64_t* __restrict__ key,
                                                         uint8_t* __restrict__ flags_cur,
                                                         uint8_t* __restrict__ flags_next, uint32_t n,
                                                         uint32_t* __restrict__ improved_ring, Ctl* __restrict__ ctl,
                                                         uint32_t sweep_offset, float delta, uint32_t near_low,
                                                         uint32_t* __restrict__ shadow, uint32_t chase_cap,
                                                         uint32_t chase_rounds, uint32_t chase_low, uint32_t profile,
                                                         uint32_t dense_low) {
  // `dense_low` (binned levels, sssp_binned.h; 0xFFFFFFFF = never): this launch is the first of its slot — it predicts the
  // level's frontier, publishes the mode, and leaves the level to the binned kernels behind it when the frontier is that large
  // the sweep index is (device-side batch base) + (static offset of this launch)
  const uint32_t sweep = ctl->base + sweep_offset;
  uint32_t* improved = improved_ring + (sweep % IMP_RING);
  __shared__ uint32_t s_any;   // some activity (improvement or deferral) in this workgroup
  __shared__ uint32_t s_near;  // near activations of this workgroup
  __shared__ float s_tau;
  __shared__ unsigned long long s_prof[2];  // arcs, states relaxed by this workgroup (profiling)
  __shared__ uint32_t s_small;             // the previous sweep left fewer than chase_low near activations
  __shared__ uint32_t s_far, s_dense;
  __shared__ uint2 s_chase[4][CHASE_MAX];  // {state, enc(d) it was listed with}
  const uint32_t slot = sweep % RING;
  const bool bin_on = dense_low != 0xFFFFFFFFu;
  if (threadIdx.x < 64) {
    uint32_t streak, prev_near, est = 0;
    const float t0 = sweep_tau(ctl, sweep, delta, near_low, &streak, &prev_near, bin_on ? &est : nullptr);
    const bool dense = bin_on && sweep > 0 && est >= dense_low;
    if (threadIdx.x == 0) {
      s_small = prev_near < chase_low ? 1u : 0u;
      s_prof[0] = 0;
      s_prof[1] = 0;
      s_tau = t0;
      s_any = 0;
      s_near = 0;
      s_far = 0;
      s_dense = dense ? 1u : 0u;
    }
    if (blockIdx.x == 0) {
      if (threadIdx.x == 0) {
        ctl->tau[slot] = __float_as_uint(t0);
        ctl->streak[slot] = streak;
        if (bin_on) ctl->mode[slot] = dense ? BN_MODE_DENSE : 0u;
      }
      if (threadIdx.x < NEAR_SHARDS) {  // recycle
        ctl->near[(sweep + 1) % NEAR_RING][threadIdx.x * NEAR_STRIDE] = 0;
        if (bin_on) ctl->far[(sweep + 1) % NEAR_RING][threadIdx.x * NEAR_STRIDE] = 0;
      }
    }
  }
  __syncthreads();
  if (s_dense) return;  // a dense level: sssp_bin_expand_kernel / sssp_bin_apply_kernel, queued behind this launch, relax it
  const float tau = s_tau;
  // only sweeps that follow a small one chase (a big sweep is not bound by its launch, and relaxing a state the moment
  // it is first improved, before the rest of the sweep's candidates for it have arrived, costs re-relaxations)
  if (!s_small) chase_cap = 0;
  uint32_t own_states = 0;  // flagged near states this wave relaxed itself
  uint32_t near_cnt = 0, far_cnt = 0;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t sub = lane % GROUP;         // lane inside its group
  const uint32_t grp = lane / GROUP;         // group inside the wave (0..3)
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint32_t n_waves = (gridDim.x * blockDim.x) >> 6;
  uint2* const chase = s_chase[threadIdx.x >> 6];
  uint32_t c_head = 0, c_tail = 0;  // wave-uniform ring positions (monotone; slot = position % CHASE_MAX)
  const uint64_t lanes_below = (1ull << lane) - 1ull;
  unsigned long long p_arcs = 0, p_states = 0;
  bool any = false;

  // the target of a successful relaxation: listed if it is near and there is room, flagged otherwise
  auto activate = [&](bool won, uint32_t t, uint32_t enc_d, float d) {
    const bool near = won && d <= tau;
    if (won) shadow[t] = enc_d;
    bool flag = won && !near;
    if (chase_cap) {
      const uint64_t bm = __ballot(near);
      if (bm) {
        const uint32_t room = chase_cap - (c_tail - c_head);
        const uint32_t rank = (uint32_t)__popcll(bm & lanes_below);
        if (near) {
          if (rank < room) chase[(c_tail + rank) % CHASE_MAX] = make_uint2(t, enc_d);
          else flag = true;
        }
        c_tail += min(room, (uint32_t)__popcll(bm));
      }
    } else {
      flag = won;
    }
    if (flag) {
      flags_next[t] = 1;
      any = true;
      near_cnt += near ? 1u : 0u;
      far_cnt += near ? 0u : 1u;
    }
  };

  // relaxes the arcs of up to 64 states: lane i owns state i of the chunk (act, its key, its arc range)
  auto relax_chunk = [&](bool act, uint64_t my_ks, uint32_t my_b, uint32_t my_e) {
    if (profile && act) {
      if (profile == 1u) p_states += 1;  // (profile == 2: the states column counts atomicMin attempts instead)
      p_arcs += my_e - my_b;
    }
    uint64_t mask = __ballot(act);
    while (mask) {
      // each of the wave's 4 groups takes TWO states per round (the 8 lowest set bits): two independent
      // load -> pre-check -> atomic chains per lane are in flight at once (the kernel is latency bound)
      const uint64_t m1 = mask & (mask - 1), m2 = m1 & (m1 - 1), m3 = m2 & (m2 - 1);
      const uint64_t m4 = m3 & (m3 - 1), m5 = m4 & (m4 - 1), m6 = m5 & (m5 - 1), m7 = m6 & (m6 - 1);
      const uint64_t mine_a = grp == 0 ? mask : grp == 1 ? m1 : grp == 2 ? m2 : m3;
      const uint64_t mine_b = grp == 0 ? m4 : grp == 1 ? m5 : grp == 2 ? m6 : m7;
      mask = m7 & (m7 - 1);
      const bool has_a = mine_a != 0, has_b = mine_b != 0;
      const int la = has_a ? __ffsll((unsigned long long)mine_a) - 1 : 0;
      const int lb = has_b ? __ffsll((unsigned long long)mine_b) - 1 : 0;
      const uint64_t ks_a = __shfl(my_ks, la), ks_b = __shfl(my_ks, lb);
      uint32_t ia = __shfl(my_b, la) + sub, ib = __shfl(my_b, lb) + sub;
      // (shuffles stay outside any lane-dependent condition: a bpermute reads 0 from a lane that is masked off)
      const uint32_t ea_all = __shfl(my_e, la), eb_all = __shfl(my_e, lb);
      const uint32_t ea = has_a ? ea_all : 0u, eb = has_b ? eb_all : 0u;
      const float da = key_f32((uint32_t)(ks_a >> 32)), db = key_f32((uint32_t)(ks_b >> 32));
      const uint32_t ha = (uint32_t)ks_a + 1u, hb = (uint32_t)ks_b + 1u;
      while (__any(ia < ea || ib < eb)) {
        const bool va = ia < ea, vb = ib < eb;
        uint2 aa = make_uint2(0x7F800000u, 0u), ab = make_uint2(0x7F800000u, 0u);  // {+inf, state 0}: never relaxes
        if (va) aa = wn[ia];
        if (vb) ab = wn[ib];
        const float ca = (da + __uint_as_float(aa.x)) + 0.0f;  // w1 (x) w2 = f32 add (tropical_weight.rs:60-70)
        const float cb = (db + __uint_as_float(ab.x)) + 0.0f;
        const bool fa = va && ca < INF, fb = vb && cb < INF;  // +inf never improves (shortest_path.rs:226)
        const uint64_t cka = ((uint64_t)f32_key(ca) << 32) | ha, ckb = ((uint64_t)f32_key(cb) << 32) | hb;
        // Plain pre-check against a 4-byte SHADOW of the distance half of the key (4 MB for 1M states: half the bytes
        // per gather and a far better L2 hit rate than the 8-byte keys).  shadow[t] is only ever written with values
        // that an atomicMin has installed in key[t], and keys only decrease, so shadow[t] >= enc(d[t]) at all times:
        // a candidate above it cannot improve; a stale (too high) shadow only costs an extra atomic; on equal
        // distance the hop half decides and the real key is read.
        const uint32_t eca = (uint32_t)(cka >> 32), ecb = (uint32_t)(ckb >> 32);
        uint32_t sa = 0, sb = 0;
        if (fa) sa = shadow[aa.y];
        if (fb) sb = shadow[ab.y];
        bool ta = fa && eca <= sa, tb = fb && ecb <= sb;
        if (ta && eca == sa) ta = cka < key[aa.y];
        if (tb && ecb == sb) tb = ckb < key[ab.y];
        uint64_t olda = 0, oldb = 0;
        if (ta) olda = atomicMin((unsigned long long*)&key[aa.y], (unsigned long long)cka);
        if (tb) oldb = atomicMin((unsigned long long*)&key[ab.y], (unsigned long long)ckb);
        if (profile == 2u) p_states += (ta ? 1u : 0u) + (tb ? 1u : 0u);
        activate(ta && cka < olda, aa.y, eca, ca);
        activate(tb && ckb < oldb, ab.y, ecb, cb);
        ia += GROUP;
        ib += GROUP;
      }
    }
  };

  for (uint32_t base = wave * 64u; base < n; base += n_waves * 64u) {
    const uint32_t sc = base + lane;
    bool act = sc < n && flags_cur[sc] != 0;
    if (__ballot(act) == 0) continue;
    // the lane that owns an active state fetches everything the relaxation of that state needs: ONE memory
    // round trip for the whole 64-state chunk; the groups get it by shuffle
    uint64_t my_ks = 0;
    uint32_t my_b = 0, my_e = 0;
    if (act) {
      flags_cur[sc] = 0;  // this buffer is the NEXT frontier two sweeps from now
      my_ks = key[sc];
      my_b = offsets[sc];
      my_e = offsets[sc + 1];
      if (key_f32((uint32_t)(my_ks >> 32)) > tau) {  // far: stays in the frontier, is not relaxed in this sweep
        flags_next[sc] = 1;
        any = true;
        act = false;
        far_cnt += 1u;
      }
    }
    own_states += (uint32_t)__popcll(__ballot(act));
    relax_chunk(act, my_ks, my_b, my_e);
  }
  // a wave that had a real share of a big frontier (the band was widened) leaves its discoveries to the next sweep
  if (own_states > CHASE_OWN_MAX) chase_rounds = 0;
  // the wave's own discoveries (wave-synchronous: the list is private to the wave, LDS accesses of one wave are ordered)
  for (uint32_t chased = 0; c_tail != c_head;) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const uint32_t take = min(64u, c_tail - c_head);
    uint2 e = make_uint2(0u, 0u);
    if (lane < take) e = chase[(c_head + lane) % CHASE_MAX];
    c_head += take;
    if (chased >= chase_rounds) {  // budget spent: what is left goes to the next sweep
      if (lane < take) {
        flags_next[e.x] = 1;
        any = true;
        near_cnt += 1;
      }
      continue;
    }
    chased += take;
    bool act = lane < take;
    uint64_t my_ks = 0;
    uint32_t my_b = 0, my_e = 0;
    if (act) {
      my_ks = key[e.x];
      my_b = offsets[e.x];
      my_e = offsets[e.x + 1];
      act = (uint32_t)(my_ks >> 32) == e.y;  // improved again since: whoever did that listed or flagged it
    }
    relax_chunk(act, my_ks, my_b, my_e);
  }
  // one conditional plain store + one sharded atomicAdd per workgroup (thousands of same-address atomics per
  // sweep would serialise at ~12 ns each)
  for (int d = 32; d >= 1; d >>= 1) near_cnt += __shfl_xor(near_cnt, d);
  if (bin_on)
    for (int d = 32; d >= 1; d >>= 1) far_cnt += __shfl_xor(far_cnt, d);
  const bool wave_any = __any(any);
  if (lane == 0) {
    if (wave_any) s_any = 1u;
    if (near_cnt) atomicAdd(&s_near, near_cnt);
    if (bin_on && far_cnt) atomicAdd(&s_far, far_cnt);
  }
  if (profile) {
    for (int d = 32; d >= 1; d >>= 1) {
      p_arcs += __shfl_xor(p_arcs, d);
      p_states += __shfl_xor(p_states, d);
    }
    if (lane == 0 && (p_states | p_arcs)) {
      atomicAdd(&s_prof[0], p_arcs);
      atomicAdd(&s_prof[1], p_states);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_any && *improved == 0u) *improved = 1u;
    if (s_near) atomicAdd(&ctl->near[sweep % NEAR_RING][(blockIdx.x % NEAR_SHARDS) * NEAR_STRIDE], s_near);
    if (s_far) atomicAdd(&ctl->far[sweep % NEAR_RING][(blockIdx.x % NEAR_SHARDS) * NEAR_STRIDE], s_far);
    if (profile && (s_prof[0] | s_prof[1])) {
      atomicAdd(&ctl->arcs[(blockIdx.x % PROF_SHARDS) * PROF_STRIDE], s_prof[0]);
      atomicAdd(&ctl->states[(blockIdx.x % PROF_SHARDS) * PROF_STRIDE], s_prof[1]);
    }
  }
}

// profiling helper: keeps the GPU busy right before the event that opens a timed sweep, as the previous sweep does in an
// un-profiled solve (a launch into an idle GPU takes ~3 us longer)
__global__ void sssp_nop_kernel(const uint8_t* __restrict__ flags, uint32_t n, uint32_t* sink) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && flags[i] == 0xFF) *sink = i;  // flags are 0 / 1: never true
}

// closes a batch: the next replay continues at base + count, and the flag slots half a ring ahead are recycled
// and the batch's flags are mirrored into pinned host memory (plain stores over the bus: cheaper than a copy node)
__global__ void sssp_advance_kernel(Ctl* ctl, uint32_t* improved_ring, uint32_t count, uint32_t* host_ring) {
  const uint32_t base = ctl->base;
  for (uint32_t i = threadIdx.x; i < count; i += blockDim.x) {
    if (host_ring) host_ring[(base + i) % IMP_RING] = improved_ring[(base + i) % IMP_RING];
    improved_ring[(base + IMP_RING / 2 + i) % IMP_RING] = 0;
  }
  __syncthreads();
  if (threadIdx.x == 0) ctl->base = base + count;
}

// f_parent = argmin over final states of (d[s] (x) rho(s), s)      (shortest_path.rs:214-220)
__global__ void __launch_bounds__(256) sssp_final_kernel(const float* __restrict__ finals, const uint64_t* __restrict__ key,
                                                        uint32_t n, Ctl* __restrict__ ctl) {
  __shared__ unsigned long long s_best[4];
  unsigned long long best = KEY_INF;
  for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += gridDim.x * blockDim.x) {
    const float f = finals[s];
    if (!(f < INF)) continue;  // most states are not final: their key is never fetched
    const uint64_t k = key[s];
    if (k == KEY_INF) continue;
    const float tot = (key_f32((uint32_t)(k >> 32)) + f) + 0.0f;
    if (!(tot < INF)) continue;
    const unsigned long long c = ((unsigned long long)f32_key(tot) << 32) | s;
    best = c < best ? c : best;
  }
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long o = __shfl_xor(best, d);
    best = o < best ? o : best;
  }
  if ((threadIdx.x & 63) == 0) s_best[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) best = s_best[w] < best ? s_best[w] : best;
    // one atomic per workgroup at most, and only if it can still lower the result (same-address atomics cost ~12 ns each)
    if (best != KEY_INF && best < __hip_atomic_load(&ctl->best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      atomicMin(&ctl->best, best);
  }
}

// Predecessor rule.  Class 0: the arc is tight in both halves of the key, (d[s] (x) w, hops[s] + 1) ==
// (d[t], hops[t]) — on weights whose f32 sums are exact every reached state but the start has such an arc.  Class 1, the
// fallback: the arc is tight in the distance and the source's key is lexicographically below the target's.  With
// inexact sums a state can keep a hop count it got from a label of its predecessor that was later improved in the
// distance (two different distances of the source can round to the same sum): then no arc is tight in the hop count,
// but the arc that produced the label is still tight in the distance and, for non-negative weights, its source's key is
// smaller, so a class-1 arc exists.  Keys strictly decrease along either class: the predecessor graph is acyclic.
constexpr unsigned long long PARENT_NONE = ~0ull;
__device__ __forceinline__ unsigned long long parent_class(uint64_t cand_key, uint64_t key_s, uint64_t key_t) {
  if (cand_key == key_t) return 0ull;
  if ((cand_key >> 32) == (key_t >> 32) && key_s < key_t) return 1ull << 63;
  return PARENT_NONE;
}

// parent[t] = min (class, s, pos) over the arcs parent_class admits
__global__ void __launch_bounds__(256) sssp_parent_kernel(const uint32_t* __restrict__ offsets,
                                                          const uint2* __restrict__ wn,
                                                          const uint64_t* __restrict__ key,
                                                          unsigned long long* __restrict__ parent, uint32_t n) {
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lane = tid % GROUP;
  const uint32_t n_groups = gridDim.x * blockDim.x / GROUP;
  for (uint32_t s = tid / GROUP; s < n; s += n_groups) {
    const uint64_t ks = key[s];
    if (ks == KEY_INF) continue;
    const float d = key_f32((uint32_t)(ks >> 32));
    const uint32_t h1 = (uint32_t)ks + 1u;
    const uint32_t b = offsets[s], e = offsets[s + 1];
    for (uint32_t i = b + lane; i < e; i += GROUP) {
      const uint2 a = wn[i];
      const float c = (d + __uint_as_float(a.x)) + 0.0f;
      if (!(c < INF)) continue;
      const uint64_t ck = ((uint64_t)f32_key(c) << 32) | h1, kt = key[a.y];
      const unsigned long long cls = parent_class(ck, ks, kt);
      if (cls != PARENT_NONE) atomicMin(&parent[a.y], cls | ((unsigned long long)s << 32) | (i - b));
    }
  }
}

__global__ void sssp_header_kernel(const float* __restrict__ finals, const uint64_t* __restrict__ key, Ctl* ctl) {
  const unsigned long long best = ctl->best;
  if (best == KEY_INF) {
    ctl->has_path = 0;
    ctl->hops = 0;
    return;
  }
  const uint32_t fp = (uint32_t)best;
  ctl->has_path = 1;
  ctl->f_parent = fp;
  ctl->hops = (uint32_t)key[fp];
  ctl->final_weight = finals[fp];
  ctl->total = key_f32((uint32_t)(best >> 32));
}

// single_shortest_path_backtrace (shortest_path.rs:241-282): walk parent[] from f_parent; the arc of the
// k-th created state (k >= 1) is ifst.trs(parent state)[pos] re-targeted to state k-1.
__global__ void sssp_backtrace_kernel(const uint32_t* __restrict__ offsets, const wfst_tr* __restrict__ arcs,
                                      const uint64_t* __restrict__ key, const unsigned long long* __restrict__ parent,
                                      Ctl* __restrict__ ctl, wfst_tr* __restrict__ out, uint32_t out_cap) {
  if (threadIdx.x || blockIdx.x) return;
  uint32_t cur = ctl->f_parent, k = 0;
  // the walk ends at the start state, the only one whose key has no arcs in it (with class-1 predecessors its length
  // need not be the hop count of the final state's key)
  while ((uint32_t)key[cur] != 0u) {
    const unsigned long long p = parent[cur];
    if (p == PARENT_NONE) {  // no admissible predecessor (inexact sums with negative weights)
      ctl->pad |= 4u;
      return;
    }
    if (k >= out_cap) {  // longer than the buffer the host sized from the hop count: it retries with room for n arcs
      ctl->pad |= 16u;
      return;
    }
    const uint32_t s = (uint32_t)(p >> 32) & 0x7FFFFFFFu, pos = (uint32_t)p;
    wfst_tr tr = arcs[offsets[s] + pos];
    tr.nextstate = k;
    out[k] = tr;
    cur = s;
    ++k;
  }
  ctl->hops = k;
}

// ---- transpose of the CSR, cached on the FST handle once it is queried again: with it the
// canonical predecessor of the ~hops states ON the path is found by looking at their in-arcs only, instead of the
// parent pass over all arcs (105 us on 10M arcs).
__global__ void __launch_bounds__(256) rev_count_kernel(const uint2* __restrict__ wn, uint64_t n_arcs, uint32_t* __restrict__ indeg) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_arcs; i += (uint64_t)gridDim.x * blockDim.x)
    atomicAdd(&indeg[wn[i].y], 1u);
}
__global__ void __launch_bounds__(256) rev_fill_kernel(const uint32_t* __restrict__ offsets, const uint2* __restrict__ wn,
                                                      uint32_t n, uint32_t* __restrict__ cursor, uint4* __restrict__ rev_arc) {
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lane = tid % GROUP;
  const uint32_t n_groups = gridDim.x * blockDim.x / GROUP;
  for (uint32_t s = tid / GROUP; s < n; s += n_groups) {
    const uint32_t b = offsets[s], e = offsets[s + 1];
    for (uint32_t i = b + lane; i < e; i += GROUP) {
      const uint2 a = wn[i];
      rev_arc[atomicAdd(&cursor[a.y], 1u)] = make_uint4(s, i - b, a.x, 0u);
    }
  }
}

// ---- the same transpose WITHOUT a global atomic, for FSTs that have a mailbox plan (sssp_mailbox.h): region (i -> j) of the
// plan holds one slot per arc from block i to block j, destination-major — so the regions of destination block j, taken
// together, ARE the in-arcs of block j's states, already contiguous and already at their final place in rev_arc; what is
// left is the order inside the block.  rev_bucket_kernel: workgroup i writes a record {source, position, weight, target mod B}
// per arc of block i into its slot (one LDS atomicAdd on the region's cursor; the records of a region fill its lines front to
// back); rev_place_kernel: workgroup j counts its records per target state in LDS, scans, writes rev_off, and moves every
// record to its target's run.  10 M arcs: ~0.2 ms against ~1.2 ms for the two atomic passes above.
template <uint32_t LOG>
__global__ void __launch_bounds__(1024) rev_bucket_kernel(const uint32_t* __restrict__ offsets, const uint2* __restrict__ wn, uint32_t n,
                                                          uint32_t nb, const uint32_t* __restrict__ roff_t, uint4* __restrict__ rec) {
  constexpr uint32_t B = 1u << LOG;
  extern __shared__ uint32_t l_cur[];  // [nb] next slot of region (i -> j)
  const uint32_t i = blockIdx.x, s0 = i << LOG, s1 = min(n, s0 + B);
  for (uint32_t j = threadIdx.x; j < nb; j += blockDim.x) l_cur[j] = roff_t[(size_t)i * nb + j];
  __syncthreads();
  // 16 lanes per state, four states of a group in flight (their row bounds, then their first 16 arcs, are requested together:
  // one workgroup per compute unit, so the loads in flight per thread are the bandwidth)
  const uint32_t sub = threadIdx.x & 15u, grp = threadIdx.x >> 4;
  constexpr uint32_t U = 4, G = 1024 / 16;
  for (uint32_t sb = s0 + grp; sb < s1; sb += U * G) {
    uint32_t b[U], e[U];
    uint2 a[U];
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
      const uint32_t s = sb + u * G;
      b[u] = s < s1 ? offsets[s] : 0u;
      e[u] = s < s1 ? offsets[s + 1] : 0u;
    }
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) a[u] = b[u] + sub < e[u] ? wn[b[u] + sub] : make_uint2(0u, 0u);
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
      const uint32_t s = sb + u * G;
      if (b[u] + sub < e[u]) {
        const uint32_t slot = atomicAdd(&l_cur[a[u].y >> LOG], 1u);
        rec[slot] = make_uint4(s, sub, a[u].x, a[u].y & (B - 1u));
      }
      for (uint32_t k = b[u] + sub + 16u; k < e[u]; k += 16u) {  // (rows beyond 16 arcs)
        const uint2 x = wn[k];
        const uint32_t slot = atomicAdd(&l_cur[x.y >> LOG], 1u);
        rec[slot] = make_uint4(s, k - b[u], x.x, x.y & (B - 1u));
      }
    }
  }
}
template <uint32_t LOG>
__global__ void __launch_bounds__(1024) rev_place_kernel(const uint32_t* __restrict__ roff, uint32_t nb, uint32_t n,
                                                         const uint4* __restrict__ rec, uint32_t* __restrict__ rev_off,
                                                         uint4* __restrict__ rev_arc) {
  constexpr uint32_t B = 1u << LOG, R = B / 1024;
  __shared__ uint32_t l_cnt[B];
  __shared__ uint32_t s_wsum[16];
  const uint32_t j = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  const uint32_t lo = roff[(size_t)j * nb], hi = roff[(size_t)(j + 1) * nb];  // all the in-arcs of block j
  for (uint32_t t = tid; t < B; t += 1024) l_cnt[t] = 0;
  __syncthreads();
  // (four records per thread in flight: one workgroup per compute unit is all the parallelism there is here)
  {
    uint32_t k = lo + tid;
    for (; k + 3u * 1024u < hi; k += 4u * 1024u) {
      const uint32_t t0 = rec[k].w, t1 = rec[k + 1024u].w, t2 = rec[k + 2048u].w, t3 = rec[k + 3072u].w;
      atomicAdd(&l_cnt[t0], 1u);
      atomicAdd(&l_cnt[t1], 1u);
      atomicAdd(&l_cnt[t2], 1u);
      atomicAdd(&l_cnt[t3], 1u);
    }
    for (; k < hi; k += 1024u) atomicAdd(&l_cnt[rec[k].w], 1u);
  }
  __syncthreads();
  // exclusive scan of the B counts: R consecutive counts per thread, a wave scan of the thread sums, the wave totals
  uint32_t c[R], mine = 0;
  for (uint32_t r = 0; r < R; ++r) {
    c[r] = l_cnt[tid * R + r];
    mine += c[r];
  }
  uint32_t x = mine;
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(x, d);
    if (lane >= (uint32_t)d) x += y;
  }
  if (lane == 63) s_wsum[wv] = x;
  __syncthreads();
  uint32_t base = 0;
  for (uint32_t w = 0; w < wv; ++w) base += s_wsum[w];
  uint32_t run = base + x - mine;
  const uint32_t s0 = j << LOG;
  for (uint32_t r = 0; r < R; ++r) {
    const uint32_t tl = tid * R + r;
    l_cnt[tl] = run;  // from here on: the next free position of the target's run
    if (s0 + tl < n) rev_off[s0 + tl] = lo + run;
    run += c[r];
  }
  if (j == gridDim.x - 1 && tid == 0) rev_off[n] = hi;
  __syncthreads();
  {
    uint32_t k = lo + tid;
    for (; k + 3u * 1024u < hi; k += 4u * 1024u) {
      const uint4 r0 = rec[k], r1 = rec[k + 1024u], r2 = rec[k + 2048u], r3 = rec[k + 3072u];
      const uint32_t p0 = atomicAdd(&l_cnt[r0.w], 1u), p1 = atomicAdd(&l_cnt[r1.w], 1u);
      const uint32_t p2 = atomicAdd(&l_cnt[r2.w], 1u), p3 = atomicAdd(&l_cnt[r3.w], 1u);
      rev_arc[lo + p0] = make_uint4(r0.x, r0.y, r0.z, 0u);
      rev_arc[lo + p1] = make_uint4(r1.x, r1.y, r1.z, 0u);
      rev_arc[lo + p2] = make_uint4(r2.x, r2.y, r2.z, 0u);
      rev_arc[lo + p3] = make_uint4(r3.x, r3.y, r3.z, 0u);
    }
    for (; k < hi; k += 1024u) {
      const uint4 r = rec[k];
      rev_arc[lo + atomicAdd(&l_cnt[r.w], 1u)] = make_uint4(r.x, r.y, r.z, 0u);
    }
  }
}

// single_shortest_path_backtrace (shortest_path.rs:241-282) over the transpose, by ONE wave: at every step the lanes test
// the in-arcs of the current state for tightness, (d[s] (x) w, hops[s] + 1) == (d[t], hops[t]), and the smallest
// (class, s, pos) wins — the same predecessor sssp_parent_kernel selects.  A step is TWO dependent trips: the in-arc
// entries (source, position, weight: nothing else of the arc is needed), then the sources' keys together with their own
// in-arc ranges (the winner's is the next step's).  The arcs of the walk themselves are fetched afterwards, all at once
// (their (state, position) wait in LDS), and go straight to `out` (pinned host memory when the path fits in it).
// Returns the number of steps taken; pad |= 4: no admissible predecessor, pad |= 8: longer than out_cap.
constexpr uint32_t WALK_LDS = 1024;
__device__ __forceinline__ uint32_t sssp_walk_back(const uint32_t* __restrict__ offsets, const wfst_tr* __restrict__ arcs,
                                                   const uint64_t* __restrict__ key, const uint32_t* __restrict__ rev_off,
                                                   const uint4* __restrict__ rev_arc, uint32_t fp, wfst_tr* __restrict__ out,
                                                   uint32_t out_cap, uint32_t& pad, uint2* s_walk /* LDS [WALK_LDS] */, uint32_t& ties) {
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t k = 0;
  uint64_t kt = key[fp];
  uint32_t rb = rev_off[fp], re = rev_off[fp + 1];
  // `ties`: states on the walk with more than one in-arc that is tight in the DISTANCE (d[s] (x) w == d[t]: any of them
  // continues an optimal path, whatever rule picks one) — the start state: with any (a zero-weight cycle through it)
  for (;;) {
    if ((uint32_t)kt == 0u) {  // the start state
      uint32_t tn = 0;
      for (uint32_t j = rb + lane; j < re; j += 64) {
        const uint4 ra = rev_arc[j];
        const uint64_t ks = key[ra.x];
        if (ks == KEY_INF) continue;
        const float c = (key_f32((uint32_t)(ks >> 32)) + __uint_as_float(ra.z)) + 0.0f;
        if (c < INF && f32_key(c) == (uint32_t)(kt >> 32)) tn += 1u;
      }
      if (__any(tn != 0u)) ties += 1u;
      break;
    }
    if (k >= out_cap) {
      pad |= 8u;
      break;
    }
    unsigned long long bp = PARENT_NONE;
    uint64_t my_ks = 0;
    uint32_t my_rb = 0, my_re = 0;
    uint32_t tn = 0;
    for (uint32_t j = rb + lane; j < re; j += 64) {
      const uint4 ra = rev_arc[j];
      const uint64_t ks = key[ra.x];
      const uint32_t sb = rev_off[ra.x], se = rev_off[ra.x + 1];
      if (ks == KEY_INF) continue;
      const float c = (key_f32((uint32_t)(ks >> 32)) + __uint_as_float(ra.z)) + 0.0f;
      if (!(c < INF)) continue;
      if (f32_key(c) == (uint32_t)(kt >> 32)) tn += 1u;
      const uint64_t ck = ((uint64_t)f32_key(c) << 32) | ((uint32_t)ks + 1u);
      const unsigned long long cls = parent_class(ck, ks, kt);
      if (cls != PARENT_NONE) {
        const unsigned long long cand = cls | ((unsigned long long)ra.x << 32) | ra.y;
        if (cand < bp) {
          bp = cand;
          my_ks = ks;
          my_rb = sb;
          my_re = se;
        }
      }
    }
    unsigned long long best = bp;
    for (int d = 32; d >= 1; d >>= 1) {
      const unsigned long long o = __shfl_xor(best, d);
      best = o < best ? o : best;
    }
    if (best == PARENT_NONE) {  // no admissible predecessor: reported, not followed
      pad |= 4u;
      break;
    }
    {
      const unsigned long long tm = __ballot(tn != 0u);
      if (__popcll(tm) > 1 || __any(tn > 1u)) ties += 1u;
    }
    const int wl = __ffsll((unsigned long long)__ballot(bp == best)) - 1;  // (source, position) is unique: one lane holds it
    kt = __shfl(my_ks, wl);
    rb = __shfl(my_rb, wl);
    re = __shfl(my_re, wl);
    const uint32_t s = (uint32_t)(best >> 32) & 0x7FFFFFFFu, pos = (uint32_t)best;
    if (lane == 0) {
      if (k < WALK_LDS) {
        s_walk[k] = make_uint2(s, pos);
      } else {  // (a path longer than the list: its arcs are fetched on the way, one dependent trip more per step)
        wfst_tr tr = arcs[offsets[s] + pos];
        tr.nextstate = k;
        out[k] = tr;
      }
    }
    ++k;
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // lane 0's list is in LDS before the wave reads it back
  for (uint32_t i = lane; i < min(k, WALK_LDS); i += 64) {
    const uint2 e = s_walk[i];
    wfst_tr tr = arcs[offsets[e.x] + e.y];
    tr.nextstate = i;
    out[i] = tr;
  }
  return k;
}

__global__ void __launch_bounds__(64) sssp_backtrace_rev_kernel(const uint32_t* __restrict__ offsets,
                                                               const wfst_tr* __restrict__ arcs, const uint64_t* __restrict__ key,
                                                               const uint32_t* __restrict__ rev_off,
                                                               const uint4* __restrict__ rev_arc, Ctl* __restrict__ ctl,
                                                               wfst_tr* __restrict__ out, uint32_t out_cap) {
  __shared__ uint2 s_walk[WALK_LDS];
  const uint32_t lane = threadIdx.x;
  if (!ctl->has_path) return;
  if (ctl->hops > out_cap) {  // the host falls back to the parent pass
    if (lane == 0) ctl->pad |= 8u;
    return;
  }
  uint32_t pad = 0, ties = 0;
  const uint32_t k = sssp_walk_back(offsets, arcs, key, rev_off, rev_arc, ctl->f_parent, out, out_cap, pad, s_walk, ties);
  if (lane == 0) {
    if (pad) ctl->pad |= pad;
    else ctl->hops = k;  // the real length of the walk
  }
}

// ---- the search over the handle's list and the walk (the merge helpers are in front of sssp_mailbox.h)
// the handle's list of its final states {state, final weight}: entries first, first + stride, ... — four in flight (two
// dependent trips per four entries; the order of the merges does not matter).  (Sixteen in flight in the early tail's ONE
// workgroup were no faster: 14 000 gathered keys are ~6 us of one compute unit's L1 however they are asked for.)
__device__ __forceinline__ void tail_search_list(const uint64_t* __restrict__ key, const uint2* __restrict__ fin_list, uint32_t n_fin,
                                                 uint32_t first, uint32_t stride, unsigned long long& best, bool& tie) {
  constexpr uint32_t U = 4;
  for (uint32_t i = first; i < n_fin; i += U * stride) {
    uint2 e[U];
    uint64_t k[U];
    for (uint32_t u = 0; u < U; ++u) {
      e[u] = make_uint2(0u, 0u);
      if (i + u * stride < n_fin) e[u] = fin_list[i + u * stride];
    }
    for (uint32_t u = 0; u < U; ++u) {
      k[u] = KEY_INF;
      if (i + u * stride < n_fin) k[u] = key[e[u].x];
    }
    for (uint32_t u = 0; u < U; ++u) tail_candidate(k[u], e[u].x, __uint_as_float(e[u].y), best, tie);
  }
}
// One wave, `best` / `tie` / `pad` uniform: the header of the result and the path's arcs go to pinned host memory (every
// TailOut field except `done` and `early`), and to the control block where `ctl` is given.  Returns pad with the walk's flags.
__device__ __forceinline__ uint32_t tail_walk_publish(unsigned long long best, bool tie, uint32_t pad, const float* __restrict__ finals,
                                                      const uint64_t* __restrict__ key, const uint32_t* __restrict__ offsets,
                                                      const wfst_tr* __restrict__ arcs, const uint32_t* __restrict__ rev_off,
                                                      const uint4* __restrict__ rev_arc, wfst_tr* __restrict__ out, uint32_t out_cap,
                                                      TailOut* __restrict__ hout, Ctl* __restrict__ ctl, uint2* s_walk) {
  const uint32_t lane = threadIdx.x & 63u;
  if (best == KEY_INF) {
    if (lane == 0) {
      if (ctl) {
        ctl->has_path = 0;
        ctl->hops = 0;
      }
      hout->has_path = 0u;
      hout->hops = 0u;
      hout->pad = pad;
      hout->f_parent = 0u;
      hout->final_weight = INF;
      hout->total = INF;
      hout->ties = 0u;
    }
    return pad;
  }
  const uint32_t fp = (uint32_t)best;
  const float final_weight = finals[fp], total = key_f32((uint32_t)(best >> 32));
  uint32_t k = 0, ties = tie ? 1u : 0u;
  if ((uint32_t)key[fp] > out_cap) pad |= 8u;  // the host falls back to the parent pass
  else k = sssp_walk_back(offsets, arcs, key, rev_off, rev_arc, fp, out, out_cap, pad, s_walk, ties);
  if (lane == 0) {
    const uint32_t hops = (pad & 12u) ? (uint32_t)key[fp] : k;
    if (ctl) {
      ctl->has_path = 1;
      ctl->f_parent = fp;
      ctl->hops = hops;
      ctl->final_weight = final_weight;
      ctl->total = total;
    }
    // (the walk's own flags go to the host only: a tail that ran ahead of the last sweeps is run again on this block)
    hout->has_path = 1u;
    hout->hops = hops;
    hout->pad = pad;
    hout->f_parent = fp;
    hout->final_weight = final_weight;
    hout->total = total;
    hout->ties = ties;
  }
  return pad;
}

// The early tail: the extra workgroup of a NARROW launch behind a hand-over (sssp_mbox_kernel, blockIdx.x == nb) does the
// tail's search (or, behind a resident launch, the merge of the blocks' best final states that launch left: `merged`) and the
// walk on keys that other workgroups of the SAME launch are still lowering, with plain loads, and leaves
// {launch, best | TIE_BIT} in the control block; sssp_tail_kernel certifies the result or computes it again.  `lds`: 16 words
// for the waves' results, WALK_LDS entries of the walk behind them.  Nothing the ordinary tail uses is touched.
__device__ __forceinline__ void sssp_early_tail(const EarlyTail& et, const uint32_t* __restrict__ offsets, const uint64_t* __restrict__ key,
                                                Ctl* __restrict__ ctl, uint32_t prev_flag, uint32_t sweep, unsigned long long* lds,
                                                bool merged, unsigned long long best, bool tie) {
  // (a launch queued behind the solve's last one: the fixed point was reached, or the solve gave up — as sssp_mbox_resident_kernel)
  const uint32_t pf = prev_flag;
  if (pf == 0u || pf == FLAG_NARROW_CLEAN || pf == FLAG_RES_ABORT) return;
  unsigned long long* const s_best = lds;
  uint2* const s_walk = (uint2*)(lds + 16);
  const uint32_t lane = threadIdx.x & 63u, waves = blockDim.x >> 6;
  // `merged` (uniform): the resident launch in front of this one left every block's best final state (MboxView::blk_best) and
  // best / tie hold this thread's share of those words — the keys as they stood before this launch wrote anything.  Otherwise
  // the list is searched, on keys this launch is lowering.  Either way sssp_tail_kernel's certificate decides.
  if (!merged) tail_search_list(key, et.fin_list, et.n_fin, threadIdx.x, blockDim.x, best, tie);
  tail_wave_reduce(best, tie);
  if (lane == 0) s_best[threadIdx.x >> 6] = tail_pack(best, tie);
  __syncthreads();
  if (threadIdx.x >= 64) return;
  best = KEY_INF;
  tie = false;
  if (lane < waves) tail_merge_packed(best, tie, s_best[lane]);
  tail_wave_reduce(best, tie);
  const uint32_t pad = tail_walk_publish(best, tie, 0u, et.finals, key, offsets, et.arcs, et.rev_off, et.rev_arc, et.out, et.out_cap,
                                         et.hout, nullptr, s_walk);
  if (lane == 0) et.hout->early_src = merged ? EARLY_SRC_BLOCKS : EARLY_SRC_LIST;
  host_stores_done();
  // (a walk that did not end at the start state, or a path beyond the pinned buffer: the ordinary tail's business)
  if (lane == 0 && !(pad & 12u)) {
    ctl->early_best = tail_pack(best, tie);
    ctl->early_sweep = sweep;
  }
}

// The tail of a repeated query in ONE launch: arg-min over the final states (sssp_final_kernel), the header
// (sssp_header_kernel) and the walk over the transpose (sssp_backtrace_rev_kernel), with the result header written into
// pinned host memory next to the path arcs.  Every workgroup leaves the best final state of its share; the workgroup
// that draws the last ticket reduces them and walks back.  (Three launches, a 1-thread kernel and a copy of the whole
// control block cost ~30 us at the end of every solve; 1024 workgroups each polling and lowering ONE word were most of
// the final-state search: same-address atomics serialise at ~12 ns.)
//
// `early_check`: the batch in front of this launch may have run the early tail (sssp_early_tail).  Let k be the launch it
// ran in and B the best total it found.  Its result — header and path, already in host memory — stands if and only if
// launch k's flag is FLAG_NARROW_CLEAN (the fixed point was reached in that launch: a launch that leaves anything waiting
// is not CLEAN) and narrow_low[k] > enc(B), strictly: every key lowered while the early tail was reading went to a value
// above B, from a value that was higher still.  Arc and final weights are >= 0 where the early tail runs, so
//   * a predecessor s of a state t on the path needs enc(d[s] + w) == enc(d[t]) <= enc(B) in either predecessor class; with
//     w >= 0 a source above B is never admissible, whether the walk read its key before or after it changed;
//   * a final state whose key changed has a total >= its key, above B before and after: neither the optimum nor a tie;
//   * a write AT B could make a tie (a second final state, a second tight in-arc), hence the strict inequality.
// Every key at or below B is one no writer of launch k touched: the early tail read what this kernel would read.
// Where the early tail took B from the blocks' best final states (mbox_blk_best: left by the resident launch k - 1 on its
// hand-over) instead of searching the list, those words are the keys as they stood BEFORE launch k wrote anything — the
// limiting case of "read while launch k was writing" — and the same two conditions cover it: a final state whose key launch k
// lowered ended above B from a value higher still, so it was neither the optimum nor a tie in the words, and is neither now.
//
// Behind a BOUNDED head (FLAG_NARROW_BOUNDED in launch 0: sssp_mailbox.h, above mbox_narrow) the same two lines let this
// kernel run its ordinary, uncertified search and walk on keys that are the fixed point only at and below the head's B: a final
// state with an unsettled key has a key — hence a total — above B, so it is neither the optimum nor a tie; a predecessor with
// an unsettled key is not admissible.  advance() treats the flag as "solve over" and the re-arm verdict is `finished`.
__global__ void __launch_bounds__(1024) sssp_tail_kernel(const float* __restrict__ finals, const uint64_t* __restrict__ key,
                                                         uint32_t n, const uint2* __restrict__ fin_list, uint32_t n_fin,
                                                         Ctl* __restrict__ ctl,
                                                         const uint32_t* __restrict__ offsets, const wfst_tr* __restrict__ arcs,
                                                         const uint32_t* __restrict__ rev_off,
                                                         const uint4* __restrict__ rev_arc, wfst_tr* __restrict__ out,
                                                         uint32_t out_cap, TailOut* __restrict__ hout,
                                                         uint32_t* __restrict__ improved_ring, uint32_t adv_count,
                                                         uint32_t* __restrict__ host_ring, uint32_t done_ticket, uint32_t early_check,
                                                         uint32_t rearm_on) {
  __shared__ unsigned long long s_best[16];
  __shared__ uint2 s_walk[WALK_LDS];
  __shared__ uint32_t s_last;
  const uint32_t lane = threadIdx.x & 63u;
  // closes the sweep batch queued in front of this launch (what sssp_advance_kernel does: the flags of its sweeps go to
  // pinned host memory, the slots half a ring ahead are recycled, the base moves on) — one launch and one flush of
  // host-memory writes less at the end of a predicted solve.  By the wave that writes the ticket at the end: ONE
  // system-scope fence orders all of it.
  // Returns (uniform) what SweepDriver::scan_flags will make of the flags on the host: the first launch of the batch whose flag
  // is 0, FLAG_NARROW_CLEAN, FLAG_NARROW_BOUNDED or FLAG_RES_ABORT exists and did not abort — the solve is over and nothing will
  // be queued behind it.
  auto advance = [&]() -> bool {
    const uint32_t base = ctl->base;
    bool finished = false, decided = false;
    for (uint32_t i0 = 0; i0 < adv_count; i0 += 64) {
      const uint32_t i = i0 + lane;
      uint32_t v = 1u;
      if (i < adv_count) {
        v = improved_ring[(base + i) % IMP_RING];
        host_ring[(base + i) % IMP_RING] = v;
        improved_ring[(base + IMP_RING / 2 + i) % IMP_RING] = 0;
      }
      const unsigned long long stop = __ballot(v == 0u || v == FLAG_NARROW_CLEAN || v == FLAG_RES_ABORT || v == FLAG_NARROW_BOUNDED);
      if (stop != 0ull && !decided) {
        decided = true;
        finished = ((__ballot(v == FLAG_RES_ABORT) >> (__ffsll((long long)stop) - 1)) & 1ull) == 0ull;
      }
    }
    if (lane == 0) ctl->base = base + adv_count;  // (every lane of the wave has read the old value above)
    return finished;
  };
  // The verdict for the re-arm launch behind this one, and for the host that parks the scratch: the solve is over AND the host
  // will not come back for the keys (a path beyond the pinned buffer, pad & 8, sends it into the parent pass over them).
  // In front of the ticket.
  auto verdict = [&](bool finished, uint32_t pad) {
    const uint32_t v = rearm_on && finished && !(pad & 8u) ? 1u : 0u;
    if (rearm_on) ctl->rearm = v;
    hout->rearmed = v;
    hout->bounded_why = ctl->bounded_why;
  };
  uint32_t early = EARLY_UNCHECKED;
  if (early_check) {  // (uniform reads: the early tail's launch, then that launch's flag and its least write)
    const uint32_t k = ctl->early_sweep;
    early = EARLY_ABSENT;
    if (k != 0u && k < adv_count && improved_ring[k % IMP_RING] == FLAG_NARROW_CLEAN) {
      const unsigned long long eb = ctl->early_best;
      early = ctl->narrow_low[k % RING] > (uint32_t)(eb >> 32) ? EARLY_USED : EARLY_REFUTED;
    }
    if (early == EARLY_USED) {
      if (blockIdx.x != 0 || threadIdx.x >= 64) return;
      const bool finished = adv_count ? advance() : false;
      if (lane == 0) {
        const uint32_t pad = ctl->pad;
        hout->pad = pad;  // (the walk's flags were clear; a relaxation may have raised the hop-count flag since)
        hout->early = EARLY_USED;
        verdict(finished, pad);
      }
      host_stores_done();
      if (lane == 0) __hip_atomic_store(&hout->done, done_ticket, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      return;
    }
  }
  unsigned long long best = KEY_INF;
  bool tie = false;
  if (fin_list) {  // the handle's list of its final states: the same candidates, found without the scan
    tail_search_list(key, fin_list, n_fin, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x, best, tie);
  } else {
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += gridDim.x * blockDim.x) {
      const float f = finals[s];
      if (f < INF) tail_candidate(key[s], s, f, best, tie);  // most states are not final: their key is never fetched
    }
  }
  tail_wave_reduce(best, tie);
  if (lane == 0) s_best[threadIdx.x >> 6] = tail_pack(best, tie);
  __syncthreads();
  if (threadIdx.x == 0) {
    best = KEY_INF;
    tie = false;
    for (uint32_t w = 0; w < (blockDim.x >> 6); ++w) tail_merge_packed(best, tie, s_best[w]);
    const unsigned long long mine = tail_pack(best, tie);
    if (gridDim.x == 1) {  // the only workgroup is the last one: nothing to hand over, nothing to draw
      s_best[0] = mine;
      s_last = 1u;
    } else {
      __hip_atomic_store(&ctl->tail_best[blockIdx.x], mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __threadfence();
      s_last = atomicAdd(&ctl->tail_ticket, 1u) == gridDim.x - 1 ? 1u : 0u;
    }
  }
  __syncthreads();
  if (!s_last || threadIdx.x >= 64) return;
  const bool finished = adv_count ? advance() : false;
  // the last workgroup's first wave: every other workgroup's result is in memory
  best = KEY_INF;
  tie = false;
  for (uint32_t b = lane; b < gridDim.x; b += 64)
    tail_merge_packed(best, tie, gridDim.x == 1 ? s_best[0] : __hip_atomic_load(&ctl->tail_best[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  tail_wave_reduce(best, tie);
  const uint32_t pad = ctl->pad;
  if (lane == 0) {
    ctl->tail_ticket = 0;  // the tail may run again on the same control block (a solve that outran its prediction)
    ctl->best = best;
    hout->early = early;
  }
  const uint32_t pad_out = tail_walk_publish(best, tie, pad, finals, key, offsets, arcs, rev_off, rev_arc, out, out_cap, hout, ctl, s_walk);
  if (lane == 0) verdict(finished, pad_out);
  // (the walk's arcs were written by several lanes of this wave)
  host_stores_done();
  if (lane == 0) __hip_atomic_store(&hout->done, done_ticket, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

#include "sssp_solo.h"

// ---- the reference's tie order on acyclic inputs (wfst_ctx_set_tie_order; include/wfst.h).  rank[s] = position of s in
// the topological order of the reference's depth-first visit (host), r2s = its inverse.
// f_parent: the FIRST state in that order whose d[s] (x) rho(s) attains the minimum (shortest_path.rs:214-220: only a
// strict improvement replaces f_parent, and states are dequeued in that order)
__global__ void __launch_bounds__(256) sssp_final_ref_kernel(const float* __restrict__ finals, const uint64_t* __restrict__ key,
                                                            const uint32_t* __restrict__ rank, uint32_t n, Ctl* __restrict__ ctl) {
  unsigned long long best = KEY_INF;
  for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += gridDim.x * blockDim.x) {
    const float f = finals[s];
    if (!(f < INF)) continue;
    const uint64_t k = key[s];
    if (k == KEY_INF) continue;
    const float tot = (key_f32((uint32_t)(k >> 32)) + f) + 0.0f;
    if (!(tot < INF)) continue;
    const unsigned long long c = ((unsigned long long)f32_key(tot) << 32) | rank[s];
    best = c < best ? c : best;
  }
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long o = __shfl_xor(best, d);
    best = o < best ? o : best;
  }
  if ((threadIdx.x & 63) == 0 && best != KEY_INF) atomicMin(&ctl->best, best);
}
// parent[t]: the FIRST arc, in (rank of the source, arc position), whose candidate d[s] (x) w equals d[t] — every later arc
// with the same candidate is no strict improvement and leaves the parent alone (shortest_path.rs:222-232)
__global__ void __launch_bounds__(256) sssp_parent_ref_kernel(const uint32_t* __restrict__ offsets, const uint2* __restrict__ wn,
                                                             const uint64_t* __restrict__ key, const uint32_t* __restrict__ rank,
                                                             unsigned long long* __restrict__ parent, uint32_t n) {
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lane = tid % GROUP;
  const uint32_t n_groups = gridDim.x * blockDim.x / GROUP;
  for (uint32_t s = tid / GROUP; s < n; s += n_groups) {
    const uint64_t ks = key[s];
    if (ks == KEY_INF) continue;
    const float d = key_f32((uint32_t)(ks >> 32));
    const uint32_t b = offsets[s], e = offsets[s + 1];
    const unsigned long long rs = (unsigned long long)rank[s] << 32;
    for (uint32_t i = b + lane; i < e; i += GROUP) {
      const uint2 a = wn[i];
      const float c = (d + __uint_as_float(a.x)) + 0.0f;
      if (!(c < INF)) continue;
      if (f32_key(c) == (uint32_t)(key[a.y] >> 32)) atomicMin(&parent[a.y], rs | (i - b));
    }
  }
}
__global__ void sssp_backtrace_ref_kernel(const uint32_t* __restrict__ offsets, const wfst_tr* __restrict__ arcs,
                                          const float* __restrict__ finals, const unsigned long long* __restrict__ parent,
                                          const uint32_t* __restrict__ r2s, uint32_t start, Ctl* __restrict__ ctl,
                                          wfst_tr* __restrict__ out, uint32_t out_cap) {
  if (threadIdx.x || blockIdx.x) return;
  const unsigned long long best = ctl->best;
  if (best == KEY_INF) {
    ctl->has_path = 0;
    ctl->hops = 0;
    return;
  }
  uint32_t cur = r2s[(uint32_t)best], k = 0;
  ctl->has_path = 1;
  ctl->f_parent = cur;
  ctl->final_weight = finals[cur];
  ctl->total = key_f32((uint32_t)(best >> 32));
  while (cur != start) {
    const unsigned long long p = parent[cur];
    if (p == PARENT_NONE || k >= out_cap) {
      ctl->pad |= 4u;
      return;
    }
    const uint32_t s = r2s[(uint32_t)(p >> 32)], pos = (uint32_t)p;
    wfst_tr tr = arcs[offsets[s] + pos];
    tr.nextstate = k;
    out[k] = tr;
    cur = s;
    ++k;
  }
  ctl->hops = k;
}

__global__ void sssp_export_kernel(const uint64_t* __restrict__ key, float* __restrict__ dist, uint32_t* __restrict__ hops,
                                   uint32_t n) {
  uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const uint64_t k = key[s];
  dist[s] = k == KEY_INF ? INF : key_f32((uint32_t)(k >> 32));
  if (hops) hops[s] = k == KEY_INF ? 0xFFFFFFFFu : (uint32_t)k;
}

// Resident solves of a device share a lease of TWO units: a grid that waits for its own workgroups must be resident as a
// whole, so a whole-device grid (one workgroup on ~245 of 256 compute units) takes both units, and a half-device grid
// (wfst_ctx_set_resident_share(ctx, 1): at most 128 workgroups) takes one — two of those fit the device together, and two
// contexts that answer queries on half the device each run their solves side by side (tools/two_queries.py).  Inside a
// process the lease is a counter per device; between processes it is an advisory lock on a file per device, held by a
// process while any of its solves holds a unit (flock, non-blocking: whoever does not get it takes one launch per level
// for that solve).  Neither covers a tenant that is not this library: the wait limit of the launch does.
struct ResidentLease {
  int held_device = -1, held_units = 0;
  ResidentLease() = default;
  ResidentLease(const ResidentLease&) = delete;
  ResidentLease& operator=(const ResidentLease&) = delete;
  // One descriptor per device and process (-1: no lock file, in-process lease only).  Opened read-only (flock works on a
  // read-only descriptor, so a file another user created is still lockable), never through a symbolic link, made world-readable
  // by whoever creates it whatever the umask; reopened after a fork (a child shares its parent's open file description, and
  // flock locks belong to the description: parent and child would both "hold" it).  Without a lock file two processes can
  // both start resident grids; the launch's wait limit is what then protects them, and that is said once on stderr.
  static int device_lock_fd(int device) {
    struct Slot { std::mutex mu; int fd = -1; pid_t pid = 0; bool tried = false; };
    static Slot slots[64];
    const unsigned d = (unsigned)device & 63u;
    Slot& sl = slots[d];
    std::lock_guard<std::mutex> lk(sl.mu);
    const pid_t me = ::getpid();
    if (sl.tried && sl.pid == me) return sl.fd;
    if (sl.tried && sl.fd >= 0) ::close(sl.fd);  // (the parent's description)
    sl.tried = true;
    sl.pid = me;
    sl.fd = -1;
    if (std::getenv("WFST_SSSP_NO_LOCKFILE")) return -1;
    const char* dir = std::getenv("WFST_LOCK_DIR");
    char path[512];
    std::snprintf(path, sizeof(path), "%s/.wfst_amd_resident_gpu%u.lock", dir ? dir : "/tmp", d);
    int fd = ::open(path, O_RDONLY | O_NOFOLLOW | O_CLOEXEC);
    if (fd < 0 && errno == ENOENT) {
      fd = ::open(path, O_CREAT | O_EXCL | O_RDONLY | O_NOFOLLOW | O_CLOEXEC, 0644);
      if (fd >= 0) (void)::fchmod(fd, 0644);
      else if (errno == EEXIST) fd = ::open(path, O_RDONLY | O_NOFOLLOW | O_CLOEXEC);  // (somebody else created it meanwhile)
    }
    if (fd < 0) {
      static std::atomic<bool> said{false};
      if (!said.exchange(true))
        std::fprintf(stderr, "libwfst_amd: no per-device lock file (%s: %s); resident launches of several processes on one GPU are only "
                             "protected by their wait limit (WFST_LOCK_DIR selects another directory)\n", path, std::strerror(errno));
    }
    sl.fd = fd;
    return fd;
  }
  struct Units { std::mutex mu; int used = 0; int fd = -1; };
  static Units& units_of(int device) {
    static Units u[64];
    return u[(unsigned)device & 63u];
  }
  bool acquire(int device, int units = 2) {
    release();
    Units& u = units_of(device);
    std::lock_guard<std::mutex> lk(u.mu);
    if (u.used + units > 2) return false;
    if (u.used == 0) {
      const int fd = device_lock_fd(device);
      if (fd >= 0 && ::flock(fd, LOCK_EX | LOCK_NB) != 0) return false;  // another process holds the device's resident slot
      u.fd = fd;
    }
    u.used += units;
    held_device = device;
    held_units = units;
    return true;
  }
  void release() {
    if (held_units) {
      Units& u = units_of(held_device);
      std::lock_guard<std::mutex> lk(u.mu);
      u.used -= held_units;
      if (u.used == 0 && u.fd >= 0) {
        (void)::flock(u.fd, LOCK_UN);
        u.fd = -1;
      }
    }
    held_units = 0;
    held_device = -1;
  }
  ~ResidentLease() { release(); }
};

// Beside the lease's counter, per device and process: did the last solve that finished on the device run WIDE levels in a
// resident launch?  record_solve writes it, the string kernels' placement reads it (string_placement.h): a grid of ~245
// whole compute units is then likely at work beside the next batch.  A process that has never solved reads "no".
std::atomic<uint8_t>& resident_work_of(int device) {
  static std::atomic<uint8_t> w[64];
  return w[(unsigned)device & 63u];
}

}  // namespace
bool resident_grid_at_work(int device) { return resident_work_of(device).load(std::memory_order_relaxed) != 0; }
}  // namespace wfst
bool wfst_ctx::resident_allowed() const {
  if (resident_hold) return false;
  if (resident_retry_at_ns == 0) return true;
  return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count() >= resident_retry_at_ns;
}
void wfst_ctx::resident_aborted(int64_t fixed_pause_ms) {
  const int64_t pause_ms = fixed_pause_ms >= 0 ? fixed_pause_ms : 50ll << std::min<uint32_t>(resident_abort_streak, 6u);
  resident_abort_streak += 1;
  resident_retry_at_ns = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count() +
                         pause_ms * 1000000ll;
  if (resident_retry_at_ns == 0) resident_retry_at_ns = 1;
}
namespace wfst {
namespace {

// The WFST_SSSP_* variables a solve reads (experiments and tests), in the order of the appendix of DESIGN.md, which says what
// each one does.  An empty optional / null / false = not set: the default stands where the variable is used.
// A NEW FIELD GOES INTO knobs_same_plan BELOW AS WELL (the solo query runs only under the knobs its scratch was planned with);
// the static_assert behind that function stops the build until both have been visited.
struct Knobs {
  std::optional<int> mailbox;           // WFST_SSSP_MAILBOX
  std::optional<uint32_t> narrow;       // WFST_SSSP_NARROW
  std::optional<bool> hint;             // WFST_SSSP_HINT
  bool big = false;                     // WFST_SSSP_BIG
  std::optional<uint32_t> stg;          // WFST_SSSP_STG
  std::optional<float> delta;           // WFST_SSSP_DELTA
  std::optional<uint32_t> near_low;     // WFST_SSSP_NEAR_LOW
  float tau0_mult = 1.0f;               // WFST_SSSP_TAU0_MULT
  std::optional<uint32_t> chase_cap, chase_rounds, chase_low;  // WFST_SSSP_CHASE_CAP / _ROUNDS / _LOW
  const char* mbox_trace = nullptr;     // WFST_SSSP_MBOX_TRACE
  int resident = 1;                     // WFST_SSSP_RESIDENT
  std::optional<uint32_t> res_levels;   // WFST_SSSP_RES_LEVELS
  std::optional<long long> res_tlim_us; // WFST_SSSP_RES_TLIM_US
  bool log12 = false;                   // WFST_SSSP_LOG12 (by presence)
  const char* res_trace = nullptr;      // WFST_SSSP_RES_TRACE
  int binned = 0;                       // WFST_SSSP_BINNED
  std::optional<long long> dense_low;   // WFST_SSSP_DENSE_LOW
  bool bin_log14 = false;               // WFST_SSSP_BIN_LOG
  std::optional<uint32_t> bin_hopcap;   // WFST_SSSP_BIN_HOPCAP
  int64_t res_retry_ms = -1;            // WFST_SSSP_RES_RETRY_MS (-1: the doubling pause)
  bool test_fail_log13 = false;         // WFST_SSSP_TEST_FAIL_LOG13 (by presence)
  bool event_wait = false;              // WFST_SSSP_EVENT_WAIT (by presence)
  bool log13 = false;                   // WFST_SSSP_LOG13
  std::optional<int> lps;               // WFST_SSSP_LPS
  std::optional<int> umax;              // WFST_SSSP_UMAX
  bool split_tail = false;              // WFST_SSSP_SPLIT_TAIL (by presence)
  bool count_atomics = false;           // WFST_SSSP_COUNT_ATOMICS (by presence)
  int final_list = 1;                   // WFST_SSSP_FINAL_LIST
  int early_tail = 1;                   // WFST_SSSP_EARLY_TAIL
  int early_best = 1;                   // WFST_SSSP_EARLY_BEST
  int rearm = 1;                        // WFST_SSSP_REARM
  int bounded = 1;                      // WFST_SSSP_BOUNDED
  int solo = 1;                         // WFST_SSSP_SOLO
  std::optional<uint32_t> solo_log;     // WFST_SSSP_SOLO_LOG
};
// Field by field, every knob that shapes a solve's plan or route (the solo query compares the knobs of the call with those the
// parked scratch was planned under: RearmRecord::solo).  Not `solo` / `solo_log`, which only say whether and how that route is
// tried; a trace file on either side is "different" (the solo kernel writes none).
bool knobs_same_plan(const Knobs& a, const Knobs& b) {
  return a.mailbox == b.mailbox && a.narrow == b.narrow && a.hint == b.hint && a.big == b.big && a.stg == b.stg && a.delta == b.delta &&
         a.near_low == b.near_low && a.tau0_mult == b.tau0_mult && a.chase_cap == b.chase_cap && a.chase_rounds == b.chase_rounds &&
         a.chase_low == b.chase_low && !a.mbox_trace && !b.mbox_trace && a.resident == b.resident && a.res_levels == b.res_levels &&
         a.res_tlim_us == b.res_tlim_us && a.log12 == b.log12 && !a.res_trace && !b.res_trace && a.binned == b.binned &&
         a.dense_low == b.dense_low && a.bin_log14 == b.bin_log14 && a.bin_hopcap == b.bin_hopcap && a.res_retry_ms == b.res_retry_ms &&
         a.test_fail_log13 == b.test_fail_log13 && a.event_wait == b.event_wait && a.log13 == b.log13 && a.lps == b.lps &&
         a.umax == b.umax && a.split_tail == b.split_tail && a.count_atomics == b.count_atomics && a.final_list == b.final_list &&
         a.early_tail == b.early_tail && a.early_best == b.early_best && a.rearm == b.rearm && a.bounded == b.bounded;
}
constexpr size_t KNOBS_BYTES = 232;
static_assert(sizeof(Knobs) == KNOBS_BYTES, "Knobs has changed: add the field to knobs_same_plan, then update KNOBS_BYTES");

// Read once per solve, by relax_setup — not once per process: tests and tools change the variables between two solves.
// One pass over the environment (EnvSnap) instead of a getenv per variable: this runs in front of the first launch.
Knobs read_knobs() {
  const EnvSnap env = EnvSnap::take();
  Knobs k;
  if (const char* e = env.get("WFST_SSSP_MAILBOX")) k.mailbox = std::atoi(e);
  if (const char* e = env.get("WFST_SSSP_NARROW")) k.narrow = (uint32_t)std::atol(e);
  if (const char* e = env.get("WFST_SSSP_HINT")) k.hint = std::atoi(e) != 0;
  if (const char* e = env.get("WFST_SSSP_BIG")) k.big = std::atoi(e) != 0;
  if (const char* e = env.get("WFST_SSSP_STG")) k.stg = (uint32_t)std::atoi(e);
  if (const char* e = env.get("WFST_SSSP_DELTA")) k.delta = (float)std::atof(e);
  if (const char* e = env.get("WFST_SSSP_NEAR_LOW")) k.near_low = (uint32_t)std::atol(e);
  if (const char* e = env.get("WFST_SSSP_TAU0_MULT")) k.tau0_mult = (float)std::atof(e);
  if (const char* e = env.get("WFST_SSSP_CHASE_CAP")) k.chase_cap = std::min<uint32_t>((uint32_t)std::atol(e), CHASE_MAX);
  if (const char* e = env.get("WFST_SSSP_CHASE_ROUNDS")) k.chase_rounds = (uint32_t)std::atol(e);
  if (const char* e = env.get("WFST_SSSP_CHASE_LOW")) k.chase_low = (uint32_t)std::atol(e);
  k.mbox_trace = env.get("WFST_SSSP_MBOX_TRACE");
  if (const char* e = env.get("WFST_SSSP_RESIDENT")) k.resident = std::atoi(e);
  if (const char* e = env.get("WFST_SSSP_RES_LEVELS")) k.res_levels = std::max<uint32_t>(2u, std::min<uint32_t>(RS_LEVEL_CAP, (uint32_t)std::atol(e)));
  if (const char* e = env.get("WFST_SSSP_RES_TLIM_US")) k.res_tlim_us = std::atoll(e);
  k.log12 = env.get("WFST_SSSP_LOG12") != nullptr;
  k.res_trace = env.get("WFST_SSSP_RES_TRACE");
  if (const char* e = env.get("WFST_SSSP_BINNED")) k.binned = std::atoi(e);
  if (const char* e = env.get("WFST_SSSP_DENSE_LOW")) k.dense_low = std::atoll(e);
  if (const char* e = env.get("WFST_SSSP_BIN_LOG")) k.bin_log14 = std::atoi(e) == 14;
  if (const char* e = env.get("WFST_SSSP_BIN_HOPCAP")) k.bin_hopcap = (uint32_t)std::atol(e);
  if (const char* e = env.get("WFST_SSSP_RES_RETRY_MS")) k.res_retry_ms = std::max<long long>(0ll, std::atoll(e));
  k.test_fail_log13 = env.get("WFST_SSSP_TEST_FAIL_LOG13") != nullptr;
  k.event_wait = env.get("WFST_SSSP_EVENT_WAIT") != nullptr;
  if (const char* e = env.get("WFST_SSSP_LOG13")) k.log13 = std::atoi(e) != 0;
  if (const char* e = env.get("WFST_SSSP_LPS")) k.lps = std::max(2, std::min(8, std::atoi(e)));
  if (const char* e = env.get("WFST_SSSP_UMAX")) k.umax = std::atoi(e) >= 4 ? 4 : 2;
  k.split_tail = env.get("WFST_SSSP_SPLIT_TAIL") != nullptr;
  k.count_atomics = env.get("WFST_SSSP_COUNT_ATOMICS") != nullptr;
  if (const char* e = env.get("WFST_SSSP_FINAL_LIST")) k.final_list = std::atoi(e);
  if (const char* e = env.get("WFST_SSSP_EARLY_TAIL")) k.early_tail = std::atoi(e);
  if (const char* e = env.get("WFST_SSSP_EARLY_BEST")) k.early_best = std::atoi(e);
  if (const char* e = env.get("WFST_SSSP_REARM")) k.rearm = std::atoi(e);
  if (const char* e = env.get("WFST_SSSP_BOUNDED")) k.bounded = std::atoi(e);
  if (const char* e = env.get("WFST_SSSP_SOLO")) k.solo = std::atoi(e);
  if (const char* e = env.get("WFST_SSSP_SOLO_LOG")) k.solo_log = std::max<uint32_t>(1u, (uint32_t)std::atol(e));
  return k;
}

struct Solve {
  Knobs kn;  // as the environment stood when relax_setup began this solve
  DBuf<uint64_t> key;
  DBuf<uint32_t> shadow;  // enc(d) half of the keys, for the pre-check gathers
  DBuf<uint8_t> flags;  // two frontiers of n bytes
  DBuf<uint32_t> improved;
  DBuf<Ctl> ctl;
  uint32_t sweeps = 0;
  // Re-armed scratch (wfst_ctx::rearm): `armed` = this solve started from the parked scratch of the last one — no set-up launch
  // was queued and launch 0 seeds the start state itself (EarlyTail::seed); otherwise `rearm_why` says why not (WFST_SSSP_REARM=2).
  // `rearm_unproven`, inside relax_setup only: buffers of this solve are parked blocks that the re-arm launch may still be writing —
  // none of them goes back to the pool before the stream has been waited for.
  bool armed = false, rearm_unproven = false;
  const char* rearm_why = "nothing parked";
  uint32_t rearm_stops = 0;  // armed: RearmRecord::stops / ::epoch of the scratch this solve adopted (the solo query's streak)
  uint64_t rearm_epoch = 0;
  float tau0 = 0.0f;  // threshold of sweep 0, as the set-up (or the re-arm launch of the solve before) leaves it in Ctl::tau0
  // schedule parameters fixed by relax_setup
  uint8_t* fl[2] = {nullptr, nullptr};
  uint32_t blocks = 1, near_low = 4096;
  float delta = 0.0f;
  uint64_t sweep_cap = 0;
  // per-wave list of near discoveries relaxed inside the same launch, in sweeps that follow a small (< chase_low) one
  uint32_t chase_cap = 32, chase_rounds = 8, chase_low = 4096;  // chase_rounds = states a wave may chase per launch
  // mailbox sweeps (sssp_mailbox.h): owner-computes relaxation, chosen by relax_setup for branching graphs of <= 2^20 states
  bool mbox = false;
  std::shared_ptr<MboxPlan> plan;
  DBuf<uint2> mb_msgs;      // two message buffers of n_arcs entries
  DBuf<uint32_t> mb_words;  // counts (2 x nb^2), wrote (2 x nb), pend masks, blk_pend, blk_mind, blk_far, wl_cnt, blk_best (nb x 64 bits)
  DBuf<uint4> mb_wl;        // work-list segments of the NARROW launches (nb x NW_SEG entries)
  DBuf<unsigned long long> mb_dbg;  // WFST_SSSP_MBOX_TRACE=<file>: per-block phase stamps of the first 64 sweeps
  MboxView mv{};
  uint32_t narrow_t = 0;     // mailbox: near + far-waiting states below which the sweeps hand over to NARROW launches (0 = never)
  uint64_t hint_mask = ~0ull;  // mailbox: bit k = launch k of this FST's last solve was not a busy WIDE sweep (gated launch)
  size_t mb_dyn = 0;         // dynamic LDS bytes of a mailbox launch
  bool force_big = false;    // tests: the many-blocks variant of the kernel on a small FST (WFST_SSSP_BIG=1)
  decltype(&sssp_mbox_kernel<false>) mbox_kernel = nullptr;  // the variant for this many blocks (bind_mailbox)
  // the bounded head (mbox_narrow<LOG, true>): launch 0 of this solve is the instance that ends the search once the best final
  // state is settled (set by shortest_path_n1_begin before the first batch is queued, with EarlyTail::finals); otherwise
  // `bounded_why` says why the solve is not eligible (WFST_SSSP_BOUNDED=2)
  decltype(&sssp_mbox_kernel<false>) mbox_head_kernel = nullptr;
  bool bounded_on = false;
  const char* bounded_why = "not a repeated single-path query";
  // the early tail (sssp_early_tail): the one-level launches get a workgroup more, which does the tail's work inside the
  // NARROW launch that drains the search (set by shortest_path_n1_begin before the first batch is queued)
  bool early_on = false;
  EarlyTail early{};
  // ... and the resident launch in front of that NARROW launch leaves every block's best final state for it (mbox_blk_best;
  // the kernel's `blk_finals` is null and EarlyTail::blk_best_on 0 unless this is on): early tail, 4096-state blocks, a resident
  // launch, WFST_SSSP_EARLY_BEST
  bool blk_best_on = false;
  // resident launches (sssp_resident.h): the WIDE levels of the solve inside ONE launch, every workgroup on a CU of its own
  bool resident = false;
  uint32_t log = 12;         // log2 of the block size (13: every launch of the solve is a resident one)
  size_t res_dyn = 0;        // dynamic LDS bytes of a resident launch
  decltype(&sssp_mbox_resident_kernel<12>) res_kernel = nullptr;  // the variant for this block size (bind_resident)
  DBuf<uint2> rs_msgs;       // two parity buffers of plan->res_units entries
  DBuf<uint32_t> rs_abort;   // one word
  DBuf<unsigned long long> rs_trace;  // WFST_SSSP_RES_TRACE=<file>: per-level stamps
  ResView rv{};
  uint32_t res_max_levels = RS_LEVEL_CAP;
  uint32_t res_lps_umax = 8u | (2u << 8);  // lanes per listed state | states per lane group of the widest round (sssp_resident.h)
  ResidentLease lease;       // units of the device's resident lease this solve holds (2 = whole device, 1 = half: two of those run together)
  // binned levels (sssp_binned.h): the dense levels of the atomic sweeps as an owner-computes pass, chosen per level on the device
  bool binned = false;
  std::shared_ptr<BinPlan> bplan;
  DBuf<uint2> bn_msgs;       // one slot per arc
  DBuf<uint32_t> bn_cnt;     // [nbin * G]
  BinView bv{};
  uint32_t dense_low = 0xFFFFFFFFu;  // predicted frontier from which a level is a binned one
  size_t bn_dyn_expand = 0, bn_dyn_apply = 0;
  decltype(&sssp_bin_expand_kernel<13>) bin_expand_kernel = nullptr;  // the variants for this bin size (bind_binned)
  decltype(&sssp_bin_apply_kernel<13>) bin_apply_kernel = nullptr;
};

// Raises the dynamic-LDS limit of `kernels`, once per device (a function attribute is per device); `once` belongs to the call site.
struct OncePerDevice {
  std::once_flag flag[64];
};
void raise_dynamic_lds(OncePerDevice& once, int device, int bytes, std::initializer_list<const void*> kernels) {
  std::call_once(once.flag[(unsigned)device & 63u], [&] {
    for (const void* k : kernels) HIP_CHECK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  });
}

constexpr uint32_t MAX_BATCH = 64;

// The relaxation runs to its fixed point in sweeps launched in batches without returning to the host, and the NEXT
// batch is enqueued before the host looks at the previous batch's flags (two batches in flight), so the device never
// idles on a host round trip.  A sweep that changes nothing leaves an empty frontier: everything enqueued behind it is
// a ~3 us no-op.
bool mbox_eligible(const wfst_fst* f) {
  return f->n_states <= (MB_NBMAX_BIG << MB_LOG) && f->n_arcs > 0 && f->n_arcs < 0x7FFFFFFFull && !f->has_negative;
}

// Region plan of the mailbox sweeps: arcs between every pair of blocks, scanned into region offsets.  Depends only on
// the (source, target) pairs of the arcs, so tr_sort leaves it valid; cached on the handle (owner's pool).
std::shared_ptr<MboxPlan> mbox_plan(wfst_ctx* ctx, const wfst_fst* f, uint32_t log, const Knobs& kn) {
  std::lock_guard<std::mutex> lk(f->cache_mu);
  std::shared_ptr<MboxPlan>& slot = log == 13 ? f->mbox13 : f->mbox;
  if (slot) return slot;
  const uint32_t n = f->n_states, nb = (uint32_t)(((uint64_t)n + (1u << log) - 1) >> log);
  hipStream_t st = ctx->stream;
  DevicePool& owner_pool = f->owner_pool ? *f->owner_pool : *ctx->pool;
  auto p = std::make_shared<MboxPlan>();
  p->nb = nb;
  p->log = log;
  const size_t cells = (size_t)nb * nb;
  p->roff = DBuf<uint32_t>(owner_pool, cells + 1);
  p->roff_t = DBuf<uint32_t>(owner_pool, cells);
  DBuf<uint32_t> hist(*ctx->pool, cells + 1);
  const auto hist_kernel = log == 13 ? mbox_hist_kernel<13> : mbox_hist_kernel<12>;
  hist_kernel<<<nb, 1024, 0, st>>>(f->dev.offsets, f->dev.wn, n, nb, hist.p);
  HIP_CHECK(hipMemsetAsync(hist.p + cells, 0, sizeof(uint32_t), st));
  const DBuf<uint8_t> scan_tmp = exclusive_scan_u32(ctx, hist.p, p->roff.p, cells + 1);
  mbox_transpose_kernel<<<(uint32_t)((cells + 255) / 256), 256, 0, st>>>(p->roff.p, nb, p->roff_t.p);
  // lanes per state of the resident kernel's expansion rounds (a lane takes two arcs): the fewest that cover all but 1/64 of
  // the rows in one pass — a lane group without arcs is a lane group that keeps no row in flight — and leave at most 1/16 of
  // the ARCS to the long-row pass (a few states with hundreds of arcs each, as in a decoding graph, would otherwise be walked 2 l
  // arcs at a time by one lane group while the rest of its wave waits)
  {
    DBuf<uint32_t> over(*ctx->pool, 16);
    DBuf<double> minw(*ctx->pool, 2);
    uint32_t h_over[16];
    double h_minw[2];
    HIP_CHECK(hipMemsetAsync(over.p, 0, sizeof(h_over), st));
    HIP_CHECK(hipMemsetAsync(minw.p, 0, sizeof(h_minw), st));
    mbox_degree_kernel<<<std::min<uint32_t>((n + 255) / 256, 1024u), 256, 0, st>>>(f->dev.offsets, f->dev.wn, n, over.p, minw.p);
    HIP_CHECK(hipMemcpyAsync(h_over, over.p, sizeof(h_over), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(h_minw, minw.p, sizeof(h_minw), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    p->mean_min_w = h_minw[1] > 0.0 ? (float)(h_minw[0] / h_minw[1]) : 0.0f;
    p->lps = 8;
    for (uint32_t l = 2; l < 8; ++l)
      if (h_over[l] <= n / 64u && (uint64_t)h_over[8 + l] <= f->n_arcs / 16u && h_over[8 + l] != 0xFFFFFFFFu) {
        p->lps = l;
        break;
      }
    if (kn.lps) p->lps = (uint32_t)*kn.lps;
  }
  uint32_t h_units = 0;
  if (nb <= MB_NBMAX) {  // the resident kernel's regions: header + one slot per arc, 64-byte aligned
    p->roffh = DBuf<uint32_t>(owner_pool, cells + 1);
    p->roffh_t = DBuf<uint32_t>(owner_pool, cells);
    DBuf<uint32_t> sizes(*ctx->pool, cells + 1);
    res_size_kernel<<<(uint32_t)((cells + 1 + 255) / 256), 256, 0, st>>>(hist.p, (uint32_t)cells, sizes.p);
    const DBuf<uint8_t> scan_tmp2 = exclusive_scan_u32(ctx, sizes.p, p->roffh.p, cells + 1);
    mbox_transpose_kernel<<<(uint32_t)((cells + 255) / 256), 256, 0, st>>>(p->roffh.p, nb, p->roffh_t.p);
    HIP_CHECK(hipMemcpyAsync(&h_units, p->roffh.p + cells, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(st));  // sizes is released here
    p->res_units = h_units;
  }
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(st));  // hist / scan_tmp are released here
  slot = p;
  return p;
}

// Region plan of the binned levels (sssp_binned.h), cached on the handle like the mailbox plan.
bool bin_eligible(const wfst_fst* f) {
  return f->n_states <= (BN_MAXBINS << 14) && f->n_arcs > 0 && f->n_arcs < 0x7FFFFFFFull && !f->has_negative;
}
std::shared_ptr<BinPlan> bin_plan(wfst_ctx* ctx, const wfst_fst* f, uint32_t logd) {
  std::lock_guard<std::mutex> lk(f->cache_mu);
  if (f->binplan && f->binplan->logd == logd) return f->binplan;
  const uint32_t n = f->n_states;
  hipStream_t st = ctx->stream;
  DevicePool& owner_pool = f->owner_pool ? *f->owner_pool : *ctx->pool;
  auto p = std::make_shared<BinPlan>();
  p->logd = logd;
  p->nbin = (uint32_t)(((uint64_t)n + (1u << logd) - 1) >> logd);
  // two expand workgroups per compute unit; a workgroup's range is a whole number of chunks
  const uint32_t g_max = (uint32_t)std::min<int>(512, std::max<int>(1, 2 * ctx->n_cus));
  p->sg = (uint32_t)(((((uint64_t)n + g_max - 1) / g_max) + BN_CH - 1) / BN_CH * BN_CH);
  p->G = (uint32_t)(((uint64_t)n + p->sg - 1) / p->sg);
  const size_t cells = (size_t)p->nbin * p->G;
  p->roff = DBuf<uint32_t>(owner_pool, cells + 1);
  p->roff_t = DBuf<uint32_t>(owner_pool, cells);
  DBuf<uint32_t> hist(*ctx->pool, cells + 1);
  const auto hist_kernel = logd == 14 ? bin_hist_kernel<14> : bin_hist_kernel<13>;
  hist_kernel<<<p->G, 1024, 0, st>>>(f->dev.offsets, f->dev.wn, n, p->sg, p->nbin, p->G, hist.p);
  HIP_CHECK(hipMemsetAsync(hist.p + cells, 0, sizeof(uint32_t), st));
  const DBuf<uint8_t> scan_tmp = exclusive_scan_u32(ctx, hist.p, p->roff.p, cells + 1);
  bin_transpose_kernel<<<(uint32_t)((cells + 255) / 256), 256, 0, st>>>(p->roff.p, p->nbin, p->G, p->roff_t.p);
  uint32_t h_slots = 0;
  HIP_CHECK(hipMemcpyAsync(&h_slots, p->roff.p + cells, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(st));  // hist / scan_tmp are released here
  p->slots = h_slots;
  f->binplan = p;
  return p;
}

// what the next solve of this FST is sized from: the launches this one needed, and how long that count has been the same
void note_sweeps(const wfst_fst* f, uint32_t sweeps) {
  const uint32_t prev = f->last_sweeps.exchange(sweeps, std::memory_order_relaxed);
  if (prev == sweeps) f->stable_sweeps.fetch_add(1, std::memory_order_relaxed);
  else f->stable_sweeps.store(0, std::memory_order_relaxed);
}

// one relaxation sweep on the stream: `j` = position inside the batch (static flag / message parity), `off` = sweep
// index relative to the device-side base, `abs_sweep` = the absolute index (what the host has queued so far)
void launch_sweep(const wfst_fst* f, Solve& sv, uint32_t n, hipStream_t st, uint32_t j, uint32_t off, uint32_t abs_sweep,
                  uint32_t profile) {
  if (sv.mbox) {
    // (message parity from the ABSOLUTE sweep index: mailbox batches may hold an odd number of sweeps)
    // hint = the launch is probably NOT a busy WIDE sweep (what the last solve of this FST did in that slot, or unknown):
    // it then finds out its mode and whether it sleeps BEFORE it asks for its 48 KB of keys and offsets
    const uint32_t hint = profile || abs_sweep >= 64 ? 1u : (uint32_t)((sv.hint_mask >> abs_sweep) & 1ull);
    // resident launches take the odd slots: slot 0 is the head of the search (NARROW), a resident launch runs every WIDE
    // level that follows and the hand-over, the next slot is the NARROW launch that drains the search; whichever kernel
    // finds another mode in its slot does that mode's work (the two kernels leave the same state behind)
    // (blocks of 8192 states exist in the resident kernel only: it also runs the NARROW launches of such a solve)
    if (sv.log == 13 && abs_sweep >= RS_MAX_SWEEP) throw Error("shortest_path: relaxation did not converge");
    if (sv.log == 13 || (sv.resident && !profile && (abs_sweep & 1u) && abs_sweep < RS_MAX_SWEEP))
      sv.res_kernel<<<sv.mv.nb, MB_THREADS, sv.res_dyn, st>>>(f->dev.offsets, f->dev.wn, sv.key.p, sv.mv, sv.rv, abs_sweep & 1u, n,
                                                              sv.improved.p, sv.ctl.p, abs_sweep, sv.delta, sv.near_low, sv.narrow_t,
                                                              sv.res_max_levels, sv.res_lps_umax, sv.blk_best_on ? f->dev.finals : nullptr);
    else {
      EarlyTail et = sv.early;
      et.seed = sv.armed && abs_sweep == 0 ? (uint32_t)f->start + 1u : 0u;  // (re-armed scratch: no set-up launch seeded the start state)
      // (launch 0 of a query whose head may end the search: the bounded instance; never under profiling)
      const auto kernel = sv.bounded_on && abs_sweep == 0 && !profile ? sv.mbox_head_kernel : sv.mbox_kernel;
      kernel<<<sv.mv.nb + (sv.early_on && !profile ? 1u : 0u), MB_THREADS, sv.mb_dyn, st>>>(
          f->dev.offsets, f->dev.wn, sv.key.p, sv.mv, abs_sweep & 1u, n, sv.improved.p, sv.ctl.p, abs_sweep, sv.delta, sv.near_low, profile,
          hint, sv.narrow_t, et);
    }
  } else {
    uint8_t* const cur = sv.fl[j & 1u];
    uint8_t* const next = sv.fl[(j & 1u) ^ 1u];
    sssp_relax_kernel<<<sv.blocks, 256, 0, st>>>(f->dev.offsets, f->dev.wn, sv.key.p, cur, next, n, sv.improved.p, sv.ctl.p, off,
                                                 sv.delta, sv.near_low, sv.shadow.p, sv.chase_cap, sv.chase_rounds, sv.chase_low,
                                                 profile, sv.binned ? sv.dense_low : 0xFFFFFFFFu);
    if (sv.binned) {  // the same level as an owner-computes pass: both leave at once unless the launch above published a dense level
      sv.bin_expand_kernel<<<sv.bv.G, BN_THREADS, sv.bn_dyn_expand, st>>>(f->dev.offsets, f->dev.wn, sv.key.p, cur, next, n,
                                                                          sv.improved.p, sv.ctl.p, off, sv.shadow.p, sv.bv, profile);
      sv.bin_apply_kernel<<<sv.bv.nbin, BN_THREADS, sv.bn_dyn_apply, st>>>(sv.key.p, sv.shadow.p, next, n, sv.improved.p, sv.ctl.p,
                                                                           off, sv.bv);
    }
  }
}

// ---- re-armed scratch (wfst_ctx::rearm).  What relax_setup took out of the context's record for the solve it sets
// up: the six blocks, live again, each handed to the buffer that would otherwise have been allocated.  The re-arm launch that
// cleans them may still be running, so whatever no buffer took waits for the stream before it goes back to the pool.
enum : size_t { RH_KEY = 0, RH_MB_WORDS, RH_IMPROVED, RH_CTL, RH_RS_MSGS, RH_RS_ABORT };
void rearm_prove(wfst_ctx* ctx, Solve& sv) {  // before a buffer of sv goes back to the pool inside relax_setup
  if (!sv.rearm_unproven) return;
  (void)hipStreamSynchronize(ctx->stream);
  sv.rearm_unproven = false;
}
struct RearmHeld {
  wfst_ctx* ctx;
  RearmRecord rec;  // (plan null: nothing was taken)
  explicit RearmHeld(wfst_ctx* c) : ctx(c) {}
  RearmHeld(const RearmHeld&) = delete;
  RearmHeld& operator=(const RearmHeld&) = delete;
  ~RearmHeld() { settle(); }
  bool left() const {
    for (void* b : rec.blk)
      if (b) return true;
    return false;
  }
  void settle() {
    if (!left()) return;
    (void)hipStreamSynchronize(ctx->stream);
    for (void*& b : rec.blk) {
      ctx->pool->free(b);
      b = nullptr;
    }
  }
  template <class T>
  void take_or_alloc(Solve& sv, DBuf<T>& buf, size_t idx, size_t count) {
    void* b = rec.cnt[idx] == count ? rec.blk[idx] : nullptr;
    if (b) {
      rec.blk[idx] = nullptr;
      sv.rearm_unproven = true;
      buf = DBuf<T>::adopt(*ctx->pool, b, count);
    } else {
      buf = DBuf<T>(*ctx->pool, count);
    }
  }
};
// The parked scratch of ctx for the solve of f that relax_setup begins, as far as can be told before the solve is planned
// (the rest is compared once it is: relax_setup).  Returns why nothing was taken, null when the blocks are in `held`.
const char* rearm_take(wfst_ctx* ctx, const wfst_fst* f, const Knobs& kn, RearmHeld& held) {
  RearmRecord& r = ctx->rearm;
  if (!r.plan) return "nothing parked";
  const char* why = nullptr;
  if (kn.rearm == 0 || ctx->profiling) {
    why = "not eligible";
  } else {
    std::lock_guard<std::mutex> lk(f->cache_mu);
    if (f->mbox != r.plan || f->n_states != r.n) why = "parked for another plan";
  }
  if (why) {
    rearm_drop(ctx);
    return why;
  }
  if (!ctx->pool->unpark(r.blk, RearmRecord::BLOCKS)) {  // (the pool's trim: hipFree has waited for the re-arm launch)
    r.clear();
    ctx->rearm_stats.dropped += 1;
    return "blocks reclaimed";
  }
  held.rec = std::move(r);
  r.clear();
  return nullptr;
}

// ---- relax_setup, piece by piece: the band, the block size and the lease, the mailbox plan, the two views, the binned levels

// near-far only pays on branching graphs (label-correcting re-relaxes them many times); on lattices every
// arc is relaxed once anyway.  delta = 1.5 x mean arc weight; +inf = plain frontier sweeps.
float band_from_mean_weight(const wfst_fst* f, const Knobs& kn) {
  const uint32_t n = f->n_states;
  float delta = INF;
  if (!f->has_negative && f->mean_weight > 0.0f && n >= 65536 && f->n_arcs >= 2ull * n) {
    delta = 1.5f * f->mean_weight;
    // ... of a graph with ~10 arcs per state.  With more, a state's BEST arc is cheaper (the minimum of d weights) while the
    // mean is not, the distances shrink and a band of 1.5 mean weights swallows the search: everything is near, everything is
    // relaxed again and again; with fewer, the band holds a few dozen states per level for many levels.  The band follows
    // 10 / (arcs per state) — 1M states (tools/fan_sweep.py): fan-out 3 / 4 / 5 / 6 / 8: 247 / 254 / 223 / 236 / 229 -> 189 /
    // 193 / 191 / 200 / 223 us; 12 / 16 / 24: 366 / 638 / 1 262 -> 275 / 327 / 523 — except between 8.5 and 10 arcs per state,
    // where the schedule was swept on the benchmark's transducer and the unscaled band is the better one (fan-out 9: 233 against 256).
    const double deg = (double)f->n_arcs / (double)n;
    if (deg > 10.0 || deg < 8.5) delta = (float)(delta * 10.0 / deg);
  }
  if (kn.delta) delta = *kn.delta;  // experiments / tests
  return delta > 0.0f ? delta : INF;
}

// The band once more, now that the plan knows the states' CHEAPEST arcs: the rule above reads the mean weight as if the
// weights were uniform on [0, 2 mean) — a state's best of d arcs then costs 2 mean / (d + 1).  Where the cheapest arcs are
// much cheaper than that (exponential, log-normal weights: a shortest path is made of them) the band shrinks by the same
// ratio; where every arc costs about the same (unit weights: the search is a breadth-first one) it widens a little.
// 1M states, fan-out 10 (tools/weight_shapes.py): exponential 410 -> 241 us, unit weights 205 -> ~125; uniform weights
// (ratio 0.9 .. 1.1): untouched.
float band_from_cheapest_arcs(const wfst_fst* f, const MboxPlan& plan, float delta, const Knobs& kn) {
  if (!(delta < INF) || kn.delta || !(plan.mean_min_w > 0.0f) || !(f->mean_weight > 0.0f)) return delta;
  const double deg = (double)f->n_arcs / (double)f->n_states;
  const double ratio = (double)plan.mean_min_w * (deg + 1.0) / (2.0 * (double)f->mean_weight);
  if (ratio < 0.7) return (float)(delta * std::max(ratio, 0.1));
  if (ratio > 2.0) return delta * 1.4f;
  return delta;
}

// log2 of the block size with which the blocks of a resident solve each get a compute unit of their own — 4096 states, or
// 8192 for the FSTs of 1M .. 2M states that then still fit one block per CU (every launch of such a solve is a resident
// one) —, 0 when neither does.
uint32_t resident_block_log(const wfst_ctx* ctx, uint32_t n, const Knobs& kn) {
  const uint32_t cus = (uint32_t)std::min<int>(ctx->n_cus, (int)MB_NBMAX);
  const uint32_t nb12 = (n + 4095u) >> 12, nb13 = (uint32_t)(((uint64_t)n + 8191u) >> 13);
  // wfst_ctx_set_resident_share(ctx, 1): the resident grid may hold at most half of the compute units, so that a large batch
  // kernel of another context runs BESIDE it (a resident workgroup needs a compute unit of its own; a grid that wants 245 of
  // 256 waits for whatever holds more than 11 of them).  8192-state blocks where that is enough, one launch per level otherwise.
  if (ctx->resident_share == 1u) {
    const uint32_t half = cus / 2u;
    if (nb12 <= half) return 12;
    return nb13 <= half && !kn.log12 ? 13 : 0;
  }
  if (nb12 <= cus) return nb13 <= cus && kn.log13 ? 13 : 12;  // (WFST_SSSP_LOG13, experiments: half the workgroups)
  return nb13 <= cus && !kn.log12 ? 13 : 0;
}

// Resident launches (sssp_resident.h) need every block on a CU of its own for the whole launch, and only one such solve
// runs per device at a time: the lease is taken first, because it decides the block size (sv.log).  Not under the per-sweep
// profiler (it times launches), not after a launch of this context gave up waiting.  true = this solve holds the lease.
bool lease_resident(wfst_ctx* ctx, uint32_t n, Solve& sv) {
  const uint32_t log = resident_block_log(ctx, n, sv.kn);
  if (!(sv.kn.resident && log && !ctx->profiling && ctx->resident_allowed() && !sv.kn.big &&
        sv.lease.acquire(ctx->device, ctx->resident_share == 1u ? 1 : 2)))
    return false;
  sv.log = log;
  return true;
}

constexpr size_t RES_LDS_BYTES = 160u * 1024u;  // LDS of a compute unit
// Staging slots per destination that a resident launch on this plan has, 0 when such a launch is not possible: no resident
// regions (more than MB_NBMAX blocks), a region buffer beyond the buffer-descriptor range, or an LDS without room for 4 slots
// (up to MB_NBMAX blocks the one-level kernel's budget allows RS_STG_MAX of them, so what is returned is 0 or at least 4).
// (deeper than the one-level kernel's slots where the LDS has room: a round of the resident kernel holds up to 4 x 16 x
// (64 / lps) states, 768 with 5 lanes per state)
uint32_t resident_staging(const MboxPlan& plan) {
  if (plan.res_units == 0 || plan.res_units * sizeof(uint2) >= 0x7FFFFFF0ull) return 0;
  const uint32_t nb = plan.nb;
  const size_t fixed = res_lds_bytes(plan.log, nb, 0);
  if (fixed + 8u * 4u * nb > RES_LDS_BYTES) return 0;
  const uint32_t stg_lim = std::min<uint32_t>(RS_STG_MAX, (MB_DYN_BUDGET - 12u * nb) / (8u * nb));  // (the one-level kernel's budget)
  return (uint32_t)std::min<size_t>(stg_lim, (RES_LDS_BYTES - fixed) / (8u * nb));
}

// The plan and the buffers of the mailbox sweeps (sv.mbox), with those of the resident launches when `want_res`; returns
// whether the solve still has the latter.
// Two message buffers of one slot per arc, the nb^2 region tables and counts come from the pool: on a tight pool (or a
// dense graph) the atomic sweeps, which need none of it, run instead.  The 8192-state plan exists in the resident kernel
// only: when it cannot be had (the pool, a region buffer beyond the buffer-descriptor range, no room for staging), the
// solve is planned again with 4096-state blocks and one launch per level — never refused.
bool plan_mailbox(wfst_ctx* ctx, const wfst_fst* f, Solve& sv, bool want_res, RearmHeld& held) {
  DevicePool& pool = *ctx->pool;
  auto release_all = [&] {
    rearm_prove(ctx, sv);
    want_res = false;
    sv.rs_msgs.reset();
    sv.rs_abort.reset();
    sv.lease.release();
    sv.plan.reset();
    sv.mb_msgs.reset();
    sv.mb_words.reset();
    sv.mb_wl.reset();
    sv.mbox = false;
  };
  auto try_plan = [&](uint32_t log, bool res) -> bool {
    try {
      sv.log = log;
      sv.plan = mbox_plan(ctx, f, log, sv.kn);
      const uint32_t nb = sv.plan->nb;
      if (res && resident_staging(*sv.plan) == 0) {
        if (log == 13) throw Error("resident launch not possible");
        res = false;
        sv.lease.release();
      }
      sv.mb_msgs = DBuf<uint2>(pool, 2 * (size_t)f->n_arcs);
      const size_t w_cnt = (size_t)nb * nb, w_pend = (size_t)nb * ((1u << log) / 32);
      held.take_or_alloc(sv, sv.mb_words, RH_MB_WORDS, 2 * w_cnt + 2 * nb + w_pend + 4 * nb + 2 * nb);
      sv.mb_wl = DBuf<uint4>(pool, (size_t)nb << log);
      if (res) {  // what the resident launch needs beyond the plan
        held.take_or_alloc(sv, sv.rs_msgs, RH_RS_MSGS, 2 * (size_t)sv.plan->res_units);
        held.take_or_alloc(sv, sv.rs_abort, RH_RS_ABORT, 16);
      }
      want_res = res;
      sv.mbox = true;
      return true;
    } catch (const Error&) {
      (void)hipGetLastError();  // (a refused allocation must not surface at the next launch check)
      release_all();
      return false;
    }
  };
  if (sv.kn.test_fail_log13 && sv.log == 13) {  // tests: the 8192-state plan refused
    release_all();
    try_plan(12, false);
  } else if (!try_plan(sv.log, want_res) && sv.log == 13) {
    try_plan(12, false);
  }
  if (!sv.mbox) sv.log = 12;
  return want_res;
}

// MboxView over the planned buffers, and the schedule of a solve that takes one launch per level
void bind_mailbox(wfst_ctx* ctx, const wfst_fst* f, Solve& sv) {
  const uint32_t n = f->n_states, nb = sv.plan->nb;
  const size_t w_cnt = (size_t)nb * nb, w_pend = (size_t)nb * ((1u << sv.log) / 32);
  MboxView& mv = sv.mv;
  mv.roff = sv.plan->roff.p;
  mv.roff_t = sv.plan->roff_t.p;
  mv.msgs[0] = sv.mb_msgs.p;
  mv.msgs[1] = sv.mb_msgs.p + f->n_arcs;
  uint32_t* w = sv.mb_words.p;
  mv.cnt[0] = w;
  mv.cnt[1] = w + w_cnt;
  w += 2 * w_cnt;
  mv.wrote[0] = w;
  mv.wrote[1] = w + nb;
  w += 2 * nb;
  mv.pend = w;
  w += w_pend;
  mv.blk_pend = w;
  mv.blk_mind = w + nb;
  mv.blk_far = w + 2 * nb;
  mv.wl_cnt = w + 3 * nb;
  // (behind wl_cnt: blk_best, nb 64-bit words — an even number of 32-bit words in front of them: 8-byte aligned)
  sv.blk_best_on = false;  // (shortest_path_n1_begin switches it on)
  mv.wl = sv.mb_wl.p;
  mv.nb = nb;
  // staging depth: what the dynamic LDS budget leaves after the three per-destination tables
  mv.stg = std::max<uint32_t>(1u, std::min<uint32_t>(MB_STG_MAX, (MB_DYN_BUDGET - 12u * nb) / (8u * nb)));
  if (sv.kn.stg) mv.stg = std::max<uint32_t>(1u, std::min<uint32_t>(mv.stg, *sv.kn.stg));
  sv.force_big = sv.kn.big;
  sv.mbox_kernel = nb > MB_NBMAX || sv.force_big ? sssp_mbox_kernel<true> : sssp_mbox_kernel<false>;
  sv.mbox_head_kernel = nb > MB_NBMAX || sv.force_big ? sssp_mbox_kernel<true, true> : sssp_mbox_kernel<false, true>;
  sv.bounded_on = false;  // (shortest_path_n1_begin switches it on)
  sv.mb_dyn = (size_t)nb * mv.stg * sizeof(uint2) + 3u * (size_t)nb * sizeof(uint32_t);
  static OncePerDevice lds_once;
  raise_dynamic_lds(lds_once, ctx->device, (int)MB_DYN_BUDGET, {(const void*)sssp_mbox_kernel<false>, (const void*)sssp_mbox_kernel<true>,
                                                                      (const void*)sssp_mbox_kernel<false, true>, (const void*)sssp_mbox_kernel<true, true>});
  // A mailbox sweep costs its ~10 us chain of dependent trips whatever it expands, up to ~256 states per block: the
  // threshold moves on as soon as the near set is below 1/16 of the states (measured, tools/param_sweep.py: 4096 ->
  // 65536 at 1M / 2M states is 0.407 -> 0.386 and 0.817 -> 0.741 ms; at 300 k states 16384 is the best)
  if (!sv.kn.near_low) sv.near_low = std::min<uint32_t>(65536u, std::max<uint32_t>(4096u, n / 16u));
  // hand-over to NARROW launches when the near set plus everything waiting beyond the threshold is this small
  sv.narrow_t = sv.kn.narrow.value_or(8192u);
  sv.hint_mask = f->last_hint_mask.load(std::memory_order_relaxed);
  if (sv.kn.hint) sv.hint_mask = *sv.kn.hint ? ~0ull : 0ull;  // experiments: all / no launches gated
  mv.dbg = nullptr;
  if (sv.kn.mbox_trace) {
    sv.mb_dbg = DBuf<unsigned long long>(*ctx->pool, (size_t)MB_DBG_SWEEPS * nb * 16);
    HIP_CHECK(hipMemsetAsync(sv.mb_dbg.p, 0, (size_t)MB_DBG_SWEEPS * nb * 16 * 8, ctx->stream));
    mv.dbg = sv.mb_dbg.p;
  }
}

// The resident launch of a mailbox solve that holds the lease and the buffers for one (`want_res`): ResView, its staging
// depth and its schedule.  Every block needs a CU of its own for the whole launch (1024 threads x 128 registers and ~150 KB
// of LDS fill one), so the grid must fit the device: lease_resident saw to that.
void bind_resident(wfst_ctx* ctx, const wfst_fst* f, Solve& sv, bool want_res) {
  const uint32_t n = f->n_states, nb = sv.plan->nb;
  sv.resident = false;
  sv.rv = ResView{};
  sv.res_dyn = 0;
  // (plan_mailbox checked resident_staging already; what is left here is WFST_SSSP_STG, which may set fewer than the 4 slots a
  // resident launch needs — the tests' way into the one-launch-per-level path of 4096-state blocks)
  uint32_t stg = want_res && !sv.force_big ? resident_staging(*sv.plan) : 0u;
  if (sv.kn.stg) stg = std::min<uint32_t>(stg, *sv.kn.stg);
  if (stg < 4) {
    if (sv.log == 13) throw Error("shortest_path: internal error (the 8192-state plan without a resident launch)");
    rearm_prove(ctx, sv);
    sv.rs_msgs.reset();
    sv.rs_abort.reset();
    sv.lease.release();
    return;
  }
  sv.resident = true;
  sv.res_kernel = sv.log == 13 ? sssp_mbox_resident_kernel<13> : sssp_mbox_resident_kernel<12>;
  MboxView& mv = sv.mv;
  mv.stg = stg;
  {
    // states per lane group in the widest round: 4, unless such a round (4 x 16 x (64 / lps) states) would send more than
    // ~0.8 of the staging slots' worth to an average destination — what overflows leaves as 8-byte stores of its own
    // (2M states, 8192-state blocks, 21 slots: 454 us with 4, 432 with 2)
    const uint32_t lps = sv.plan->lps, g = 16u * (64u / lps);
    const double per_dest = 4.0 * g * ((double)f->n_arcs / (double)n) / (double)nb;
    const uint32_t umax = sv.kn.umax ? (uint32_t)*sv.kn.umax : per_dest <= 0.8 * mv.stg ? 4u : 2u;
    sv.res_lps_umax = lps | (umax << 8);
  }
  sv.mb_dyn = (size_t)nb * mv.stg * sizeof(uint2) + 3u * (size_t)nb * sizeof(uint32_t);
  sv.res_dyn = res_lds_bytes(sv.log, nb, mv.stg);
  ResView& rv = sv.rv;
  rv.msgs[0] = sv.rs_msgs.p;
  rv.msgs[1] = sv.rs_msgs.p + sv.plan->res_units;
  rv.roffh = sv.plan->roffh.p;
  rv.roffh_t = sv.plan->roffh_t.p;
  rv.abort = sv.rs_abort.p;
  rv.bytes = (uint32_t)(sv.plan->res_units * sizeof(uint2));
  rv.tlim_ticks = 2000000u;  // 20 ms of wall_clock64
  if (sv.kn.res_tlim_us) rv.tlim_ticks = (uint32_t)std::min<long long>(4000000000ll, *sv.kn.res_tlim_us * 100ll);
  sv.res_max_levels = sv.kn.res_levels.value_or(RS_LEVEL_CAP);
  rv.trace = nullptr;
  if (sv.kn.res_trace) {
    sv.rs_trace = DBuf<unsigned long long>(*ctx->pool, (size_t)RS_TRACE_LEVELS * nb * 4);
    HIP_CHECK(hipMemsetAsync(sv.rs_trace.p, 0, (size_t)RS_TRACE_LEVELS * nb * 4 * 8, ctx->stream));
    rv.trace = sv.rs_trace.p;
  }
  // a resident level costs ~7 us when thin (a launch per level: ~10): the band's tail is cut a little later and the
  // hand-over to the NARROW launch comes a little earlier (measured on C3: 298.8 -> 289.5 us per solve)
  if (!sv.kn.near_low) sv.near_low = std::min<uint32_t>(65536u, std::max<uint32_t>(4096u, n / 32u));
  // (what the NARROW launch can hold is ~48 - 96 entries per workgroup: handing it more per workgroup than that sends the
  // search back and forth between the modes — 150 k states, 37 blocks, threshold 16 384: 7.6 launches and 0.55 ms per
  // query from random sources; with 64 per block 3 launches and 0.40 ms: tools/varied_sources.py)
  if (!sv.kn.narrow) sv.narrow_t = std::min<uint32_t>(16384u, std::max<uint32_t>(1024u, nb * (sv.log == 13 ? 128u : 64u)));
  static OncePerDevice lds_once;
  raise_dynamic_lds(lds_once, ctx->device, (int)RES_LDS_BYTES,
                    {(const void*)sssp_mbox_resident_kernel<12>, (const void*)sssp_mbox_resident_kernel<13>});
}

// Binned levels (sssp_binned.h): the dense levels of the solve as owner-computes passes, chosen per level on the device.
// Parity-green and measured (profiles/r05*): NOT faster than the atomic sweeps on MI355X at any size tried (5M states:
// 2.9 vs 2.4 ms; a binned level costs ~50 us + 25 ps per arc against 14.5 ps per arc + 78 ps per atomic), so it is an
// option, not the default.  WFST_SSSP_BINNED=1: on wherever the message format allows.
void bind_binned(wfst_ctx* ctx, const wfst_fst* f, Solve& sv) {
  const uint32_t n = f->n_states;
  sv.binned = false;
  sv.bplan.reset();
  if (!(bin_eligible(f) && sv.delta < INF && sv.kn.binned >= 1 && ctx->n_cus > 0)) return;
  const uint32_t logd = n <= (BN_MAXBINS << 13) && !sv.kn.bin_log14 ? 13u : 14u;
  try {  // (a slot per arc and the region tables come from the pool: on a tight pool the atomic sweeps run every level)
    sv.bplan = bin_plan(ctx, f, logd);
    const BinPlan& bp = *sv.bplan;
    if (bp.slots == 0 || bp.slots >= 0xFFFF0000ull) throw Error("binned levels: region table out of range");
    sv.bn_msgs = DBuf<uint2>(*ctx->pool, (size_t)bp.slots);
    sv.bn_cnt = DBuf<uint32_t>(*ctx->pool, (size_t)bp.nbin * bp.G);
    HIP_CHECK(hipMemsetAsync(sv.bn_cnt.p, 0, (size_t)bp.nbin * bp.G * sizeof(uint32_t), ctx->stream));
    BinView& bv = sv.bv;
    bv.roff = bp.roff.p;
    bv.roff_t = bp.roff_t.p;
    bv.msgs = sv.bn_msgs.p;
    bv.cnt = sv.bn_cnt.p;
    bv.nbin = bp.nbin;
    bv.G = bp.G;
    bv.sg = bp.sg;
    bv.hop_cap = 1u << (32u - logd);
    if (sv.kn.bin_hopcap) bv.hop_cap = std::max<uint32_t>(1u, std::min<uint32_t>(bv.hop_cap, *sv.kn.bin_hopcap));
    sv.bn_dyn_expand = bin_expand_lds(bp.nbin);
    sv.bn_dyn_apply = bin_apply_lds(logd);
    sv.bin_expand_kernel = logd == 14 ? sssp_bin_expand_kernel<14> : sssp_bin_expand_kernel<13>;
    sv.bin_apply_kernel = logd == 14 ? sssp_bin_apply_kernel<14> : sssp_bin_apply_kernel<13>;
    static OncePerDevice lds_once;
    raise_dynamic_lds(lds_once, ctx->device, BN_LDS_MAX,
                      {(const void*)sssp_bin_expand_kernel<13>, (const void*)sssp_bin_expand_kernel<14>,
                       (const void*)sssp_bin_apply_kernel<13>, (const void*)sssp_bin_apply_kernel<14>});
    // a binned level costs two launches and the keys of every bin that receives anything (12 B per state when all do):
    // it pays from a frontier of ~1/64 of the states (measured, profiles/r05*: the atomic sweep relaxes ~10 G arcs/s there)
    sv.dense_low = std::max<uint32_t>(16384u, n / 64u);
    if (sv.kn.dense_low) sv.dense_low = (uint32_t)std::min<long long>(0xFFFFFFFEll, *sv.kn.dense_low);
    sv.binned = true;
  } catch (const Error&) {
    (void)hipGetLastError();  // (a refused allocation must not surface at the next launch check)
    sv.bplan.reset();
    sv.bn_msgs.reset();
    sv.bn_cnt.reset();
  }
}

// relax_setup allocates and initialises the state of a solve (keys, frontier flags, control block) and fixes its schedule parameters
void relax_setup_held(wfst_ctx* ctx, const wfst_fst* f, Solve& sv, RearmHeld& held) {
  const Knobs& kn = sv.kn;
  const uint32_t n = f->n_states;
  DevicePool& pool = *ctx->pool;
  held.take_or_alloc(sv, sv.key, RH_KEY, n);
  sv.shadow = DBuf<uint32_t>(pool, n);
  const size_t n_pad = ((size_t)n + 15) & ~(size_t)15;
  sv.flags = DBuf<uint8_t>(pool, 2 * n_pad);
  held.take_or_alloc(sv, sv.improved, RH_IMPROVED, IMP_RING);
  held.take_or_alloc(sv, sv.ctl, RH_CTL, 1);
  hipStream_t st = ctx->stream;
  sv.fl[0] = sv.flags.p;
  sv.fl[1] = sv.flags.p + n_pad;
  sv.blocks = std::max<uint32_t>(1u, std::min<uint32_t>((uint32_t)ctx->n_cus * 8, (n + 255) / 256));
  sv.delta = band_from_mean_weight(f, kn);
  sv.near_low = kn.near_low.value_or(4096u);  // activations below which a sweep is launch-latency bound anyway
  const float tau0_mult = kn.tau0_mult > 0.0f ? kn.tau0_mult : 1.0f;  // first band = tau0_mult x delta
  static_assert(sizeof(Ctl) % 4 == 0, "Ctl is cleared word by word");
  // mailbox sweeps where they pay: branching graphs (the near-far case) whose state ids fit the message format
  // ... and few enough blocks that the per-pair regions still hold runs of messages: measured on MI355X (fan-out 10), the
  // mailbox launches win at 1M and 2M states (0.41 vs 0.50 ms, 0.84 vs 0.89), tie at 3M and lose at 5M (3.2 vs 2.4 ms: a
  // region then receives ~3 messages per sweep, and 1221 workgroups take five turns on 256 CUs).  Beyond MB_NB_DEFAULT
  // blocks the atomic sweeps stay the default; WFST_SSSP_MAILBOX=1 still selects the mailbox kernel up to 8M states.
  int mbox_mode = sv.delta < INF && mbox_eligible(f) && ((n + MB_B - 1) >> MB_LOG) <= MB_NB_DEFAULT ? 1 : 0;
  if (kn.mailbox) mbox_mode = mbox_eligible(f) ? *kn.mailbox : 0;
  sv.log = 12;
  sv.lease.release();
  bool want_res = mbox_mode >= 1 && lease_resident(ctx, n, sv);
  if (mbox_mode >= 1) want_res = plan_mailbox(ctx, f, sv, want_res, held);
  if (sv.mbox) {
    sv.delta = band_from_cheapest_arcs(f, *sv.plan, sv.delta, kn);
    bind_mailbox(ctx, f, sv);
    bind_resident(ctx, f, sv, want_res);
  }
  sv.tau0 = sv.delta * tau0_mult;
  uint32_t tau0_bits;
  std::memcpy(&tau0_bits, &sv.tau0, sizeof(tau0_bits));
  if (held.rec.plan) {  // parked scratch was taken: it is this solve's initial state if the solve is the one it was cleaned for
    const RearmRecord& r = held.rec;
    const bool eligible = sv.mbox && sv.log == 12 && sv.narrow_t != 0;
    if (eligible && !held.left() && sv.plan == r.plan && r.log == sv.log && r.resident == sv.resident && r.stg == sv.mv.stg && r.narrow &&
        r.tau0_bits == tau0_bits) {
      sv.armed = true;
      sv.rearm_why = nullptr;
      sv.rearm_stops = r.stops;
      sv.rearm_epoch = r.epoch;
      ctx->rearm_stats.adopted += 1;
    } else {  // (the blocks this solve took are its own now: whatever it queues comes behind the re-arm launch on the stream)
      sv.rearm_why = eligible ? "knobs differ" : "not eligible";
      ctx->rearm_stats.dropped += 1;
      held.settle();
    }
  }
  if (sv.mbox) {
    if (!sv.armed) {
      const auto setup_kernel = sv.log == 13 ? sssp_mbox_setup_kernel<13> : sssp_mbox_setup_kernel<12>;
      setup_kernel<<<sv.blocks, 256, 0, st>>>(sv.key.p, sv.mv, sv.improved.p, sv.ctl.p, f->dev.offsets, n, (uint32_t)f->start,
                                              sv.tau0, sv.narrow_t, sv.rv.msgs[0], sv.rv.msgs[1], sv.rv.roffh, sv.rv.abort);
    }
  } else {
    bind_binned(ctx, f, sv);
    sssp_setup_kernel<<<sv.blocks, 256, 0, st>>>(sv.key.p, sv.shadow.p, (uint32_t*)sv.flags.p, (uint32_t)(2 * n_pad / 4),
                                                 sv.improved.p, sv.ctl.p, n, (uint32_t)f->start, sv.tau0);
  }
  HIP_CHECK(hipGetLastError());
  ctx->stats.relax_kernel = sv.mbox ? (sv.resident ? 2u : 1u) : (sv.binned ? 3u : 0u);
  sv.sweep_cap = 4ull * n + 64;
  if (kn.chase_cap) sv.chase_cap = *kn.chase_cap;
  if (kn.chase_rounds) sv.chase_rounds = *kn.chase_rounds;
  if (kn.chase_low) sv.chase_low = *kn.chase_low;
}
void relax_setup(wfst_ctx* ctx, const wfst_fst* f, Solve& sv, const Knobs* kn = nullptr /*the caller has read them already*/) {
  sv.kn = kn ? *kn : read_knobs();
  sv.armed = false;
  sv.rearm_stops = 0;
  sv.rearm_unproven = false;
  RearmHeld held(ctx);
  sv.rearm_why = rearm_take(ctx, f, sv.kn, held);
  try {
    relax_setup_held(ctx, f, sv, held);
  } catch (...) {
    rearm_prove(ctx, sv);  // (the caller lets go of sv's buffers)
    throw;
  }
  // (from here on a buffer of the solve is released only after the solve's own launches, which come behind the re-arm launch)
  sv.rearm_unproven = false;
}

// Queues the sweeps of a solve in batches and finds the sweep that changed nothing.  start() queues the first batch and
// returns; finish() waits for it and continues until convergence (see the launch schedule in DESIGN.md §3.2).
struct SweepBatch {
  uint32_t first, count;
  int which;
};
struct SweepDriver {
  wfst_ctx* ctx = nullptr;
  const wfst_fst* f = nullptr;
  Solve* sv = nullptr;
  uint32_t n = 0;
  uint32_t* h_imp = nullptr;
  uint32_t next_sweep = 0, first_count = 8, sweeps_done = 0;
  bool predicted = false;  // the first batch is expected to cover the whole solve: nothing is queued behind it
  bool extended = false;   // more than the first batch was needed
  hipEvent_t evs[2] = {nullptr, nullptr};
  SweepBatch cur{};

  void init(wfst_ctx* c, const wfst_fst* fst, Solve* s) {
    ctx = c;
    f = fst;
    sv = s;
    n = fst->n_states;
    h_imp = (uint32_t*)ctx->pinned_flags.get(3 * IMP_RING * sizeof(uint32_t));
    // A batch boundary costs ~14 us of idle GPU (profiles/r01d), so the FIRST batch of a solve is sized to what the
    // previous solve of this FST needed (+1 sweep to see the quiet one, rounded up to an even count; batch sizes stay
    // even because the flag parity of a sweep inside a batch is static).
    // The mailbox sweeps repeat themselves closely but not exactly (a state expanded while other waves of the same launch
    // improve it sends its old or its new key; NARROW launches follow discoveries in whatever order the atomics land), so a
    // repeated query gets the launches the last one needed, the quiet one included, plus ONE: a gated idle launch is ~3 us,
    // a second batch is a host round trip and a re-run of the fused tail.
    // (the margin is dropped once three solves in a row needed the same count: wfst_fst::stable_sweeps)
    const uint32_t last_sweeps = f->last_sweeps.load(std::memory_order_relaxed);
    // (wfst_fst_set_start resets the count of stable solves: a query from another source than the last one gets the spare launch back)
    const uint32_t margin = f->stable_sweeps.load(std::memory_order_relaxed) >= 3 ? 0u : 1u;
    if (last_sweeps) first_count = std::min<uint32_t>(MAX_BATCH, sv->mbox ? last_sweeps + margin : ((last_sweeps + 1 + 1) & ~1u));
    predicted = last_sweeps != 0 && (sv->mbox ? last_sweeps <= first_count : last_sweeps < first_count);
    evs[0] = ctx->ev0;
    evs[1] = ctx->ev1;
  }

  // `defer_advance`: the caller queues a kernel behind the batch that closes it (sssp_tail_kernel mirrors the flags and
  // advances the base itself); no event is recorded (wait_first_batch)
  SweepBatch enqueue_batch(hipEvent_t ev, bool defer_advance = false) {
    hipStream_t st = ctx->stream;
    // after the first batch: constant small batches while the solve is shallow, larger ones for deep lattices
    SweepBatch b{next_sweep, 8u, 1};
    if (next_sweep == 0) b = SweepBatch{0u, first_count, 0};
    else if (next_sweep >= 64) b = SweepBatch{next_sweep, MAX_BATCH, 2};
    // plain launches: the GPU starts on the first sweep while the host is still queueing the rest (the same batch as a HIP
    // graph was measured and dropped: a replay of N nodes only starts after ~2.7 us x N of host-side work, 89 us for 32
    // sweeps, profiles/r01g)
    const bool time_chain = ctx->chain_timing && b.first == 0;
    if (time_chain) HIP_CHECK(hipEventRecord(ctx->ev_chain[0], st));
    for (uint32_t j = 0; j < b.count; ++j) launch_sweep(f, *sv, n, st, j, j, b.first + j, 0u);
    if (time_chain) HIP_CHECK(hipEventRecord(ctx->ev_chain[1], st));
    if (!defer_advance) sssp_advance_kernel<<<1, 64, 0, st>>>(sv->ctl.p, sv->improved.p, b.count, h_imp + b.which * IMP_RING);
    HIP_CHECK(hipGetLastError());
    if (!defer_advance) HIP_CHECK(hipEventRecord(ev, st));
    next_sweep += b.count;
    return b;
  }
  uint32_t* host_flags(const SweepBatch& b) const { return h_imp + b.which * IMP_RING; }

  bool aborted = false;    // a resident launch raised FLAG_RES_ABORT
  bool bounded = false;    // a bounded head raised FLAG_NARROW_BOUNDED: the keys above its B are not the fixed point
  uint64_t seen_busy = 0;  // bit k: launch k was a busy WIDE sweep (flag value 1 + MODE_WIDE)
  bool scan_flags(const SweepBatch& b) {  // true when a sweep of the batch changed nothing
    const uint32_t* hf = h_imp + b.which * IMP_RING;
    for (uint32_t k = 0; k < b.count; ++k) {
      sweeps_done = b.first + k + 1;
      const uint32_t v = hf[(b.first + k) % IMP_RING];
      if (!v) return true;
      if (v == FLAG_RES_ABORT) {  // a resident launch gave up waiting for its own workgroups: the caller solves again without
        aborted = true;
        return true;
      }
      if (v == FLAG_NARROW_CLEAN) return true;  // a NARROW launch that left nothing anywhere: the fixed point, certified
      if (v == FLAG_NARROW_BOUNDED) {  // the head settled the best final state: the path is decided, the solve is over
        bounded = true;
        return true;
      }
      // (WIDE and COLLECT launches have every block awake and loading its keys: no gate next time)
      if ((v == 1u + MODE_WIDE || v == 1u + MODE_COLLECT) && b.first + k < 64) seen_busy |= 1ull << (b.first + k);
    }
    return false;
  }
  // which launches of the next solve of this FST may skip the gate (they were busy WIDE sweeps this time)
  uint64_t hint_mask() const { return ~seen_busy; }

  void start(bool defer_advance = false) { cur = enqueue_batch(evs[0], defer_advance); }

  // The fused tail's ticket in pinned memory (wfst_sp_job::h_tail->done), when the first batch ends with one: the host waits
  // for that word — every result of the launch chain is in host memory before it — and falls back to the stream.
  const volatile uint32_t* done_word = nullptr;
  uint32_t done_ticket = 0;
  bool done_seen = false;  // the ticket arrived: nothing of this job is still running on the stream
  void wait_first_batch() {
    if (done_word && !sv->kn.event_wait) {
      const auto t0 = std::chrono::steady_clock::now();
      for (uint32_t spins = 0;; ++spins) {
        if (*done_word == done_ticket) {
          std::atomic_thread_fence(std::memory_order_acquire);
          done_seen = true;
          return;
        }
        cpu_relax();
        if ((spins & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;  // (a long solve: sleep on the event)
      }
    }
    // (the batch that ends with the fused tail records no event — a host call in front of whatever the caller queues next,
    // for a wait that is taken only after 2 ms of spinning or under WFST_SSSP_EVENT_WAIT: it waits for the stream instead)
    if (done_word) HIP_CHECK(hipStreamSynchronize(ctx->stream));
    else HIP_CHECK(hipEventSynchronize(evs[0]));
  }

  void finish() {
    int which = 0;
    bool done = false;
    if (predicted) {  // expected to finish inside the first batch: no idle sweeps were queued behind it
      wait_first_batch();
      done = scan_flags(cur);
      if (!done) {
        extended = true;
        cur = enqueue_batch(evs[0]);
      }
    }
    while (!done) {
      if (next_sweep > sv->sweep_cap) throw Error("shortest_path: relaxation did not converge (negative-weight cycle?)");
      // keep the device busy while the host inspects `cur`: the next batch is enqueued first
      const SweepBatch nxt = enqueue_batch(evs[which ^ 1]);
      extended = true;
      HIP_CHECK(hipEventSynchronize(evs[which]));
      done = scan_flags(cur);
      cur = nxt;
      which ^= 1;
    }
  }
};

// tuning aids: the phase stamps of a mailbox solve go to the file named by WFST_SSSP_MBOX_TRACE (u64 [64][nb][16]), the level
// stamps of its resident launches to the one named by WFST_SSSP_RES_TRACE (u64 [64][nb][4])
void dump_trace(wfst_ctx* ctx, const char* path, const unsigned long long* stamps, uint32_t rows, uint32_t nb, uint32_t width) {
  if (!stamps || !path) return;
  std::vector<unsigned long long> h((size_t)rows * nb * width);
  HIP_CHECK(hipMemcpyAsync(h.data(), stamps, h.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  if (FILE* fp = std::fopen(path, "wb")) {
    const uint32_t hdr[2] = {rows, nb};
    std::fwrite(hdr, 4, 2, fp);
    std::fwrite(h.data(), 8, h.size(), fp);
    std::fclose(fp);
  }
}

// the book-keeping of a solve that reached its fixed point after `sweeps` launches
// (`bounded`: a bounded head ended it — its one launch says nothing about what a full solve of this FST needs)
void record_solve(wfst_ctx* ctx, const wfst_fst* f, Solve& sv, uint32_t sweeps, bool bounded = false) {
  sv.lease.release();
  sv.sweeps = sweeps;
  ctx->stats.sweeps = sweeps;
  if (!bounded) note_sweeps(f, sweeps);
  if (bounded) f->bounded_streak.fetch_add(1, std::memory_order_relaxed);
  else if (sv.bounded_on) f->bounded_streak.store(0, std::memory_order_relaxed);
  // (a head that stopped leaves its resident launch at entry; a solve of one launch per level never holds whole compute units)
  resident_work_of(ctx->device).store(sv.resident && !bounded ? 1 : 0, std::memory_order_relaxed);
  if (sv.mbox) dump_trace(ctx, sv.kn.mbox_trace, sv.mb_dbg.p, MB_DBG_SWEEPS, sv.mv.nb, 16);
  if (sv.resident) dump_trace(ctx, sv.kn.res_trace, sv.rs_trace.p, RS_TRACE_LEVELS, sv.mv.nb, 4);
}

// The end of a solve whose first batch `drv` has queued: the rest of the sweeps, then the book-keeping.  false = a resident
// launch gave up waiting (its grid was not resident as a whole) and nothing of the solve stands: the caller solves again,
// inside a ResidentHold, with one launch per level.
bool finish_solve(wfst_ctx* ctx, const wfst_fst* f, Solve& sv, SweepDriver& drv) {
  drv.finish();
  if (drv.aborted) {
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    ctx->resident_aborted(sv.kn.res_retry_ms);
    ctx->stats.resident_aborts += 1;
    sv.lease.release();
    return false;
  }
  if (sv.resident) ctx->resident_completed();
  if (!drv.bounded) f->last_hint_mask.store(drv.hint_mask(), std::memory_order_relaxed);
  record_solve(ctx, f, sv, drv.sweeps_done, drv.bounded);
  return true;
}
struct ResidentHold {  // the repeat of a solve whose resident launch gave up: never a resident one (wfst_ctx::resident_allowed)
  wfst_ctx* ctx;
  explicit ResidentHold(wfst_ctx* c) : ctx(c) { ctx->resident_hold = true; }
  ~ResidentHold() { ctx->resident_hold = false; }
};

// Runs the relaxation to its fixed point. f must have a device copy and a start state.
void run_relaxation(wfst_ctx* ctx, const wfst_fst* f, Solve& sv) {
  relax_setup(ctx, f, sv);
  const uint32_t n = f->n_states;
  hipStream_t st = ctx->stream;
  uint8_t* const* fl = sv.fl;
  const uint32_t blocks = sv.blocks;
  const uint64_t sweep_cap = sv.sweep_cap;
  ctx->stats.sweeps = 0;

  uint32_t sweeps_done = 0;
  if (ctx->profiling) {
    // one sweep at a time, bracketed by events; a counting kernel (outside the events) sizes the frontier
    uint32_t* h_imp = (uint32_t*)ctx->pinned.get(64 + sizeof(Ctl));
    Ctl* h_ctl = (Ctl*)((char*)h_imp + 64);
    ctx->sweep_trace.clear();
    uint64_t prev_arcs = 0, prev_states = 0;
    auto shard_sum = [](const unsigned long long* v) {
      uint64_t t = 0;
      for (uint32_t j = 0; j < PROF_SHARDS; ++j) t += v[j * PROF_STRIDE];
      return t;
    };
    for (uint32_t k = 0;; ++k) {
      if (k > sweep_cap) throw Error("shortest_path: relaxation did not converge (negative-weight cycle?)");
      sssp_nop_kernel<<<blocks, 256, 0, st>>>(fl[k & 1u], n, sv.improved.p);
      HIP_CHECK(hipEventRecord(ctx->ev0, st));
      launch_sweep(f, sv, n, st, k, 0u, k, sv.kn.count_atomics ? 2u : 1u);  // counts the states / arcs it relaxes
      HIP_CHECK(hipEventRecord(ctx->ev1, st));
      sssp_advance_kernel<<<1, 64, 0, st>>>(sv.ctl.p, sv.improved.p, 1u, nullptr);
      HIP_CHECK(hipMemcpyAsync(h_imp, sv.improved.p + (k % IMP_RING), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
      HIP_CHECK(hipMemcpyAsync(h_ctl, sv.ctl.p, sizeof(Ctl), hipMemcpyDeviceToHost, st));
      HIP_CHECK(hipStreamSynchronize(st));
      float ms = 0;
      HIP_CHECK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
      const uint64_t arcs = shard_sum(h_ctl->arcs), states = shard_sum(h_ctl->states);
      ctx->sweep_trace.push_back({(double)ms, arcs - prev_arcs, states - prev_states, (sv.mbox || sv.binned) ? h_ctl->mode[k % RING] : 0u});
      prev_arcs = arcs;
      prev_states = states;
      ctx->stats.relax_ms += ms;
      ctx->stats.relax_launches += 1;
      sweeps_done = k + 1;
      if (!h_imp[0]) break;
    }
    ctx->stats.relax_arcs += prev_arcs;
    ctx->stats.relax_states += prev_states;
    record_solve(ctx, f, sv, sweeps_done);
  } else {
    SweepDriver drv;
    drv.init(ctx, f, &sv);
    drv.start();
    if (!finish_solve(ctx, f, sv, drv)) {  // a resident launch gave up waiting: one launch per level
      ResidentHold hold(ctx);
      run_relaxation(ctx, f, sv);
    }
  }
}

// The order in which the reference relaxes the states of an acyclic FST (queues/auto_queue.rs:23-99): state order when the
// TOP_SORTED bit is set, else the topological order of dfs_visit (dfs_visit.rs:97-187: root = start, then 0, 1, 2, ...; arcs
// in stored order) — TopOrderQueue from TopOrderVisitor (top_sort.rs:12-61) when the ACYCLIC bit is known, from the SCC
// numbering otherwise (scc_visitors.rs:173-179): both are the reverse finishing order.  false when the reference would use
// another discipline: LIFO (unweighted input), or an SCC queue (the input has a cycle).
bool reference_top_rank(const wfst_fst* f, std::vector<uint32_t>& rank) {
  const uint32_t n = f->n_states;
  if (f->start < 0 || n == 0) return false;
  ensure_host(f);
  const HostCsr& h = f->host;
  rank.resize(n);
  if (f->props & props::TOP_SORTED) {
    for (uint32_t s = 0; s < n; ++s) rank[s] = s;
    return true;
  }
  if (!(f->props & props::ACYCLIC)) {
    if (f->props & props::UNWEIGHTED) return false;  // LifoQueue
    bool unweighted = true;                          // scc_queue_type's scan
    for (const wfst_tr& a : h.arcs)
      if (weighted(a.weight)) {
        unweighted = false;
        break;
      }
    if (unweighted) return false;
  }
  enum : uint8_t { White, Grey, Black };
  std::vector<uint8_t> color(n, White);
  std::vector<std::pair<uint32_t, uint32_t>> stack;
  uint32_t finished = 0;
  uint32_t root = (uint32_t)f->start;
  while (root < n) {
    color[root] = Grey;
    stack.push_back({root, h.offsets[root]});
    while (!stack.empty()) {
      const uint32_t s = stack.back().first;
      uint32_t& pos = stack.back().second;
      if (pos >= h.offsets[s + 1]) {
        color[s] = Black;
        rank[s] = n - 1 - finished++;
        stack.pop_back();
        continue;
      }
      const uint32_t t = h.arcs[pos++].nextstate;
      if (color[t] == White) {
        color[t] = Grey;
        stack.push_back({t, h.offsets[t]});
      } else if (color[t] == Grey) {
        return false;  // a cycle: the reference uses an SCC queue
      }
    }
    root = root == (uint32_t)f->start ? 0 : root + 1;
    while (root < n && color[root] != White) root++;
  }
  return true;
}

// shortest_path (nshortest = 1) with the reference's choice among tied optima, for an acyclic input whose relaxation order
// `rank` is known: distances on the GPU as always, then the final state and the predecessors by the rule above.
wfst_fst* shortest_path_reference_order(wfst_ctx* ctx, const wfst_fst* f, const std::vector<uint32_t>& rank) {
  const uint32_t n = f->n_states;
  hipStream_t st = ctx->stream;
  Solve sv;
  run_relaxation(ctx, f, sv);
  std::vector<uint32_t> r2s(n);
  for (uint32_t s = 0; s < n; ++s) r2s[rank[s]] = s;
  DBuf<uint32_t> d_rank(*ctx->pool, n), d_r2s(*ctx->pool, n);
  HIP_CHECK(hipMemcpyAsync(d_rank.p, rank.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
  HIP_CHECK(hipMemcpyAsync(d_r2s.p, r2s.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
  DBuf<unsigned long long> parent(*ctx->pool, n);
  DBuf<wfst_tr> out(*ctx->pool, n);
  HIP_CHECK(hipMemsetAsync(parent.p, 0xFF, (size_t)n * sizeof(unsigned long long), st));
  HIP_CHECK(hipMemsetAsync(&sv.ctl.p->best, 0xFF, sizeof(unsigned long long), st));
  HIP_CHECK(hipMemsetAsync(&sv.ctl.p->pad, 0, sizeof(uint32_t), st));
  sssp_final_ref_kernel<<<std::min<uint32_t>((n + 255) / 256, (uint32_t)ctx->n_cus * 4), 256, 0, st>>>(f->dev.finals, sv.key.p, d_rank.p, n,
                                                                                                          sv.ctl.p);
  const uint32_t blocks = std::min<uint32_t>((uint32_t)ctx->n_cus * 8, (uint32_t)(((uint64_t)n * GROUP + 255) / 256));
  sssp_parent_ref_kernel<<<blocks, 256, 0, st>>>(f->dev.offsets, f->dev.wn, sv.key.p, d_rank.p, parent.p, n);
  sssp_backtrace_ref_kernel<<<1, 64, 0, st>>>(f->dev.offsets, f->dev.arcs, f->dev.finals, parent.p, d_r2s.p, (uint32_t)f->start, sv.ctl.p,
                                              out.p, n);
  Ctl* hc = (Ctl*)ctx->pinned.get(sizeof(Ctl));
  HIP_CHECK(hipMemcpyAsync(hc, sv.ctl.p, sizeof(Ctl), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(st));
  if (hc->pad & 1u) throw Error("shortest_path: hop count overflow in the mailbox sweeps (internal error)");
  if (hc->pad & 4u) throw Error("shortest_path: no admissible predecessor on the path (internal error)");
  if (!hc->has_path) return make_path_fst(ctx, false, 0, INF, nullptr);
  const uint32_t len = hc->hops;
  const float final_weight = hc->final_weight;
  std::vector<wfst_tr> path(len);
  if (len) HIP_CHECK(hipMemcpy(path.data(), out.p, (size_t)len * sizeof(wfst_tr), hipMemcpyDeviceToHost));
  return make_path_fst(ctx, true, len, final_weight, path.data());
}

// What shortest_distance and shortest_distance_device share: the solve, then the keys as plain distances — left in
// `d_distance`, or, when that is null, copied to `h_distance` (and the hop counts to `h_hops`, unless null) — and the wait.
void solve_distances(wfst_ctx* ctx, const wfst_fst* f, float* d_distance, float* h_distance, uint32_t* h_hops) {
  const uint32_t n = f->n_states;
  hipStream_t st = ctx->stream;
  ensure_device(const_cast<wfst_fst*>(f));
  Solve sv;
  run_relaxation(ctx, f, sv);
  DBuf<float> d;
  DBuf<uint32_t> hh;
  if (!d_distance) {  // (from the pool AFTER the solve: the solve's buffers get the blocks they had last time, api.cpp)
    d = DBuf<float>(*ctx->pool, n);
    hh = DBuf<uint32_t>(*ctx->pool, n);
    d_distance = d.p;
  }
  sssp_export_kernel<<<(n + 255) / 256, 256, 0, st>>>(sv.key.p, d_distance, h_hops ? hh.p : nullptr, n);
  HIP_CHECK(hipGetLastError());
  if (h_distance) HIP_CHECK(hipMemcpyAsync(h_distance, d.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, st));
  if (h_hops) HIP_CHECK(hipMemcpyAsync(h_hops, hh.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
}

}  // namespace

void shortest_distance(wfst_ctx* ctx, const wfst_fst* f, float* distance, uint32_t* hops) {
  const uint32_t n = f->n_states;
  if (f->start < 0 || n == 0) {
    for (uint32_t i = 0; i < n; ++i) {
      distance[i] = INF;
      if (hops) hops[i] = 0xFFFFFFFFu;
    }
    return;
  }
  solve_distances(ctx, f, nullptr, distance, hops);
}

// the same distances left in HBM (d_distance[n_states], +inf = unreachable) for device consumers (push.hip); f must have a
// start state
void shortest_distance_device(wfst_ctx* ctx, const wfst_fst* f, float* d_distance) {
  if (f->start < 0 || f->n_states == 0) throw Error("shortest_distance_device: no start state");
  solve_distances(ctx, f, d_distance, nullptr, nullptr);
}

// Transpose of f (in-arcs as {source, position}); built the SECOND time shortest_path sees the same large FST — a one-shot
// query keeps the parent pass, a resident transducer that is queried again pays the build once, inside its second query:
// ~0.3 ms for 10 M arcs through the mailbox plan (rev_bucket_kernel / rev_place_kernel), ~1.2 ms by the two atomic passes for
// FSTs without a plan.  (Building it on a second stream beside the FIRST query was measured: that query's resident launch
// waits for the compute units the build holds — 0.65 -> 1.8 ms, and a one-shot query pays for a transpose it never uses.)
// `force`: the caller needs the in-arcs of the path's states now (tie order 1 on a cyclic input).
namespace {
constexpr uint32_t FINAL_LIST_MAX = 65536;  // entries; and at most one state in eight may be final

__global__ void __launch_bounds__(256) final_flag_kernel(const float* __restrict__ finals, uint32_t n, uint32_t* __restrict__ flag) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s <= n) flag[s] = s < n && finals[s] < INF ? 1u : 0u;  // (n + 1 entries: the scan's last output is the count)
}
__global__ void __launch_bounds__(256) final_list_kernel(const float* __restrict__ finals, uint32_t n, const uint32_t* __restrict__ pos,
                                                        uint2* __restrict__ list, uint32_t cap) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const float fw = finals[s];
  if (fw < INF && pos[s] < cap) list[pos[s]] = make_uint2(s, __float_as_uint(fw));
}

// The list of final states of f (RevCsr::fin), built with the transpose: sssp_tail_kernel then reads a few thousand pairs
// instead of n final weights in every query.
void final_list_build(wfst_ctx* ctx, const wfst_fst* f, DevicePool& owner_pool, RevCsr& r) {
  const uint32_t n = f->n_states;
  hipStream_t st = ctx->stream;
  r.has_fin = false;
  r.fin_nonneg = false;
  r.n_fin = 0;
  if (n < 8 || n >= 0xFFFFFFF0u) return;
  DBuf<uint32_t> flag(*ctx->pool, (size_t)n + 1), pos(*ctx->pool, (size_t)n + 1);
  final_flag_kernel<<<n / 256 + 1, 256, 0, st>>>(f->dev.finals, n, flag.p);
  HIP_CHECK(hipGetLastError());
  const DBuf<uint8_t> scan_tmp = exclusive_scan_u32(ctx, flag.p, pos.p, (size_t)n + 1);
  const uint32_t n_fin = read_u32(ctx, pos.p + n);  // (synchronises the stream)
  if (n_fin > FINAL_LIST_MAX || n_fin > n / 8) return;
  r.fin = DBuf<uint2>(owner_pool, n_fin);
  if (n_fin) {
    final_list_kernel<<<(n + 255) / 256, 256, 0, st>>>(f->dev.finals, n, pos.p, r.fin.p, n_fin);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(st));  // flag / pos / scan_tmp are released here
  }
  // (once per handle: the early tail needs every final weight >= 0)
  r.fin_nonneg = true;
  if (n_fin) {
    std::vector<uint2> h(n_fin);
    HIP_CHECK(hipMemcpy(h.data(), r.fin.p, (size_t)n_fin * sizeof(uint2), hipMemcpyDeviceToHost));
    for (const uint2& e : h) {
      float w;
      std::memcpy(&w, &e.y, sizeof(w));
      if (!(w >= 0.0f)) r.fin_nonneg = false;
    }
  }
  r.n_fin = n_fin;
  r.has_fin = true;
}

void reverse_csr_build(wfst_ctx* ctx, const wfst_fst* f, RevCsr& r) {
  const uint32_t n = f->n_states;
  hipStream_t st = ctx->stream;
  DevicePool& owner_pool = f->owner_pool ? *f->owner_pool : *ctx->pool;  // cached with the handle: the owner's pool outlives it
  final_list_build(ctx, f, owner_pool, r);
  r.off = DBuf<uint32_t>(owner_pool, (size_t)n + 1);
  r.arc = DBuf<uint4>(owner_pool, f->n_arcs);
  const MboxPlan* plan = f->mbox ? f->mbox.get() : f->mbox13.get();  // (cache_mu is held by the caller)
  if (plan && !(std::getenv("WFST_SSSP_TRANSPOSE_PLAN") && std::atoi(std::getenv("WFST_SSSP_TRANSPOSE_PLAN")) == 0)) {
    DBuf<uint4> rec(*ctx->pool, f->n_arcs);  // one record per arc, bucketed by destination block
    const auto bucket_kernel = plan->log == 13 ? rev_bucket_kernel<13> : rev_bucket_kernel<12>;
    const auto place_kernel = plan->log == 13 ? rev_place_kernel<13> : rev_place_kernel<12>;
    bucket_kernel<<<plan->nb, 1024, plan->nb * sizeof(uint32_t), st>>>(f->dev.offsets, f->dev.wn, n, plan->nb, plan->roff_t.p, rec.p);
    place_kernel<<<plan->nb, 1024, 0, st>>>(plan->roff.p, plan->nb, n, rec.p, r.off.p, r.arc.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(st));  // rec is released here
    return;
  }
  DBuf<uint32_t> indeg(*ctx->pool, (size_t)n + 1), cursor(*ctx->pool, n);
  HIP_CHECK(hipMemsetAsync(indeg.p, 0, ((size_t)n + 1) * sizeof(uint32_t), st));
  const uint32_t blocks = (uint32_t)std::min<uint64_t>((f->n_arcs + 255) / 256, (uint64_t)ctx->n_cus * 8);
  rev_count_kernel<<<blocks, 256, 0, st>>>(f->dev.wn, f->n_arcs, indeg.p);
  // rev_off = exclusive scan of the in-degrees (n + 1 outputs: the extra zero input makes rev_off[n] the total)
  const DBuf<uint8_t> scan_tmp = exclusive_scan_u32(ctx, indeg.p, r.off.p, (size_t)n + 1);
  HIP_CHECK(hipMemcpyAsync(cursor.p, r.off.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  const uint32_t fblocks = std::min<uint32_t>((uint32_t)ctx->n_cus * 8, (uint32_t)(((uint64_t)n * GROUP + 255) / 256));
  rev_fill_kernel<<<fblocks, 256, 0, st>>>(f->dev.offsets, f->dev.wn, n, cursor.p, r.arc.p);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(st));  // indeg / cursor / scan_tmp are released here
}
}  // namespace

const RevCsr* reverse_csr(wfst_ctx* ctx, const wfst_fst* f, bool force = false) {
  std::lock_guard<std::mutex> lk(f->cache_mu);
  if (f->rev_dev) return f->rev_dev.get();
  if (f->n_arcs >= 0xFFFFFFFFull || f->n_arcs == 0) return nullptr;
  if (!force) {
    if (f->sp_queries.fetch_add(1) + 1 < 2 || f->n_arcs < (1u << 18)) return nullptr;
    if (const char* e = std::getenv("WFST_SSSP_TRANSPOSE")) if (std::atoi(e) == 0) return nullptr;
  }
  auto r = std::make_shared<RevCsr>();
  reverse_csr_build(ctx, f, *r);
  f->rev_dev = r;
  return r.get();
}

}  // namespace wfst

// One single-shortest-path solve split in two halves: begin queues the set-up, the first batch of sweeps and (when the
// solve is predicted to fit in that batch and the transpose is cached) the final-state search, the backtrace and the
// read-back of the path behind it, then returns; end waits, continues the sweeps if the prediction was short, and
// builds the output FST.  The synchronous shortest_path(nshortest = 1) is begin followed by end.
struct wfst_sp_job {
  wfst_ctx* ctx = nullptr;
  const wfst_fst* f = nullptr;
  bool trivial = false;      // no start state: the result is the empty FST (shortest_path.rs:185-187)
  wfst_fst* ready = nullptr;  // the result, already computed (reference tie order: a synchronous path)
  bool tail_queued = false;  // final / header / backtrace / read-back already queued behind the first batch
  bool fused_tail = false;   // ... as the one-launch sssp_tail_kernel (result header in h_tail instead of hc)
  wfst::Solve sv;
  wfst::SweepDriver drv;
  const wfst::RevCsr* rev = nullptr;
  wfst::Ctl* hc = nullptr;
  wfst_tr* h_path = nullptr;
  wfst::TailOut* h_tail = nullptr;  // header of the result, written by sssp_tail_kernel (transpose cached)
  uint32_t done_ticket = 0;         // what the fused tail writes into h_tail->done when everything else is in host memory
  bool need_unique = false;         // tie order 1 on an input the reference does not relax in a topological order: the result
                                    // is returned only when the optimum is unique (then it IS the reference's), KO otherwise
  // sssp_mbox_rearm_kernel is queued behind the fused tail and the solve's scratch has neither been parked nor waited for: the
  // ticket no longer means that nothing of this job is on the stream
  bool rearm_queued = false;
  // The solo query (sssp_solo.h): the whole job is ONE launch on the context's parked scratch, which is live (unparked) until end
  // parks it again; sv holds the knobs only, drv the ticket.  solo_why: why the route was not taken (WFST_SSSP_SOLO=2).
  bool solo = false;
  wfst::RearmRecord solo_rec;  // ... taken out of the context while the launch is in flight (whatever else runs on the context
                               // between begin and end finds nothing parked), put back by end
  const char* solo_why = nullptr;
  uint64_t epoch = 0;  // wfst_fst::sp_epoch as this query left it
#ifdef WFST_SP_HOST_TIMING
  std::chrono::steady_clock::time_point t_begin[4];
#endif
  ~wfst_sp_job() {
    if (rearm_queued && ctx) (void)hipStreamSynchronize(ctx->stream);  // (before sv's buffers go back to the pool)
    // a solo job that ends on an error between its launch and solo_restore (the ticket's stream-wait fall-back reporting a fault):
    // the six blocks it holds are live in the pool and nobody else knows them — back to the pool behind the stream
    if (solo_rec.plan && ctx) {
      (void)hipStreamSynchronize(ctx->stream);
      for (void* b : solo_rec.blk) ctx->pool->free(b);
      solo_rec.clear();
    }
  }
};

namespace wfst {
namespace {
constexpr uint32_t PATH_PINNED = 4096;  // arcs of the path written straight into pinned memory by the backtrace

// `adv`: the sweep batch this tail closes (enqueued with defer_advance), or null
void queue_tail(wfst_sp_job* j, const SweepBatch* adv = nullptr) {
  wfst_ctx* ctx = j->ctx;
  const wfst_fst* f = j->f;
  const uint32_t n = f->n_states;
  hipStream_t st = ctx->stream;
  Solve& sv = j->sv;
  if (j->rev && !sv.kn.split_tail) {  // one launch, header straight into pinned memory
    // over the handle's list of final states where it has one (WFST_SSSP_FINAL_LIST=0: the scan of `finals`; 2: the list or
    // an error, for tests): 4 entries per thread, ONE workgroup — no hand-over between workgroups — up to 4096 entries
    const bool listed = j->rev->has_fin && sv.kn.final_list != 0;
    const uint32_t blocks = listed ? std::max<uint32_t>(1u, std::min<uint32_t>(TAIL_LIST_BLOCKS, (j->rev->n_fin + 4095) / 4096))
                                   : std::min<uint32_t>(TAIL_BLOCKS, (n + 1023) / 1024);
    sssp_tail_kernel<<<blocks, 1024, 0, st>>>(
        f->dev.finals, sv.key.p, n, listed ? j->rev->fin.p : nullptr, listed ? j->rev->n_fin : 0u, sv.ctl.p, f->dev.offsets, f->dev.arcs,
        j->rev->off.p, j->rev->arc.p, j->h_path,
        PATH_PINNED, j->h_tail, sv.improved.p, adv ? adv->count : 0u, adv ? j->drv.host_flags(*adv) : nullptr, j->done_ticket,
        adv && sv.early_on ? 1u : 0u, adv && j->rearm_queued ? 1u : 0u);
    j->fused_tail = true;
    return;
  }
  if (adv) throw Error("shortest_path: internal error (deferred advance without the one-launch tail)");
  j->fused_tail = false;
  sssp_final_kernel<<<std::min<uint32_t>((n + 255) / 256, (uint32_t)ctx->n_cus * 4), 256, 0, st>>>(f->dev.finals, sv.key.p,
                                                                                                          n, sv.ctl.p);
  sssp_header_kernel<<<1, 1, 0, st>>>(f->dev.finals, sv.key.p, sv.ctl.p);
  if (j->rev)
    sssp_backtrace_rev_kernel<<<1, 64, 0, st>>>(f->dev.offsets, f->dev.arcs, sv.key.p, j->rev->off.p,
                                                j->rev->arc.p, sv.ctl.p, j->h_path, PATH_PINNED);
  HIP_CHECK(hipMemcpyAsync(j->hc, sv.ctl.p, sizeof(Ctl), hipMemcpyDeviceToHost, st));
}

// ---- host phases of begin / end by steady-clock stamps (build with -DWFST_SP_HOST_TIMING; printed by sp_host_timing_report).
// begin: entry -> checks and set-up done -> launches queued -> return; end: entry -> ticket seen -> scratch parked -> FST built.
#ifdef WFST_SP_HOST_TIMING
#define SP_STAMP(t) (t) = std::chrono::steady_clock::now()
// [route: 0 ordinary, 1 solo][the three phases of begin, then those of end]; per context, kept in this file so that the macro
// changes no struct another source sees (tools/build_variant.sh compiles this source alone with it)
struct SpHostTiming {
  uint64_t calls[2] = {0, 0};
  double sum_us[2][6] = {{0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}};
  double min_us[2][6] = {{1e30, 1e30, 1e30, 1e30, 1e30, 1e30}, {1e30, 1e30, 1e30, 1e30, 1e30, 1e30}};
};
void sp_timing_print(const SpHostTiming& s) {
  static const char* const route[2] = {"ordinary", "solo"};
  static const char* const phase[6] = {"begin: entry -> set-up done", "begin: -> launches queued", "begin: -> return",
                                       "end: entry -> ticket seen", "end: -> parked", "end: -> FST built"};
  for (int r = 0; r < 2; ++r) {
    const uint64_t c = s.calls[r];
    if (!c) continue;
    for (int k = 0; k < 6; ++k)
      std::fprintf(stderr, "sp_host_timing %-8s %-30s calls %8llu mean %8.2f us min %8.2f us\n", route[r], phase[k], (unsigned long long)c,
                   s.sum_us[r][k] / (double)c, s.min_us[r][k]);
  }
}
std::mutex sp_timing_mu;
std::map<const wfst_ctx*, SpHostTiming> sp_timing_of;
struct SpTimingAtExit {  // (a context that is never destroyed — an interpreter that exits with it — is reported here)
  ~SpTimingAtExit() {
    for (const auto& kv : sp_timing_of) sp_timing_print(kv.second);
  }
} sp_timing_at_exit;
void sp_timing_add(wfst_ctx* ctx, int route, int first, const std::chrono::steady_clock::time_point* t) {
  std::lock_guard<std::mutex> lk(sp_timing_mu);
  SpHostTiming& s = sp_timing_of[ctx];
  for (int k = 0; k < 3; ++k) {
    const double us = std::chrono::duration<double, std::micro>(t[k + 1] - t[k]).count();
    s.sum_us[route][first + k] += us;
    s.min_us[route][first + k] = std::min(s.min_us[route][first + k], us);
  }
  if (first == 0) s.calls[route] += 1;
}
struct SpEndTimer {  // (end has many exits: the last stamp is taken when the result has been built)
  wfst_ctx* ctx;
  int route = 0;
  std::chrono::steady_clock::time_point t[4];
  explicit SpEndTimer(wfst_ctx* c) : ctx(c) { t[0] = t[1] = t[2] = std::chrono::steady_clock::now(); }
  ~SpEndTimer() {
    t[3] = std::chrono::steady_clock::now();
    sp_timing_add(ctx, route, 3, t);
  }
};
#else
#define SP_STAMP(t) ((void)0)
#endif

// What the solve that parked a context's scratch was planned under (RearmRecord::solo), kept only where a bounded head could
// have ended that solve: the solo query compares the knobs of its call with these, field by field.
struct SoloArm {
  Knobs kn;
  uint32_t relax_kernel;  // wfst_stats::relax_kernel as relax_setup set it
};
const char* solo_abort_text(uint32_t verdict) {
  return verdict == SOLO_ABORT_BAND   ? "no total at or below the first band"
         : verdict == SOLO_ABORT_GREW ? "a level outgrew its workgroup"
         : verdict == SOLO_ABORT_LOG  ? "the log of written keys is full"
                                      : "its list did not run empty";
}

// The scratch a solo job took out of its context goes back, parked as it was (the kernel has put every key back; the caller has
// seen the ticket or waited for the stream).  false: other scratch has been parked on the context since — these blocks go back
// to the pool.
bool solo_restore(wfst_sp_job* j) {
  wfst_ctx* ctx = j->ctx;
  RearmRecord& r = ctx->rearm;
  const bool back = !r.plan;
  if (back) {
    r = std::move(j->solo_rec);
    ctx->pool->park(r.blk, RearmRecord::BLOCKS);
    ctx->rearm_stats.armed += 1;
  } else {
    // (the ticket only says that wave 0's stores have landed: blocks that leave this stream's custody — another context may take
    // them from the shared pool at once — wait for the kernel's end)
    (void)hipStreamSynchronize(ctx->stream);
    for (void* b : j->solo_rec.blk) ctx->pool->free(b);
    ctx->rearm_stats.dropped += 1;
  }
  j->solo_rec.clear();
  return back;
}

// The solo query (sssp_solo.h) where today's code would queue "the bounded head and nothing behind it" on re-armed scratch: the
// checks that keep the route correct across edits, knob changes and other queries, then ONE launch on the parked key[].  No
// allocation, no plan, no view: the scratch stays as the re-arm launch left it, apart from the keys the kernel writes and puts
// back.  What is left of the pool and the lease: the six parked blocks are made live for the launch and parked again by end (one
// lock each way), and the resident lease is held where the scratch was planned with it (below).  Returns why the route is not taken (nothing has happened then), null when the launch is queued.
const char* solo_begin(wfst_sp_job* j, const Knobs& kn) {
  wfst_ctx* ctx = j->ctx;
  const wfst_fst* f = j->f;
  RearmRecord& r = ctx->rearm;
  if (kn.solo == 0) return "switched off (WFST_SSSP_SOLO=0)";
  if (ctx->solo_hold) return "not eligible: the repeat of a query that the solo kernel gave up";
  if (ctx->chain_timing || ctx->bounded_hold || ctx->resident_hold) return "not eligible: profiling, or the repeat of a query";
  if (!r.plan) return "nothing parked";
  if (!r.solo) return "not eligible: the parked scratch is not that of a query a bounded head may end";
  const SoloArm& arm = *static_cast<const SoloArm*>(r.solo.get());
  if (!knobs_same_plan(kn, arm.kn)) return "knobs differ";
  if (!j->rev || !j->rev->has_fin || !j->rev->fin_nonneg) return "not eligible: no list of final states, or a negative final weight";
  if (!mbox_eligible(f) || f->last_sweeps.load(std::memory_order_relaxed) == 0) return "not eligible";
  {
    std::lock_guard<std::mutex> lk(f->cache_mu);
    if (f->mbox != r.plan || f->n_states != r.n) return "parked for another plan";
  }
  // (the first band, as relax_setup computes it: an edit of the weights that keeps the plan shows here)
  const float tau0 = band_from_cheapest_arcs(f, *r.plan, band_from_mean_weight(f, kn), kn) * (kn.tau0_mult > 0.0f ? kn.tau0_mult : 1.0f);
  uint32_t tau0_bits;
  std::memcpy(&tau0_bits, &tau0, sizeof(tau0_bits));
  if (tau0_bits != r.tau0_bits || r.log != 12 || !r.narrow) return "knobs differ";
  // (resident or not, as lease_resident would decide now: a lease that is out, a pause behind an abort or another device share
  // would make the ordinary route drop this scratch and plan again — and say so in wfst_stats.relax_kernel)
  const bool res_now = kn.resident && resident_block_log(ctx, f->n_states, kn) != 0 && ctx->resident_allowed() && !kn.big;
  if (res_now != r.resident) return "not eligible: the device share or a pause of the resident launches has changed the plan";
  // three stops in a row on this context, nobody else's query of the handle in between, and the start where it was (set_start
  // resets the handle's own streak); WFST_SSSP_SOLO=2 goes whatever the streak
  if (kn.solo < 2 && (r.stops < 3 || r.epoch + 1 != j->epoch || f->bounded_streak.load(std::memory_order_relaxed) < 3))
    return "fewer than three stops in a row";
  if (!ctx->solo_log.p) ctx->solo_log = DBuf<uint32_t>(*ctx->pool, SOLO_LOG_CAP);
  // The lease, held from here to end like that of the solve this launch replaces — the kernel itself needs no compute unit to
  // itself, but who else finds a unit while this query is in flight, and what their wfst_stats.relax_kernel says, stays as it was
  // (tests/test_gpu_parity.py: a third query beside two half-device ones takes one launch per level).
  if (r.resident && !j->sv.lease.acquire(ctx->device, ctx->resident_share == 1u ? 1 : 2)) return "not eligible: the resident lease is out";
  if (!ctx->pool->unpark(r.blk, RearmRecord::BLOCKS)) {  // (the pool's trim: hipFree has waited for the re-arm launch)
    j->sv.lease.release();
    r.clear();
    ctx->rearm_stats.dropped += 1;
    return "blocks reclaimed";
  }
  ctx->rearm_stats.adopted += 1;
  j->solo_rec = std::move(r);
  r.clear();
  const uint32_t log_cap = std::min<uint32_t>(SOLO_LOG_CAP, kn.solo_log.value_or(SOLO_LOG_CAP));
  SP_STAMP(j->t_begin[1]);
  sssp_solo_kernel<<<1, MB_THREADS, 0, ctx->stream>>>(f->dev.offsets, f->dev.wn, (uint64_t*)j->solo_rec.blk[RH_KEY], f->n_states, (uint32_t)f->start,
                                                      tau0, f->dev.finals, j->rev->fin.p, j->rev->n_fin, f->dev.arcs, j->rev->off.p,
                                                      j->rev->arc.p, j->h_path, PATH_PINNED, j->h_tail, ctx->solo_log.p, log_cap,
                                                      j->done_ticket);
  SP_STAMP(j->t_begin[2]);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) {
    (void)solo_restore(j);
    throw Error(std::string("HIP error ") + hipGetErrorString(err) + " launching the solo query");
  }
  ctx->solo_query.attempts += 1;
  ctx->stats.sweeps = 0;
  ctx->stats.relax_kernel = arm.relax_kernel;
  j->solo = true;
  j->fused_tail = true;
  j->tail_queued = true;
  j->sv.kn = kn;
  j->sv.armed = true;
  j->drv.ctx = ctx;
  j->drv.sv = &j->sv;
  j->drv.done_word = &j->h_tail->done;
  j->drv.done_ticket = j->done_ticket;
  return nullptr;
}
}  // namespace

void sp_host_timing_report(wfst_ctx* ctx) {
#ifdef WFST_SP_HOST_TIMING
  std::lock_guard<std::mutex> lk(sp_timing_mu);
  const auto it = sp_timing_of.find(ctx);
  if (it == sp_timing_of.end()) return;
  sp_timing_print(it->second);
  sp_timing_of.erase(it);
#else
  (void)ctx;
#endif
}

wfst_sp_job* shortest_path_n1_begin(wfst_ctx* ctx, const wfst_fst* f) {
  std::unique_ptr<wfst_sp_job> j(new wfst_sp_job());
  j->ctx = ctx;
  j->f = f;
  SP_STAMP(j->t_begin[0]);
  const uint32_t n = f->n_states;
  if (f->start < 0 || n == 0) {
    j->trivial = true;
    return j.release();
  }
  ensure_device(const_cast<wfst_fst*>(f));
  if (ctx->tie_reference) {  // the reference's own choice among tied optima, where its relaxation order is a topological one
    std::vector<uint32_t> rank;
    ctx->stats.tied_choices = WFST_TIES_UNKNOWN;
    if (reference_top_rank(f, rank)) {
      j->ready = shortest_path_reference_order(ctx, f, rank);
      return j.release();
    }
    // A cycle (the reference relaxes inside an SCC queue) or unit weights (LIFO): its choice among tied optima is a function
    // of its whole relaxation history there.  A UNIQUE optimum needs no choice: the canonical path is then the reference's
    // path, and the tail kernel counts the tied choices along it (sssp_walk_back) — with any, the call is KO.
    j->need_unique = true;
  }
  ctx->stats.tied_choices = WFST_TIES_UNKNOWN;
  char* pin = (char*)ctx->pinned.get(sizeof(Ctl) + 128 + PATH_PINNED * sizeof(wfst_tr));
  j->hc = (Ctl*)pin;
  j->h_tail = (TailOut*)(pin + ((sizeof(Ctl) + 63) & ~(size_t)63));
  j->h_path = (wfst_tr*)(pin + ((sizeof(Ctl) + 63) & ~(size_t)63) + 64);
  static_assert(sizeof(TailOut) <= 64, "the path's arcs follow the header at + 64");
  static std::atomic<uint32_t> tickets{0};
  do j->done_ticket = tickets.fetch_add(1, std::memory_order_relaxed) + 1u; while (j->done_ticket == 0u);
  j->h_tail->done = 0u;
  j->h_tail->rearmed = 0u;
  j->h_tail->bounded_why = 0u;
  j->h_tail->solo = 0u;
  j->rev = reverse_csr(ctx, f, j->need_unique);  // may build the transpose (second query of a large FST): before anything is queued
  j->epoch = f->sp_epoch.fetch_add(1, std::memory_order_relaxed) + 1u;
  if (ctx->profiling) {
    run_relaxation(ctx, f, j->sv);  // per-sweep events: synchronous
    return j.release();
  }
  const Knobs kn = read_knobs();
  j->solo_why = solo_begin(j.get(), kn);
  if (j->solo) {  // (one launch is queued; end waits for its ticket)
    SP_STAMP(j->t_begin[3]);  // ([1], [2]: solo_begin, in front of and behind the launch)
#ifdef WFST_SP_HOST_TIMING
    sp_timing_add(ctx, 1, 0, j->t_begin);
#endif
    return j.release();
  }
  relax_setup(ctx, f, j->sv, &kn);
  SP_STAMP(j->t_begin[1]);
  if (j->sv.armed && j->sv.rearm_epoch + 1u != j->epoch) j->sv.rearm_stops = 0;  // (somebody else has queried the handle since)
  if (j->sv.kn.final_list >= 2 && j->rev && !j->rev->has_fin) {  // tests: which of the two tails a handle gets
    (void)hipStreamSynchronize(ctx->stream);  // (the set-up is queued: the solve's buffers go back to the pool after this)
    throw Error("shortest_path: WFST_SSSP_FINAL_LIST=2 and the handle has no list of final states");
  }
  ctx->stats.sweeps = 0;
  j->drv.init(ctx, f, &j->sv);
  const bool fuse = j->drv.predicted && j->rev && !j->sv.kn.split_tail;
  // the early tail: the fused tail over the handle's list of final states, no negative weight anywhere (arcs: mbox_eligible)
  if (fuse && j->sv.mbox && j->sv.kn.early_tail != 0 && j->rev->has_fin && j->sv.kn.final_list != 0 && j->rev->fin_nonneg) {
    j->sv.early_on = true;
    j->sv.early = EarlyTail{j->rev->fin.p, f->dev.finals, f->dev.arcs, j->rev->off.p, j->rev->arc.p, j->h_path, j->h_tail,
                            j->rev->n_fin, PATH_PINNED, 0u};
    // the blocks' best final states from the resident launch's hand-over (8192-state blocks: that kernel runs the NARROW
    // launches itself and there is no extra workgroup)
    if (j->sv.kn.early_best != 0 && j->sv.resident && j->sv.log == 12) {
      j->sv.blk_best_on = true;
      j->sv.early.blk_best_on = 1u;
    }
  }
  // The bounded head (sssp_mailbox.h, above mbox_narrow): launch 0 ends the search once the best final state is settled.  Only
  // where the ordinary tail that follows is the fused one over the handle's list of final states, the launches are mailbox ones
  // with NARROW launches on 4096-state blocks, and no arc (mbox_eligible) or final weight is negative.  Profiling (1: this
  // function has returned above; 2: the chain is timed as the relaxation of every arc) runs the full solve, and so do the strict
  // settings of the knobs that demand a later stage of the solve (WFST_SSSP_EARLY_TAIL=2, WFST_SSSP_EARLY_BEST=2) and the
  // repeat of a query whose path outgrew the pinned buffer (wfst_ctx::bounded_hold).
  {
    Solve& sv = j->sv;
    const char* why = nullptr;
    if (sv.kn.bounded == 0) why = "switched off (WFST_SSSP_BOUNDED=0)";
    else if (ctx->chain_timing) why = "not eligible: profiling is on";
    else if (ctx->bounded_hold) why = "not eligible: the repeat of a query whose path outgrew the pinned buffer";
    else if (!sv.mbox || sv.narrow_t == 0) why = "not eligible: no mailbox solve with NARROW launches";
    else if (sv.log != 12) why = "not eligible: blocks of 8192 states";
    else if (!fuse) why = "not eligible: no fused tail (first query of the handle, no transpose, or WFST_SSSP_SPLIT_TAIL)";
    else if (!j->rev->has_fin || sv.kn.final_list == 0) why = "not eligible: the handle has no list of final states";
    else if (!j->rev->fin_nonneg) why = "not eligible: a negative final weight";
    else if (sv.kn.early_tail >= 2 || sv.kn.early_best >= 2) why = "not eligible: WFST_SSSP_EARLY_TAIL=2 / WFST_SSSP_EARLY_BEST=2 demand the full solve";
    // (WFST_SSSP_RES_LEVELS caps the levels of the resident launch so that a solve outruns its prediction, WFST_SSSP_RES_TLIM_US
    // sets its wait limit so that it gives up: experiments on the later launches of the full solve, which a stop in launch 0
    // would never reach — tests/test_rearm.py and tests/test_gpu_parity.py pin those routes)
    else if (sv.kn.res_levels || sv.kn.res_tlim_us)
      why = "not eligible: WFST_SSSP_RES_LEVELS / WFST_SSSP_RES_TLIM_US shape the later launches of the full solve";
    sv.bounded_on = why == nullptr;
    sv.bounded_why = why;
    if (sv.bounded_on) sv.early.finals = f->dev.finals;  // (what the early tail, if it is on, has set already)
    // The chain of a query whose predecessors on this FST stopped in launch 0: that launch and a spare one (none after three in a
    // row).  A head that does not stop after all takes the extended path, like any solve that outruns its prediction.
    const uint32_t streak = f->bounded_streak.load(std::memory_order_relaxed);
    if (sv.bounded_on && streak) j->drv.first_count = std::min<uint32_t>(j->drv.first_count, streak >= 3 ? 1u : 2u);
  }
  j->drv.start(/*defer_advance=*/fuse);
  SP_STAMP(j->t_begin[2]);  // (taken again behind each later launch: what is left to [3] is the launch checks and the return)
  if (fuse) {  // the tail closes the batch: flags to the host, base advanced, then the ticket finish() waits for
    // ... and behind the ticket, where the stream has nothing to do until the next query, the scratch is cleaned for that query
    // if the tail finds this one over (Ctl::rearm): 4096-state blocks with NARROW launches (launch 0 then seeds the start itself)
    Solve& sv = j->sv;
    j->rearm_queued = sv.mbox && sv.log == 12 && sv.narrow_t != 0 && sv.kn.rearm != 0;
    queue_tail(j.get(), &j->drv.cur);
    j->tail_queued = true;
    j->drv.done_word = &j->h_tail->done;
    j->drv.done_ticket = j->done_ticket;
    if (j->rearm_queued) {
      sssp_mbox_rearm_kernel<12><<<sv.blocks, 256, 0, ctx->stream>>>(sv.key.p, sv.mv, sv.improved.p, sv.ctl.p, n, sv.tau0, sv.rv.msgs[0],
                                                                     sv.rv.msgs[1], sv.rv.roffh, sv.rv.abort);
      SP_STAMP(j->t_begin[2]);
      HIP_CHECK(hipGetLastError());
    } else {
      SP_STAMP(j->t_begin[2]);
    }
  } else if (j->drv.predicted && j->rev) {
    queue_tail(j.get());
    SP_STAMP(j->t_begin[2]);
    j->tail_queued = true;
  }
  SP_STAMP(j->t_begin[3]);
#ifdef WFST_SP_HOST_TIMING
  sp_timing_add(ctx, 0, 0, j->t_begin);
#endif
  return j.release();
}

wfst_fst* shortest_path_n1_end(wfst_sp_job* job) {
  std::unique_ptr<wfst_sp_job> j(job);
  wfst_ctx* ctx = j->ctx;
  const wfst_fst* f = j->f;
  if (j->trivial) {
    ctx->stats.tied_choices = 0;
    return make_path_fst(ctx, false, 0, INF, nullptr);
  }
  if (j->ready) return j->ready;
  const uint32_t n = f->n_states;
  hipStream_t st = ctx->stream;
  Solve& sv = j->sv;
#ifdef WFST_SP_HOST_TIMING
  SpEndTimer timer(ctx);
  timer.route = j->solo ? 1 : 0;
#endif
  // A bounded stop (or the solo kernel's answer) whose path is longer than the pinned buffer: the parent pass would read every
  // key, and the keys above B are not the fixed point.  The whole query again, unbounded.
  auto again_unbounded = [&]() -> wfst_fst* {
    j.reset();
    struct Hold {
      wfst_ctx* c;
      explicit Hold(wfst_ctx* x) : c(x) { c->bounded_hold = true; }
      ~Hold() { c->bounded_hold = false; }
    } hold(ctx);
    return shortest_path_n1_end(shortest_path_n1_begin(ctx, f));
  };
  if (j->solo) {
    // The ticket, then the scratch parked again as it was (the kernel has put every key back), then the verdict: an abort is the
    // query again by the ordinary route — nothing of the attempt is reused, and the next queries are ordinary until three stop in
    // a row again.  An answer is booked as the bounded stop of one launch that it replaces.
    j->drv.wait_first_batch();
    sv.lease.release();
    SP_STAMP(timer.t[1]);
    HIP_CHECK(hipPeekAtLastError());
    RearmRecord& r = ctx->rearm;
    const bool back = solo_restore(j.get());
    SP_STAMP(timer.t[2]);
    const uint32_t verdict = j->h_tail->solo;
    ctx->solo_query.cleaned = j->h_tail->solo_cleaned;
    // (a stop whose path is longer than the pinned buffer is no answer either: the result comes from the unbounded repeat, and
    // it is decided before anything is booked as answered)
    const bool too_long = verdict == SOLO_ANSWERED && (j->h_tail->pad & 8u) && !(j->h_tail->pad & 5u);
    if (verdict != SOLO_ANSWERED || too_long) {
      ctx->solo_query.aborted += 1;
      ctx->solo_query.last_abort = too_long ? SOLO_ABORT_OTHER - 1u : verdict - 1u;
      if (back) r.stops = 0;
      f->bounded_streak.store(0, std::memory_order_relaxed);
      const bool strict = sv.kn.solo >= 2;
      j.reset();
      Handle out;
      {
        struct Hold {  // (too_long: the repeat may not stop bounded either — the same header would come back)
          wfst_ctx* c;
          bool unbounded;
          Hold(wfst_ctx* x, bool u) : c(x), unbounded(u) {
            c->solo_hold = true;
            if (unbounded) c->bounded_hold = true;
          }
          ~Hold() {
            c->solo_hold = false;
            if (unbounded) c->bounded_hold = false;
          }
        } hold(ctx, too_long);
        out.reset(shortest_path_n1_end(shortest_path_n1_begin(ctx, f)));
      }
      if (strict)  // tests: a query that the solo kernel answered, or an error that says why not
        throw Error(std::string("shortest_path: WFST_SSSP_SOLO=2 and the solo kernel gave the query up: ") +
                    (too_long ? "the path is longer than the pinned buffer" : solo_abort_text(verdict)));
      return out.release();
    }
    ctx->solo_query.answered += 1;
    if (back) {
      r.stops += 1;
      r.epoch = j->epoch;
    }
    ctx->stats.sweeps = 1;
    ctx->bounded.stops += 1;
    f->bounded_streak.fetch_add(1, std::memory_order_relaxed);
    resident_work_of(ctx->device).store(0, std::memory_order_relaxed);  // (record_solve's hint: no grid of whole compute units ran)
  } else {
  if (!ctx->profiling && !finish_solve(ctx, f, sv, j->drv)) {  // a resident launch gave up waiting: the whole query again
    j.reset();  // (its buffers go back to the pool)
    ResidentHold hold(ctx);
    return shortest_path_n1_end(shortest_path_n1_begin(ctx, f));
  }
  if (j->tail_queued && j->drv.extended) {  // the speculative tail ran on unfinished distances: once more
    HIP_CHECK(hipMemsetAsync(&sv.ctl.p->best, 0xFF, sizeof(unsigned long long), st));
    j->tail_queued = false;
  }
  if (!j->tail_queued) queue_tail(j.get());
  // (the ticket of the fused tail was the last thing this job had on the stream: nothing to wait for)
  if (!(j->tail_queued && j->fused_tail && j->drv.done_seen && !j->drv.extended) || ctx->chain_timing) HIP_CHECK(hipStreamSynchronize(st));
  else HIP_CHECK(hipPeekAtLastError());  // (no stream wait on this path.  Reports launch-configuration / sticky API errors the runtime has already
                                              // seen — NOT an asynchronous kernel fault: a chain that faults never writes its ticket, and the spin above then
                                              // ends in the stream wait, which reports it.  Peek, not Get: the error may belong to another thread's launch)
  SP_STAMP(timer.t[1]);
  if (j->rearm_queued) {
    // The tail's verdict, believed as it stands: the re-arm launch is cleaning (or has cleaned) the scratch, which is parked for
    // the next solve on this context instead of going back to the pool — other contexts allocate from it on other streams.
    // A re-arm launch that was queued and whose scratch is not parked is waited for (it returns at once when the verdict is 0).
    RearmRecord& r = ctx->rearm;
    if (j->h_tail->rearmed != 0u && !j->drv.extended && !r.plan) {
      r.plan_pool = f->owner_pool ? f->owner_pool : ctx->pool;
      r.plan = sv.plan;
      r.n = n;
      r.log = sv.log;
      r.stg = sv.mv.stg;
      std::memcpy(&r.tau0_bits, &sv.tau0, sizeof(r.tau0_bits));
      r.resident = sv.resident;
      r.narrow = sv.narrow_t != 0;
      // (the solo query's view of this scratch: sssp_solo.h)
      r.solo = sv.bounded_on ? std::make_shared<SoloArm>(SoloArm{sv.kn, (uint32_t)ctx->stats.relax_kernel}) : nullptr;
      r.stops = j->drv.bounded ? sv.rearm_stops + 1u : 0u;
      r.epoch = j->epoch;
      auto note = [&](size_t i, auto& buf) {
        r.blk[i] = buf.p;
        r.cnt[i] = buf.p ? buf.n : 0;
      };
      note(RH_KEY, sv.key);
      note(RH_MB_WORDS, sv.mb_words);
      note(RH_IMPROVED, sv.improved);
      note(RH_CTL, sv.ctl);
      note(RH_RS_MSGS, sv.rs_msgs);
      note(RH_RS_ABORT, sv.rs_abort);
      ctx->pool->park(r.blk, RearmRecord::BLOCKS);
      (void)sv.key.release();
      (void)sv.mb_words.release();
      (void)sv.improved.release();
      (void)sv.ctl.release();
      (void)sv.rs_msgs.release();
      (void)sv.rs_abort.release();
      ctx->rearm_stats.armed += 1;
    } else {
      HIP_CHECK(hipStreamSynchronize(st));
    }
    j->rearm_queued = false;
  }
  SP_STAMP(timer.t[2]);
  // The bounded head's book-keeping.  `stopped`: launch 0 posted FLAG_NARROW_BOUNDED and the fused tail behind the first batch
  // searched keys that are exact at and below B (never an extended solve: the flag is launch 0's).
  const bool b_stopped = j->drv.bounded;
  if (sv.bounded_on) {
    if (b_stopped) ctx->bounded.stops += 1;
    else {
      const uint32_t w = j->fused_tail ? j->h_tail->bounded_why : 0u;
      ctx->bounded.full_solves += 1;
      ctx->bounded_last_refusal = w == BOUNDED_WHY_BAND   ? "the head did not stop: no total at or below the first band"
                                  : w == BOUNDED_WHY_GREW ? "the head did not stop: a level outgrew its workgroup"
                                                          : "the head did not stop: its list did not run empty";
    }
  } else {
    ctx->bounded.full_solves += 1;
    ctx->bounded_last_refusal = ctx->profiling ? "not eligible: profiling is on" : sv.bounded_why ? sv.bounded_why : "not eligible";
  }
  // (a path longer than the pinned buffer; the tail gave this solve no re-arm verdict: the stream was waited for above)
  if (b_stopped && j->fused_tail && (j->h_tail->pad & 8u) && !(j->h_tail->pad & 5u)) return again_unbounded();
  if (sv.kn.bounded >= 2 && !b_stopped)  // tests: a query that the bounded head ended, or an error that says why not
    throw Error(std::string("shortest_path: WFST_SSSP_BOUNDED=2 and the bounded head did not end the solve: ") + ctx->bounded_last_refusal);
  if (sv.kn.rearm >= 2 && !sv.armed)  // tests: a solve that started from re-armed scratch, or an error that says why not
    throw Error(std::string("shortest_path: WFST_SSSP_REARM=2 and the solve did not start from re-armed scratch: ") +
                (sv.rearm_why ? sv.rearm_why : "not eligible"));
  if (ctx->chain_timing && !ctx->profiling) {  // the sweeps of this query as one chain (wfst_ctx_set_profiling(ctx, 2))
    ctx->stats.relax_ms = 0.0;
    ctx->stats.relax_launches = 0;
    if (j->drv.predicted && !j->drv.extended) {
      float ms = 0.0f;
      HIP_CHECK(hipEventElapsedTime(&ms, ctx->ev_chain[0], ctx->ev_chain[1]));
      ctx->stats.relax_ms = ms;
      ctx->stats.relax_launches = j->drv.first_count;
    }
  }
  if (sv.kn.early_tail >= 2) {  // tests: the early tail's result or an error that says why not
    const uint32_t e = sv.early_on && j->fused_tail && !j->drv.extended ? j->h_tail->early : EARLY_ABSENT;
    if (e != EARLY_USED)
      throw Error(std::string("shortest_path: WFST_SSSP_EARLY_TAIL=2 and the early tail's result was ") +
                  (!sv.early_on ? "not eligible" : e == EARLY_REFUTED ? "refuted" : "absent"));
  }
  if (sv.kn.early_best >= 2) {  // tests: the result the early tail merged from the blocks' best final states, or an error that says why not
    const bool ran = sv.early_on && sv.log == 12 && j->fused_tail && !j->drv.extended;
    const uint32_t e = ran ? j->h_tail->early : EARLY_ABSENT;
    if (e != EARLY_USED || !sv.blk_best_on || j->h_tail->early_src != EARLY_SRC_BLOCKS)
      throw Error(std::string("shortest_path: WFST_SSSP_EARLY_BEST=2 and the blocks' best final states were not the result's source: ") +
                  (!sv.early_on || sv.log != 12 ? "not eligible" : !sv.blk_best_on ? "no resident hand-over" : e == EARLY_REFUTED ? "refuted"
                   : e != EARLY_USED ? "absent" : "no resident hand-over"));
  }
  // tests: a query that the solo kernel answered, or an error that says why the route was not taken (the repeat behind an abort
  // of that kernel reports through the call that made it)
  if (sv.kn.solo >= 2 && !ctx->solo_hold)
    throw Error(std::string("shortest_path: WFST_SSSP_SOLO=2 and the solo kernel did not answer the query: ") +
                (j->solo_why ? j->solo_why : "not eligible"));
  }  // (the ordinary route)
  const Ctl* hc = j->hc;
  const uint32_t r_pad = j->fused_tail ? j->h_tail->pad : hc->pad, r_has_path = j->fused_tail ? j->h_tail->has_path : hc->has_path;
  if (r_pad & 1u) throw Error("shortest_path: hop count overflow in the mailbox sweeps (internal error)");
  if (r_pad & 4u) throw Error("shortest_path: no admissible predecessor on the path (inexact weight sums with negative weights)");
  if (!r_has_path) {  // no final state is reachable: the empty FST, and nothing to choose
    ctx->stats.tied_choices = 0;
    return make_path_fst(ctx, false, 0, INF, nullptr);
  }
  const uint32_t hops = j->fused_tail ? j->h_tail->hops : hc->hops;
  const float final_weight = j->fused_tail ? j->h_tail->final_weight : hc->final_weight;
  // tied choices along the returned path: counted by the one-launch tail's walk over the in-arcs (unknown on the other paths)
  const uint64_t ties = j->fused_tail && !(r_pad & 8u) ? (uint64_t)j->h_tail->ties : WFST_TIES_UNKNOWN;
  ctx->stats.tied_choices = ties;
  if (j->need_unique) {
    if (ties == WFST_TIES_UNKNOWN)
      throw Error("shortest_path: tie order 1 on a cyclic input: the optimum could not be certified unique (no transpose for this input, or a path "
                  "beyond the walk's buffer)");
    if (ties != 0)
      throw Error("shortest_path: ambiguous optimum: " + std::to_string(ties) + " tied choice(s) on the optimal path of a cyclic input — the "
                  "reference's choice there depends on its relaxation order (tie order 1 returns only what is provably its result)");
  }
  if (j->rev && !(r_pad & 8u)) return make_path_fst(ctx, true, hops, final_weight, j->h_path);
  // the parent pass (first query of an FST, or a path longer than the pinned buffer): a path has at most n - 1 arcs
  std::vector<wfst_tr> path;
  uint32_t len = 0;
  {
    DBuf<unsigned long long> parent(*ctx->pool, n);
    HIP_CHECK(hipMemsetAsync(parent.p, 0xFF, (size_t)n * sizeof(unsigned long long), st));
    HIP_CHECK(hipMemsetAsync(&sv.ctl.p->pad, 0, sizeof(uint32_t), st));
    const uint32_t blocks = std::min<uint32_t>((uint32_t)ctx->n_cus * 8, (uint32_t)(((uint64_t)n * GROUP + 255) / 256));
    sssp_parent_kernel<<<blocks, 256, 0, st>>>(f->dev.offsets, f->dev.wn, sv.key.p, parent.p, n);
    // the walk is as long as the final state's hop count except where class-1 predecessors lengthen it: room for four times
    // that (not 16 B per STATE of a multi-million-state input for a path of a few thousand arcs), all of n on the rare retry
    uint32_t cap = (uint32_t)std::min<uint64_t>(n, 4ull * hops + 1024);
    DBuf<wfst_tr> out(*ctx->pool, cap);
    for (;;) {
      sssp_backtrace_kernel<<<1, 64, 0, st>>>(f->dev.offsets, f->dev.arcs, sv.key.p, parent.p, sv.ctl.p, out.p, cap);
      HIP_CHECK(hipMemcpyAsync(j->hc, sv.ctl.p, sizeof(Ctl), hipMemcpyDeviceToHost, st));
      HIP_CHECK(hipStreamSynchronize(st));
      if (!(hc->pad & 16u) || cap >= n) break;
      cap = n;
      out = DBuf<wfst_tr>(*ctx->pool, cap);
      HIP_CHECK(hipMemsetAsync(&sv.ctl.p->pad, 0, sizeof(uint32_t), st));
    }
    if (hc->pad & 4u) throw Error("shortest_path: no admissible predecessor on the path (inexact weight sums with negative weights)");
    len = hc->hops;
    path.resize(len);
    if (len) HIP_CHECK(hipMemcpy(path.data(), out.p, (size_t)len * sizeof(wfst_tr), hipMemcpyDeviceToHost));
  }
  return make_path_fst(ctx, true, len, final_weight, path.data());
}

void shortest_path_n1_abandon(wfst_sp_job* job) {
  std::unique_ptr<wfst_sp_job> j(job);
  delete j->ready;
  if (!j->trivial) (void)hipStreamSynchronize(j->ctx->stream);  // the solve's buffers go back to the pool after this
  if (j->solo) {  // (the kernel has put every key back: the scratch is parked again as it was, its streak over)
    if (solo_restore(j.get())) j->ctx->rearm.stops = 0;
  }
}

wfst_ctx* sp_job_ctx(wfst_sp_job* job) { return job->ctx; }

wfst_fst* shortest_path_n1(wfst_ctx* ctx, const wfst_fst* f) {
  wfst_fst* tiny = nullptr;
  if (shortest_path_n1_tiny(ctx, f, &tiny)) return tiny;
  return shortest_path_n1_end(shortest_path_n1_begin(ctx, f));
}

}  // namespace wfst

// The solo query's counters (common.h: wfst_ctx::solo_query), beside the route that keeps them.  Any out-pointer may be null.
extern "C" wfst_status wfst_ctx_get_solo_query(wfst_ctx* ctx, uint64_t* attempts, uint64_t* answered, uint64_t* aborted,
                                               uint64_t* last_abort, uint64_t* cleaned) {
  return wfst::wrap([&] {
    if (!ctx) throw wfst::Error("null pointer");
    const wfst_ctx::SoloQueryCounts& c = ctx->solo_query;
    if (attempts) *attempts = c.attempts;
    if (answered) *answered = c.answered;
    if (aborted) *aborted = c.aborted;
    if (last_abort) *last_abort = c.last_abort;
    if (cleaned) *cleaned = c.cleaned;
  });
}

// Tests: the words of ctx's parked key[] that are not KEY_INF (an armed scratch has none).  Synchronous; KO and 0 words when
// nothing is parked.
extern "C" wfst_status wfst_ctx_parked_key_check(wfst_ctx* ctx, uint64_t* not_inf) {
  return wfst::wrap([&] {
    using namespace wfst;
    if (!ctx || !not_inf) throw Error("null pointer");
    *not_inf = 0;
    RearmRecord& r = ctx->rearm;
    if (!r.plan || !r.blk[RH_KEY]) throw Error("wfst_ctx_parked_key_check: nothing is parked on this context");
    HIP_CHECK(hipSetDevice(ctx->device));
    if (!ctx->pool->unpark(r.blk, RearmRecord::BLOCKS)) {  // (the pool's trim has taken the blocks)
      r.clear();
      ctx->rearm_stats.dropped += 1;
      throw Error("wfst_ctx_parked_key_check: nothing is parked on this context");
    }
    struct Repark {  // (live while the kernel reads them, parked again on every exit)
      wfst_ctx* c;
      ~Repark() { c->pool->park(c->rearm.blk, RearmRecord::BLOCKS); }
    } repark{ctx};
    DBuf<unsigned long long> count(*ctx->pool, 1);
    HIP_CHECK(hipMemsetAsync(count.p, 0, sizeof(unsigned long long), ctx->stream));
    sssp_key_check_kernel<<<std::max<uint32_t>(1u, std::min<uint32_t>((uint32_t)ctx->n_cus * 4, (r.n + 255) / 256)), 256, 0, ctx->stream>>>(
        (const uint64_t*)r.blk[RH_KEY], r.n, count.p);
    HIP_CHECK(hipGetLastError());
    unsigned long long h = 0;
    HIP_CHECK(hipMemcpyAsync(&h, count.p, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    *not_inf = h;
  });
}
