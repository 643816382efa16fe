// push.hip — shortest_distance(fst, reverse), reweight and push_weights on the device
// (rustfst/src/algorithms/{shortest_distance.rs:307-336, reweight.rs, push.rs:76-170}):
//   reverse distances  reverse(fst) (nshortest.hip reverse_fst, cached on the handle as rev_fst) + the relaxation (sssp.hip)
//   Vec length         frontier BFS from the source (bfs_round_kernel): one plus the largest state id the search touches
//   reweight           reweight_arcs_kernel (16 lanes per state, facts reduced in the same pass) + reweight_finals_kernel
//   total weight       total_weight_kernel: wave min-reduction, one atomicMin per wave on the order-preserving u32 key
//   INITIAL_ACYCLIC    only when the start branch runs and the word does not know it: reachability (BFS from the start),
//                      co-reachability (BFS on the reversed handle), cycle existence (in-degree peeling), start on a cycle
//   the start state    (at most one arc list and one final weight) and the property word: on the host
//   which route ran    wfst_ctx_get_push_stats, tallied on the host (include/wfst.h; WFST_PUSH_MAX_BLOCKS for tests)
// TropicalWeight with the reference's semantics: tropical.h (a start potential within 1/1024 of 0 is one).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "common.h"
#include "fst_props.h"

namespace wfst {

// WFST_PUSH_MAX_BLOCKS=n (tests): at most n blocks for bfs_round_kernel, reweight_arcs_kernel and total_weight_kernel, the
// three kernels that stride, so that inputs of a few hundred states run their stride loops.  0: no cap (unset or empty).
uint32_t push_max_blocks_knob() {
  const char* e = std::getenv("WFST_PUSH_MAX_BLOCKS");
  if (!e || !*e) return 0;
  char* end = nullptr;
  const unsigned long v = std::strtoul(e, &end, 10);
  if (*e < '0' || *e > '9' || *end || std::strlen(e) > 9 || v == 0)
    throw Error(std::string("WFST_PUSH_MAX_BLOCKS: expected a positive number of blocks, not '") + e + "'");
  return (uint32_t)v;
}

namespace {

// blocks of a strided launch: what the work asks for, at most per_cu blocks per compute unit, at most the knob's cap
constexpr uint32_t BFS_BLOCKS_PER_CU = 8;     // bfs_round_kernel
constexpr uint32_t ARCS_BLOCKS_PER_CU = 32;   // reweight_arcs_kernel
constexpr uint32_t TOTAL_BLOCKS_PER_CU = 4;   // total_weight_kernel
uint32_t strided_grid(const wfst_ctx* ctx, uint32_t wanted, uint32_t per_cu) {
  uint32_t blocks = std::max<uint32_t>(1, std::min<uint32_t>(wanted, (uint32_t)ctx->n_cus * per_cu));
  if (const uint32_t cap = push_max_blocks_knob()) blocks = std::min(blocks, cap);
  return blocks;
}

// ---------------------------------------------------------------- structural passes
// One round of a frontier search: every state of the frontier (16 lanes per state) looks at its arcs.
//   mode 0 (reachability): a target not yet visited (vis 0 -> 1) joins the next frontier;
//   mode 1 (peeling): the target's in-degree drops by one, at zero it joins the next frontier.
// Every state joins a frontier at most once, so a frontier never holds more than n states.  cnt_clear is the counter of
// the round after the next one (a ring of three): cleared here, while nothing reads or writes it.
__global__ void __launch_bounds__(256) bfs_round_kernel(const uint32_t* __restrict__ off, const wfst_tr* __restrict__ arcs,
                                                        const uint32_t* __restrict__ fin, const uint32_t* __restrict__ cnt_in,
                                                        uint32_t* __restrict__ fout, uint32_t* __restrict__ cnt_out,
                                                        uint32_t* __restrict__ cnt_clear, uint32_t* __restrict__ mark,
                                                        uint32_t* __restrict__ stats, int mode) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *cnt_clear = 0u;
  const uint32_t m = *cnt_in;
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lane = tid & 15u;
  uint32_t pushed = 0, maxid = 0;
  for (uint32_t k = tid >> 4; k < m; k += (gridDim.x * blockDim.x) >> 4) {
    const uint32_t s = fin[k];
    for (uint32_t i = off[s] + lane; i < off[s + 1]; i += 16) {
      const uint32_t t = arcs[i].nextstate;
      bool join;
      if (mode == 0)
        join = mark[t] == 0u && atomicExch(&mark[t], 1u) == 0u;
      else
        join = atomicSub(&mark[t], 1u) == 1u;
      if (join) {
        fout[atomicAdd(cnt_out, 1u)] = t;
        pushed += 1;
        maxid = max(maxid, t + 1);
      }
    }
  }
  for (int d = 32; d >= 1; d >>= 1) {
    pushed += __shfl_xor(pushed, d);
    maxid = max(maxid, __shfl_xor(maxid, d));
  }
  if ((threadIdx.x & 63) == 0 && pushed) {
    atomicAdd(&stats[0], pushed);  // states that joined a frontier
    atomicMax(&stats[1], maxid);   // 1 + the largest of them
  }
}
// the states without in-arcs: the first frontier of the peeling
__global__ void zero_indegree_kernel(const uint32_t* __restrict__ indeg, uint32_t n, uint32_t* __restrict__ fout,
                                     uint32_t* __restrict__ cnt_out, uint32_t* __restrict__ stats) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s < n && indeg[s] == 0u) {
    fout[atomicAdd(cnt_out, 1u)] = s;
    atomicAdd(&stats[0], 1u);
  }
}

struct Search {
  uint32_t joined = 0;  // states that joined a frontier (the seeds count when `seeds_count`)
  uint32_t maxid = 0;   // 1 + the largest of them (0: none)
};
constexpr uint32_t ROUNDS_PER_CHECK = 16;  // rounds queued between two reads of the frontier size

// Frontier search over g (offsets / arcs on the device) from the states in `seeds`.  mode 0: `mark` holds the visited
// flags (the caller sets those of the seeds it does not want visited again); mode 1: `mark` holds in-degrees and the
// frontier starts with the states of in-degree 0 (seeds ignored).  Rounds are launched ROUNDS_PER_CHECK at a time; the
// host reads the size of the next frontier between batches and stops at an empty one.  The round rule:
// after round R = 1, 2, .. the host reads the size of frontier R when R is a multiple of ROUNDS_PER_CHECK or R = n + 1,
// and stops at the first read that finds it empty or at R = n + 1.
Search frontier_search(wfst_ctx* ctx, uint32_t n, const uint32_t* off, const wfst_tr* arcs, const std::vector<uint32_t>& seeds,
                       uint32_t* mark, int mode) {
  hipStream_t st = ctx->stream;
  DevicePool& pool = *ctx->pool;
  DBuf<uint32_t> fr0(pool, n), fr1(pool, n), ctl(pool, 8);  // ctl: counters[3], stats[2]
  HIP_CHECK(hipMemsetAsync(ctl.p, 0, 8 * sizeof(uint32_t), st));
  uint32_t* cnt = ctl.p;
  uint32_t* stats = ctl.p + 4;
  const uint32_t c = (uint32_t)seeds.size();
  if (mode == 0) {
    if (!seeds.empty()) {
      HIP_CHECK(hipMemcpyAsync(fr0.p, seeds.data(), seeds.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
      HIP_CHECK(hipMemcpyAsync(cnt, &c, sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }
  } else if (n) {
    zero_indegree_kernel<<<(n + 255) / 256, 256, 0, st>>>(mark, n, fr0.p, cnt, stats);
    HIP_CHECK(hipGetLastError());
  }
  const uint32_t blocks = strided_grid(ctx, (n + 15) / 16, BFS_BLOCKS_PER_CU);  // 16 lanes per state
  uint32_t* fr[2] = {fr0.p, fr1.p};
  uint32_t next = 1;
  uint32_t rounds = 0, reads = 0;
  for (uint32_t r = 0;; ++r) {
    bfs_round_kernel<<<blocks, 256, 0, st>>>(off, arcs, fr[r & 1], cnt + r % 3, fr[(r + 1) & 1], cnt + (r + 1) % 3,
                                             cnt + (r + 2) % 3, mark, stats, mode);
    HIP_CHECK(hipGetLastError());
    rounds = r + 1;
    if ((r + 1) % ROUNDS_PER_CHECK == 0 || r + 1 >= n + 1) {
      HIP_CHECK(hipMemcpyAsync(&next, cnt + (r + 1) % 3, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
      HIP_CHECK(hipStreamSynchronize(st));
      reads += 1;
      if (next == 0 || r + 1 >= n + 1) break;  // (n + 1 rounds empty any frontier: each state joins once)
    }
  }
  wfst_ctx::PushStats& ps = ctx->push_stats;
  ps.searches += 1;
  ps.rounds += rounds;
  ps.reads += reads;
  ps.rounds_max = std::max<uint64_t>(ps.rounds_max, rounds);
  ps.bfs_blocks = blocks;
  uint32_t h[2] = {0, 0};
  HIP_CHECK(hipMemcpyAsync(h, stats, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  return Search{h[0], h[1]};
}

// reachability from one state: visited count (the source included) and 1 + the largest visited id
Search reach_from(wfst_ctx* ctx, uint32_t n, const uint32_t* off, const wfst_tr* arcs, uint32_t source) {
  DBuf<uint32_t> vis(*ctx->pool, n);
  HIP_CHECK(hipMemsetAsync(vis.p, 0, (size_t)n * sizeof(uint32_t), ctx->stream));
  const uint32_t one = 1;
  HIP_CHECK(hipMemcpyAsync(vis.p + source, &one, sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
  Search s = frontier_search(ctx, n, off, arcs, {source}, vis.p, 0);
  s.joined += 1;
  s.maxid = std::max(s.maxid, source + 1);
  return s;
}

// reverse(f) as a device handle, cached on f (reverse distances and co-reachability do not depend on the start state, nor on
// the order of arcs inside a state or on their labels)
const wfst_fst* reversed_handle(wfst_ctx* ctx, const wfst_fst* f) {
  std::lock_guard<std::mutex> lk(f->rev_mu);
  if (!f->rev_fst) {
    wfst_fst* r = reverse_fst(ctx, f);
    f->rev_fst = std::shared_ptr<wfst_fst>(r, [](wfst_fst* p) {
      (void)hipSetDevice(p->device);
      delete p;
    });
  }
  ensure_device(f->rev_fst.get());
  return f->rev_fst.get();
}

}  // namespace

// The SccVisitor's four facts (visitors/scc_visitors.rs) on f's graph, with f's final states (reweight never changes which
// states have Some(final weight): set_final is only called on those).  Without a start state dfs_visit returns before it
// visits anything (dfs_visit.rs:104-110), so the visitor's word is the one it was constructed with: all four positive bits.
uint64_t structural_bits(wfst_ctx* ctx, const wfst_fst* f) {
  if (f->start < 0) return props::dfs_bits(true, true, false, false);
  ctx->push_stats.structural = 1;
  const uint32_t n = f->n_states;
  const uint32_t s0 = (uint32_t)f->start;
  ensure_device(const_cast<wfst_fst*>(f));
  // ACCESSIBLE: every state reachable from the start (the DFS opens a new tree for any other state)
  const bool accessible = reach_from(ctx, n, f->dev.offsets, f->dev.arcs, s0).joined == n;
  // COACCESSIBLE: every state reaches a final one = reachable from the super-initial state 0 of the reversed FST
  const wfst_fst* r = reversed_handle(ctx, f);
  const bool coaccessible = reach_from(ctx, n + 1, r->dev.offsets, r->dev.arcs, 0).joined == n + 1;
  // CYCLIC: a back arc anywhere = a cycle anywhere: in-degree peeling leaves states behind exactly then
  bool cyclic;
  {
    DBuf<uint32_t> indeg(*ctx->pool, n);
    HIP_CHECK(hipMemsetAsync(indeg.p, 0, (size_t)n * sizeof(uint32_t), ctx->stream));
    count_indegrees(ctx, f->dev.arcs, f->n_arcs, indeg.p);
    cyclic = frontier_search(ctx, n, f->dev.offsets, f->dev.arcs, {}, indeg.p, 1).joined != n;
  }
  // INITIAL_CYCLIC: a back arc into the start = the start reachable from its own successors (search seeded with the start,
  // the start itself left unvisited)
  bool initial_cyclic;
  {
    DBuf<uint32_t> vis(*ctx->pool, n);
    HIP_CHECK(hipMemsetAsync(vis.p, 0, (size_t)n * sizeof(uint32_t), ctx->stream));
    frontier_search(ctx, n, f->dev.offsets, f->dev.arcs, {s0}, vis.p, 0);
    initial_cyclic = read_u32(ctx, vis.p + s0) != 0;
  }
  return props::dfs_bits(accessible, coaccessible, cyclic, initial_cyclic);
}

namespace {

// ---------------------------------------------------------------- reweight (reweight.rs:48-103)
// potentials pot[0..len); a state >= len has potential zero.  16 lanes per state: read the arc and the two potentials,
// write the arc with its new weight.  Per state s:  d_s zero -> the arcs stay (reweight.rs:64-66); per arc: d_ns zero -> the
// weight stays (:72-74); else ToInitial (w (x) d_ns) / d_s, ToFinal (d_s (x) w) / d_ns (:76-83), in that order of operations.
// facts: 1 = some arc went through set_weight_unchecked
__global__ void __launch_bounds__(256) reweight_arcs_kernel(const uint32_t* __restrict__ off, const wfst_tr* __restrict__ arcs,
                                                            uint32_t n, const float* __restrict__ pot, uint32_t len,
                                                            uint32_t to_final, wfst_tr* __restrict__ out,
                                                            uint32_t* __restrict__ facts_out) {
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lane = tid & 15u;
  uint32_t facts = 0;
  for (uint32_t s = tid >> 4; s < n; s += (gridDim.x * blockDim.x) >> 4) {
    const float d_s = s < len ? pot[s] : INF;
    const bool skip = is_zero(d_s);
    for (uint32_t i = off[s] + lane; i < off[s + 1]; i += 16) {
      wfst_tr a = arcs[i];
      if (!skip) {
        const float d_ns = a.nextstate < len ? pot[a.nextstate] : INF;
        if (!is_zero(d_ns)) {
          a.weight = to_final ? wdivide(wtimes(d_s, a.weight), d_ns) : wdivide(wtimes(a.weight, d_ns), d_s);
          facts |= 1u;
        }
      }
      out[i] = a;
    }
  }
  for (int d = 32; d >= 1; d >>= 1) facts |= __shfl_xor(facts, d);
  if ((threadIdx.x & 63) == 0 && facts) atomicOr(facts_out, facts);
}

// final weights (reweight.rs:42-53 for states >= len, :88-103), then, for push ToFinal with a total to remove,
// remove_weight's division (push.rs:155-162).  A final weight of +inf stands for None here; reweight never adds a final
// weight and every Some(zero) it produces is stored as +inf.
// facts: 2 = some final weight went through set_final.  last_op (push ToFinal): the highest (state + 1) << 1 | weighted(new)
// over the set_final_unchecked calls of remove_weight whose old or new weight is weighted — the call that decides WEIGHTED.
__global__ void reweight_finals_kernel(const float* __restrict__ fin, uint32_t n, const float* __restrict__ pot, uint32_t len,
                                       uint32_t to_final, float total, uint32_t remove, float* __restrict__ fout,
                                       uint32_t* __restrict__ facts_out, unsigned long long* __restrict__ last_op) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t facts = 0;
  unsigned long long op = 0;
  if (s < n) {
    float f = fin[s];
    if (f != INF) {
      const float d_s = s < len ? pot[s] : INF;
      if (to_final) {
        f = wtimes(f, d_s);  // s >= len: set_final(zero (x) f), then (x) zero again: +inf either way
        facts |= 2u;
        if (remove) {
          const float nf = wdivide(f, total);
          if (weighted(f) || weighted(nf)) op = ((unsigned long long)(s + 1) << 1) | (weighted(nf) ? 1ull : 0ull);
          f = nf;
        }
      } else if (!is_zero(d_s)) {
        f = wdivide(f, d_s);
        facts |= 2u;
      }
    }
    fout[s] = f;
  }
  for (int d = 32; d >= 1; d >>= 1) {
    facts |= __shfl_xor(facts, d);
    const unsigned long long o = __shfl_xor(op, d);
    op = o > op ? o : op;
  }
  if ((threadIdx.x & 63) == 0) {
    if (facts) atomicOr(facts_out, facts);
    if (op) atomicMax(last_op, op);
  }
}

// compute_total_weight, forward case (push.rs:128-141): (+)_s dist[s] (x) final[s] — the tropical sum is a minimum
__global__ void total_weight_kernel(const float* __restrict__ dist, const float* __restrict__ fin, uint32_t n,
                                    uint32_t* __restrict__ key_out) {
  uint32_t best = f32_key(INF);
  for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += gridDim.x * blockDim.x)
    best = min(best, f32_key(wtimes(dist[s], fin[s])));
  for (int d = 32; d >= 1; d >>= 1) best = min(best, (uint32_t)__shfl_xor(best, d));
  if ((threadIdx.x & 63) == 0) atomicMin(key_out, best);
}

__global__ void fill_kernel(float* __restrict__ p, uint32_t n, float v) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

// distances of f into d_dist[0..n) on the device: forward from the start, or (reverse) on reverse(f) with entry 0 dropped
void distances_device(wfst_ctx* ctx, const wfst_fst* f, bool reverse, DBuf<float>& buf, const float** d_dist) {
  const uint32_t n = f->n_states;
  if (!reverse) {
    buf = DBuf<float>(*ctx->pool, n);
    if (f->start < 0) {
      if (n) fill_kernel<<<(n + 255) / 256, 256, 0, ctx->stream>>>(buf.p, n, INF);
      HIP_CHECK(hipGetLastError());
    } else {
      shortest_distance_device(ctx, f, buf.p);
    }
    *d_dist = buf.p;
    return;
  }
  // shortest_distance_with_config(.., true, ..) (shortest_distance.rs:322-334): the reversed FST always starts at 0
  const wfst_fst* r = reversed_handle(ctx, f);
  buf = DBuf<float>(*ctx->pool, (size_t)n + 1);
  shortest_distance_device(ctx, r, buf.p);
  *d_dist = buf.p + 1;
}

struct Reweighted {
  uint32_t facts = 0;
  unsigned long long last_op = 0;
};

// reweight() of f with potentials pot[0..len) on the device, and for push_weights the total weight to remove; returns the
// NEW handle.  remove_total: 0 none, else remove_weight(total, at_final = to_final) after reweight (push.rs:107-118).
wfst_fst* reweight_device(wfst_ctx* ctx, const wfst_fst* f, const float* pot, uint32_t len, uint32_t to_final, bool remove_total,
                          float total) {
  ensure_device(const_cast<wfst_fst*>(f));
  const uint32_t n = f->n_states;
  const uint64_t E = f->n_arcs;
  hipStream_t st = ctx->stream;
  DevicePool& pool = *ctx->pool;
  // remove_weight does nothing when the total is one or zero (push.rs:150-152)
  const bool remove = remove_total && !is_one(total) && !is_zero(total);
  ctx->push_stats.removed = remove ? 2 : remove_total ? 1 : 0;
  // room for the state reweight may add (reweight.rs:129-138)
  DBuf<uint32_t> off_out(pool, (size_t)n + 2);
  DBuf<wfst_tr> arcs_out(pool, E + 1);
  DBuf<float> fin_out(pool, (size_t)n + 1);
  DBuf<uint32_t> facts(pool, 4);
  HIP_CHECK(hipMemsetAsync(facts.p, 0, 4 * sizeof(uint32_t), st));
  unsigned long long* last_op = (unsigned long long*)(facts.p + 2);
  HIP_CHECK(hipMemcpyAsync(off_out.p, f->dev.offsets, ((size_t)n + 1) * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  if (n && E) {
    const uint32_t blocks = strided_grid(ctx, (n + 15) / 16, ARCS_BLOCKS_PER_CU);
    reweight_arcs_kernel<<<blocks, 256, 0, st>>>(f->dev.offsets, f->dev.arcs, n, pot, len, to_final, arcs_out.p, facts.p);
    HIP_CHECK(hipGetLastError());
    ctx->push_stats.arcs_blocks = blocks;
  }
  if (n) {
    reweight_finals_kernel<<<(n + 255) / 256, 256, 0, st>>>(f->dev.finals, n, pot, len, to_final, total,
                                                            (remove && to_final) ? 1u : 0u, fin_out.p, facts.p, last_op);
    HIP_CHECK(hipGetLastError());
  }
  Reweighted rw;
  uint32_t h_facts[4] = {0, 0, 0, 0};
  HIP_CHECK(hipMemcpyAsync(h_facts, facts.p, sizeof(h_facts), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  rw.facts = h_facts[0];
  std::memcpy(&rw.last_op, h_facts + 2, 8);

  // ---- the property word through the reference's mutations, in its order
  uint64_t p = f->props;
  // set_final (reweight.rs:46-49, 101) and set_weight_unchecked (:84): masks (their WEIGHTED / UNWEIGHTED updates are
  // dropped by reweight_properties below)
  p = props::reweight_marks(p, rw.facts);
  int64_t start = f->start;
  uint32_t n_out = n;
  uint64_t e_out = E;
  // ---- the start state (reweight.rs:105-146): runs when d[start] is neither one nor zero (approximate ==)
  float d_start = INF;
  if (start >= 0 && (uint64_t)start < len)
    HIP_CHECK(hipMemcpy(&d_start, pot + start, sizeof(float), hipMemcpyDeviceToHost));
  // the start's arc list and final weight as the kernels left them (host copies: one state)
  std::vector<wfst_tr> sarcs;
  uint32_t sb = 0;
  float sfin = INF;
  auto fetch_start = [&](uint32_t s) {
    uint32_t be[2];
    HIP_CHECK(hipMemcpy(be, off_out.p + s, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    sb = be[0];
    sarcs.resize(be[1] - be[0]);
    if (!sarcs.empty())
      HIP_CHECK(hipMemcpy(sarcs.data(), arcs_out.p + sb, sarcs.size() * sizeof(wfst_tr), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(&sfin, fin_out.p + s, sizeof(float), hipMemcpyDeviceToHost));
  };
  bool start_dirty = false;
  if (start >= 0 && !is_one(d_start) && !is_zero(d_start)) {
    // compute_and_update_properties(INITIAL_ACYCLIC) (:109): the stored bit if the word knows it, else the DFS bits
    if (!props::knows(p, props::INITIAL_CYCLIC)) p = props::merge_dfs(p, structural_bits(ctx, f));
    // (ToFinal: one / d_s = 0 - d_s)
    const float factor = to_final ? wdivide(0.0f, d_start) : d_start;
    if (p & props::INITIAL_ACYCLIC) {  // (:111-128) the start's arcs and final weight
      fetch_start((uint32_t)start);
      for (wfst_tr& a : sarcs) {
        a.weight = wtimes(factor, a.weight);
        p = p & props::ARC_RELEVANT;
      }
      if (sfin != INF) {
        sfin = wtimes(factor, sfin);
        p = props::set_final(p, nullptr, nullptr);
      }
      start_dirty = true;
      ctx->push_stats.start_branch = 1;
    } else {  // (:129-138) a new start state n with one eps:eps arc into the old start
      const wfst_tr a{0u, 0u, factor, (uint32_t)start};
      p = props::add_state(p);
      p = props::add_tr(p, n, a, nullptr);
      p = props::set_start(p);
      const uint32_t ends[1] = {(uint32_t)E + 1};
      HIP_CHECK(hipMemcpy(off_out.p + n + 1, ends, sizeof(uint32_t), hipMemcpyHostToDevice));
      HIP_CHECK(hipMemcpy(arcs_out.p + E, &a, sizeof(wfst_tr), hipMemcpyHostToDevice));
      const float none = INF;
      HIP_CHECK(hipMemcpy(fin_out.p + n, &none, sizeof(float), hipMemcpyHostToDevice));
      start = n;
      n_out = n + 1;
      e_out = E + 1;
      ctx->push_stats.start_branch = 2;
    }
  }
  p = props::reweight(p);  // (:148-151)
  // ---- remove_weight (push.rs:147-170)
  if (remove && to_final) {  // every Some(final weight) divided (the kernel did it); set_final_unchecked's bookkeeping
    if (rw.facts & 2u) {
      p = props::set_final(p, nullptr, nullptr);
      if (rw.last_op) p = (rw.last_op & 1ull) ? ((p | props::WEIGHTED) & ~props::UNWEIGHTED) : (p & ~props::WEIGHTED);
    }
  } else if (remove && start >= 0) {  // the (possibly new) start state's arcs, then its final weight
    if (!start_dirty) fetch_start((uint32_t)start);
    for (wfst_tr& a : sarcs) {
      const float w = wdivide(a.weight, total);
      p = props::set_weight(p, a.weight, w);
      a.weight = w;
    }
    if (sfin != INF) {
      const float w = wdivide(sfin, total);
      p = props::set_final(p, &sfin, &w);
      sfin = w;
    }
    start_dirty = true;
  }
  if (start_dirty) {
    if (!sarcs.empty())
      HIP_CHECK(hipMemcpy(arcs_out.p + sb, sarcs.data(), sarcs.size() * sizeof(wfst_tr), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(fin_out.p + start, &sfin, sizeof(float), hipMemcpyHostToDevice));
  }
  return adopt_device(ctx, n_out, e_out, start, p & props::ALL, off_out.p, arcs_out.p, fin_out.p);
}

wfst_fst* empty_copy(wfst_ctx* ctx, const wfst_fst* f) {  // an FST without states comes back as it is
  HostCsr h;
  h.offsets.push_back(0);
  return make_host_fst(ctx, 0, -1, f->props & props::ALL, std::move(h));
}

}  // namespace

// shortest_distance_with_config(fst, reverse, ..) (shortest_distance.rs:313-336): distance[0..n) (+inf past the reference's
// Vec), *len = that Vec's length: one plus the largest state id the search touches.  The search relaxes every arc of every
// state it dequeues and dequeues every state reachable from its source (an unreached target is "improved" even by an
// infinite weight: approx_equal(inf, inf) is false, |inf - inf| = NaN), so the length comes from plain reachability.
void shortest_distance_ex(wfst_ctx* ctx, const wfst_fst* f, bool reverse, float* distance, uint32_t* len) {
  const uint32_t n = f->n_states;
  if (!reverse) {
    shortest_distance(ctx, f, distance, nullptr);  // exactly wfst_shortest_distance
    if (len) {
      *len = 0;
      if (f->start >= 0 && n) {
        ensure_device(const_cast<wfst_fst*>(f));
        *len = reach_from(ctx, n, f->dev.offsets, f->dev.arcs, (uint32_t)f->start).maxid;
      }
    }
    return;
  }
  if (n == 0) {  // reverse(empty) = one super-initial state: rdistance = [one], distance = []
    if (len) *len = 0;
    return;
  }
  DBuf<float> buf;
  const float* d = nullptr;
  distances_device(ctx, f, true, buf, &d);
  HIP_CHECK(hipMemcpyAsync(distance, d, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  if (len) {  // rdistance.len() - 1: the largest reversed state reached (state s + 1 of reverse(f) is s)
    const wfst_fst* r = reversed_handle(ctx, f);
    const Search s = reach_from(ctx, n + 1, r->dev.offsets, r->dev.arcs, 0);
    *len = s.maxid - 1;
  }
}

wfst_fst* reweight_fst(wfst_ctx* ctx, const wfst_fst* f, const float* potentials, uint64_t n_potentials, uint32_t reweight_type) {
  const uint32_t n = f->n_states;
  if (n == 0) return empty_copy(ctx, f);  // (reweight.rs:37-39)
  const uint32_t len = (uint32_t)std::min<uint64_t>(n_potentials, n);  // (entries past the last state are never read)
  DBuf<float> pot(*ctx->pool, std::max<uint32_t>(len, 1));
  if (len) HIP_CHECK(hipMemcpyAsync(pot.p, potentials, (size_t)len * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  return reweight_device(ctx, f, pot.p, len, reweight_type, false, 0.0f);
}

// push_weights_with_config (push.rs:89-118): distances towards the side weights are pushed to (reverse ones for
// ToInitial), the total weight from the ORIGINAL FST, reweight, then remove_weight.  The potentials are the whole distance
// array (+inf past the reference's Vec): reweight treats a state >= potentials.len() exactly as one whose potential is zero.
wfst_fst* push_weights_fst(wfst_ctx* ctx, const wfst_fst* f, uint32_t reweight_type, bool remove_total_weight) {
  const uint32_t n = f->n_states;
  if (n == 0) return empty_copy(ctx, f);
  ensure_device(const_cast<wfst_fst*>(f));
  const bool to_final = reweight_type == 1;
  DBuf<float> buf;
  const float* d = nullptr;
  distances_device(ctx, f, !to_final, buf, &d);
  float total = INF;
  if (remove_total_weight) {
    if (!to_final) {  // dist[start], or zero without a start (push.rs:122-127)
      if (f->start >= 0) HIP_CHECK(hipMemcpy(&total, d + f->start, sizeof(float), hipMemcpyDeviceToHost));
    } else {
      DBuf<uint32_t> key(*ctx->pool, 1);
      const uint32_t kinf = f32_key(INF);  // zero
      HIP_CHECK(hipMemcpyAsync(key.p, &kinf, sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
      const uint32_t blocks = strided_grid(ctx, (n + 255) / 256, TOTAL_BLOCKS_PER_CU);
      total_weight_kernel<<<blocks, 256, 0, ctx->stream>>>(d, f->dev.finals, n, key.p);
      HIP_CHECK(hipGetLastError());
      ctx->push_stats.total_blocks = blocks;
      total = key_f32(read_u32(ctx, key.p));
    }
  }
  return reweight_device(ctx, f, d, n, reweight_type, remove_total_weight, total);
}

}  // namespace wfst
