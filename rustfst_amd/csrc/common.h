// common.h — shared host-side definitions of libwfst_amd (context, FST handle, device pool, errors).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/wfst.h"
#include "tropical.h"

extern "C" char** environ;

namespace wfst {

// one turn of a host spin loop on a word in pinned memory (the completion tickets)
inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
  __builtin_ia32_pause();
#elif defined(__aarch64__)
  asm volatile("yield" ::: "memory");
#else
  asm volatile("" ::: "memory");
#endif
}

// The WFST_* variables of the process as they stand now: ONE pass over `environ` instead of one getenv (each a walk over
// the whole environment of a Python / torch process) per variable.  Taken at the start of a solve or a batch call and
// asked from then on; get() is getenv() for names that begin with "WFST_" — null when the variable is not set.
// The values point into the environment, like getenv's: valid until somebody changes the variable.
class EnvSnap {
 public:
  EnvSnap() = default;
  static EnvSnap take();
  const char* get(const char* name) const {
    if (vars_.empty()) return nullptr;
    const size_t len = std::strlen(name);
    for (const char* e : vars_)
      if (std::strncmp(e, name, len) == 0 && e[len] == '=') return e + len + 1;
    return nullptr;
  }
  bool has(const char* name) const { return get(name) != nullptr; }

 private:
  std::vector<const char*> vars_;  // "WFST_NAME=value" entries
};
inline EnvSnap EnvSnap::take() {
  EnvSnap s;
  if (environ)
    for (char** e = environ; *e; ++e)
      if ((*e)[0] == 'W' && std::strncmp(*e, "WFST_", 5) == 0) s.vars_.push_back(*e);
  return s;
}

// ---------------------------------------------------------------- errors
struct Error : std::runtime_error {
  using std::runtime_error::runtime_error;
};
void set_last_error(const std::string& msg);

// a WFST_*_PATH variable (tests): which of an operation's two level routes may run
enum class Path { Auto, Narrow, Wide };
static inline Path path_knob(const char* var) {  // (internal linkage: no exported symbol)
  const char* e = std::getenv(var);
  if (!e || !*e || !std::strcmp(e, "auto")) return Path::Auto;
  if (!std::strcmp(e, "narrow")) return Path::Narrow;
  if (!std::strcmp(e, "wide")) return Path::Wide;
  throw Error(std::string(var) + ": expected auto, narrow or wide, not '" + e + "'");
}

#define HIP_CHECK(expr)                                                                                  \
  do {                                                                                                   \
    hipError_t _e = (expr);                                                                              \
    if (_e != hipSuccess)                                                                                \
      throw ::wfst::Error(std::string("HIP error ") + hipGetErrorString(_e) + " at " __FILE__ ":" +     \
                          std::to_string(__LINE__) + " in " #expr);                                      \
  } while (0)

template <class F>
wfst_status wrap(F&& f) noexcept {  // rustfst-ffi/src/lib.rs:43-56 `wrap`
  try {
    f();
    return WFST_OK;
  } catch (const std::exception& e) {
    set_last_error(e.what());
    return WFST_KO;
  } catch (...) {
    set_last_error("unknown error");
    return WFST_KO;
  }
}

// ---------------------------------------------------------------- device memory pool
// Size-bucketed caching allocator: hot paths never call hipMalloc/hipFree after warm-up.  Thread-safe: an FST shared
// by several contexts (threads) may grow its cached derived data from any of them.
class DevicePool {
 public:
  explicit DevicePool(int device) { (void)device; }
  ~DevicePool();
  void* alloc(size_t bytes);
  void free(void* p);
  void trim();
  // Parked blocks: live blocks set aside with their contents for a later owner (the re-armed scratch of a relaxation, which a
  // kernel may still be writing when its solve lets go of it: wfst_ctx::rearm).  Out of alloc's reach; trim (the out-of-memory
  // retry included) and the destructor hipFree them like cached blocks — hipFree synchronises the device, so a kernel that still
  // writes one is over first — and the unpark that follows reports them gone.  All of `ps` or none, under one lock.
  void park(void* const* ps, size_t count);
  bool unpark(void* const* ps, size_t count);  // live again, as alloc would have returned them; false: reclaimed (none is live)

 private:
  static size_t bucket(size_t bytes);
  void trim_locked();
  std::mutex mu_;
  std::multimap<size_t, void*> free_;
  std::map<void*, size_t> live_;
  std::map<void*, size_t> parked_;
};

// RAII device buffer from the pool
template <class T>
struct DBuf {
  DevicePool* pool = nullptr;
  T* p = nullptr;
  size_t n = 0;
  DBuf() = default;
  DBuf(DevicePool& pl, size_t count) : pool(&pl), p((T*)pl.alloc(std::max<size_t>(count, 1) * sizeof(T))), n(count) {}
  DBuf(const DBuf&) = delete;
  DBuf& operator=(const DBuf&) = delete;
  DBuf(DBuf&& o) noexcept : pool(o.pool), p(o.p), n(o.n) { o.p = nullptr; }
  DBuf& operator=(DBuf&& o) noexcept {
    reset();
    pool = o.pool;
    p = o.p;
    n = o.n;
    o.p = nullptr;
    return *this;
  }
  void reset() {
    if (p) pool->free(p);
    p = nullptr;
  }
  // a live block of the pool that somebody else allocated (DevicePool::unpark), and the way out again (DevicePool::park)
  static DBuf adopt(DevicePool& pl, void* block, size_t count) {
    DBuf b;
    b.pool = &pl;
    b.p = (T*)block;
    b.n = count;
    return b;
  }
  T* release() {
    T* r = p;
    p = nullptr;
    return r;
  }
  ~DBuf() { reset(); }
};

// pinned host staging buffer (grow-only)
struct PinnedBuf {
  void* p = nullptr;
  size_t cap = 0;
  void* get(size_t bytes);
  ~PinnedBuf();
};

// Pinned host blocks handed out by reference count: the kernel of a fused batch writes its results and path arcs into one,
// and the path FSTs the batch returns point into it (wfst_fst::path_form) until somebody asks for their arrays.  The
// block goes back to the ring when the job and every such result are gone (a serving loop alternates between two).
struct PinnedBlock {
  void* p = nullptr;
  size_t cap = 0;
};
class PinnedRing : public std::enable_shared_from_this<PinnedRing> {
 public:
  std::shared_ptr<PinnedBlock> take(size_t bytes);
  ~PinnedRing();

 private:
  std::mutex mu_;
  std::vector<PinnedBlock*> free_;
};

struct MboxPlan;
// The scratch of a mailbox relaxation that the re-arm launch behind the solve's tail has cleaned (or is cleaning) for the next
// solve on this context (sssp.hip: relax_setup adopts it, shortest_path_n1_end parks it).  Nothing here refers to a handle by
// address — a destroyed handle's address can be reused; the plan cannot while the record holds it.
struct RearmRecord {
  std::shared_ptr<DevicePool> plan_pool;  // the pool the plan's tables came from (the handle's owner's): outlives the plan
  std::shared_ptr<MboxPlan> plan;         // identity of the graph's structure (null: nothing parked)
  uint32_t n = 0, log = 0, stg = 0, tau0_bits = 0;
  bool resident = false, narrow = false;
  static constexpr size_t BLOCKS = 6;  // key, mb_words, improved, ctl, rs_msgs, rs_abort (null: the solve had none)
  void* blk[BLOCKS] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  size_t cnt[BLOCKS] = {0, 0, 0, 0, 0, 0};
  // The solo query (sssp_solo.h) answers from this scratch without adopting it.  `solo`: what the solve that parked it was planned
  // under (sssp.hip SoloArm; null: that solve was not one a bounded head may end); `stops`: the queries in a row up to the one
  // that parked it that a bounded head or the solo kernel ended on this context; `epoch`: wfst_fst::sp_epoch as the last of them
  // left it — any other single-path query of the handle since, from whatever context, shows there.
  std::shared_ptr<void> solo;
  uint32_t stops = 0;
  uint64_t epoch = 0;
  void clear() {  // (the plan goes before its pool)
    solo.reset();
    stops = 0;
    epoch = 0;
    plan.reset();
    plan_pool.reset();
    for (void*& b : blk) b = nullptr;
    for (size_t& c : cnt) c = 0;
  }
};
// Route counters: host-side tallies that say which kernel route a call took.  One struct per family, uint64_t fields only, declared
// in the order of the family's wfst_ctx_get_*_stats parameters (include/wfst.h) and named exactly as they are: api.cpp copies a
// family out by position, tests/test_host.py compares the names.  Each comment says when the family is zeroed.
// One call of a one-workgroup-per-item batch operation; zeroed when that call begins, also when an argument is refused.
struct BatchStats {
  uint64_t launches = 0, items_in_kernel = 0, items_single = 0;
};
// One wfst_optimize_batch call, zeroed like BatchStats; launches per stage: rm_epsilon, tr_sum, determinize, minimize
struct OptimizeBatchStats {
  uint64_t launches[4] = {0, 0, 0, 0};
  uint64_t items_in_kernel = 0, items_single = 0, items_transducer = 0;
};
// The last wfst_fst_count_paths / wfst_fst_paths / wfst_fst_paths_batch call (paths.hip; wfst_ctx_get_paths_counters): kernel
// launches and library calls (a rocPRIM sort or scan counts one) of the call; items counted by the one-workgroup kernel (those
// without a start state among them) and by the device-wide route; the deepest peel of an item; the paths counted (saturating,
// up to and including a refused item); the arcs of the longest path of the table; items whose count saturated.  Zeroed when
// the call begins, also when an argument is refused.
struct PathsCounters {
  uint64_t launches = 0, items_in_kernel = 0, items_single = 0, levels = 0, paths = 0, max_path_arcs = 0, saturated = 0;
};
}  // namespace wfst

// ---------------------------------------------------------------- handles
struct wfst_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool owns_stream = false;
  // shared with every FST handle created on this context (and its arenas): the device memory of a handle that outlives
  // its context (interpreter shutdown destroys in any order) is still released to a live pool, which goes with the last owner
  std::shared_ptr<wfst::DevicePool> pool;
  wfst::PinnedBuf pinned;      // small D2H/H2D staging
  wfst::PinnedBuf pinned_big;  // batch descriptors / results
  bool profiling = false;
  bool tie_reference = false;  // wfst_ctx_set_tie_order: the reference's predecessor choice on acyclic inputs
  uint32_t resident_share = 0; // wfst_ctx_set_resident_share: 0 = resident launches may fill the device, 1 = at most half of it
  // A resident relaxation launch of this context gave up waiting (its grid was not resident as a whole: another tenant held
  // compute units): solves take one launch per level until `resident_retry_at`, then a resident launch is tried again;
  // the pause doubles with every abort in a row (50 ms .. 3.2 s) and is forgotten by the first resident solve that completes.
  int64_t resident_retry_at_ns = 0;  // steady clock; 0 = resident launches allowed
  bool resident_hold = false;        // the repeat of a solve whose resident launch gave up: never a resident one
  uint32_t resident_abort_streak = 0;
  bool resident_allowed() const;
  void resident_aborted(int64_t fixed_pause_ms);  // (< 0: the doubling pause; tests fix it)
  void resident_completed() { resident_abort_streak = 0; }
  // wfst_ctx_set_profiling(ctx, 2): no per-launch events; the sweeps of a repeated (predicted) shortest_path query are timed
  // as ONE chain between two events on the stream, without any synchronisation between launches
  bool chain_timing = false;
  hipEvent_t ev_chain[2] = {nullptr, nullptr};
  bool batch_in_flight = false;  // wfst_compose_shortest_path_batch_begin .. _end
  bool sp_in_flight = false;     // wfst_shortest_path_begin .. _end
  wfst_stats stats{};
  struct SweepSample {
    double ms;
    uint64_t arcs, states;
    uint32_t mode = 0;  // what ran the level (Ctl::mode of its slot): mailbox MODE_*, or 0 atomic sweep / 7 binned level
  };
  std::vector<SweepSample> sweep_trace;  // profiling only: one entry per relaxation launch of the last solve
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  wfst::PinnedBuf pinned_flags;  // host mirror of the per-sweep activity flags: [0] first batch of a solve, [1] batches of 8 sweeps, [2] of 64
  std::shared_ptr<wfst::PinnedRing> pinned_ring = std::make_shared<wfst::PinnedRing>();  // result blocks of the fused batches
  // ---- route counters (the rules: wfst::BatchStats above).  The last wfst_determinize_batch / wfst_determinize_with_distance_batch,
  // wfst_minimize_batch, wfst_rm_epsilon_batch, wfst_tr_sum_batch / wfst_tr_unique_batch, wfst_top_sort_batch and
  // wfst_optimize_batch call (batch_driver.h counts)
  wfst::BatchStats det_batch, min_batch, rm_batch, trsum_batch, top_sort_batch;
  wfst::OptimizeBatchStats opt_batch;
  // Which route the levels of the last wfst_determinize / wfst_determinize_with_distance call took: tallied on the host from
  // the control block determinize.hip already reads back.  Zeroed when determinize.hip's driver begins.
  struct DeterminizeStats {
    uint64_t levels = 0, wide_levels = 0, narrow_launches = 0;
    uint64_t exit_wide_states = 0, exit_wide_cands = 0, exit_budget = 0, exit_need = 0, exit_done = 0, wide_need = 0;
    uint64_t grow_states = 0, grow_elts = 0, grow_arcs = 0, grow_cands = 0, rehashes = 0;
    uint64_t cap_states = 0, cap_elts = 0, cap_arcs = 0, cap_cands = 0;
    uint64_t rounds_max = 0;
  } det_stats;
  // Which route the last wfst_minimize call took: tallied on the host from the control block minimize.hip's level loop already
  // reads back; check = the cycle check on the untrimmed input, refine = the refinement of the connected machine.  Zeroed when
  // wfst_minimize begins, also when an argument is refused, and when minimize.hip's driver begins.
  struct MinimizeStats {
    // flat: check_levels, check_wide_levels, check_narrow_launches, check_exit_wide, check_exit_done, levels, wide_levels,
    //       narrow_launches, exit_wide, exit_done, branch, wave_states, unequal_compares
    struct Pass {
      uint64_t levels = 0, wide_levels = 0, narrow_launches = 0, exit_wide = 0, exit_done = 0;
    } check, refine;
    uint64_t branch = 0, wave_states = 0, unequal_compares = 0;
  } min_stats;
  // The route of the last wfst_shortest_distance_with_config / wfst_reweight / wfst_push_weights call: tallied on the host by
  // push.hip from its launch geometry, its loop counter and the values it reads back anyway.  Zeroed when one of the three
  // begins, also when an argument is refused.
  struct PushStats {
    uint64_t searches = 0, rounds = 0, reads = 0, rounds_max = 0;
    uint64_t bfs_blocks = 0, arcs_blocks = 0, total_blocks = 0;
    uint64_t structural = 0, start_branch = 0, removed = 0;
  } push_stats;
  // The one-wave path kernels.  n1_*: the last sp1_wave_kernel launch since the last wfst_shortest_path /
  // wfst_shortest_path_batch call began — zeroed when either begins (small_path_begin, api.cpp) and before each such launch is
  // counted; nbest_*: the last shortest_path_nbest_batch, zeroed when it begins.
  struct SmallPathStats {
    uint64_t n1_in_kernel = 0, n1_staged = 0, n1_handed_back = 0;
    uint64_t nbest_in_kernel = 0, nbest_tree_full = 0, nbest_out_full = 0, nbest_tree_capacity = 0;
  } small_path;
  // Which route answered the problems of the last compose / fused-batch call: tallied on the host from the status words the
  // kernels of compose.hip already report.  Zeroed when either call begins.
  struct ComposePathStats {
    uint64_t string_answered = 0, string_handed_back = 0, wave_first = 0;
    uint64_t relaunch_states = 0, relaunch_arcs = 0, relaunch_hash = 0, relaunch_path = 0;
    uint64_t switched_wide = 0, two_step = 0;
    uint64_t caps_states = 0, caps_arcs = 0, caps_hash = 0;  // Caps of the last compose_wave_kernel launch
  } compose_path;
  // The chase runs of the string o T kernel in the last fused-batch call: levels taken inside runs and the number of runs,
  // summed over the problems the kernel answered.  Zeroed when the fused-batch call begins.
  struct StringRunStats {
    uint64_t run_levels = 0, runs = 0;
  } string_run;
  // The pair levels of the same kernel in the same call (compose.hip, wfst_ctx_get_string_pair_counts): levels its run loop
  // carried that are not run levels — a frontier of two states, or one state that matches two arcs — and those of them with
  // two matches.  Tallied and zeroed where string_run is.
  struct StringPairCounts {
    uint64_t pair_levels = 0, pair_splits = 0;
  } string_pair;
  // Where the waves of this context's last string launch sat (string_placement.h; wfst_ctx_get_string_placement, defined in
  // compose.hip): string_compose_sp_kernel in a fused-batch call, string_sigma_sp_kernel in one with matcher configs.
  // packed_for_resident, forced: 0 / 1.  Zeroed where string_run is, and where sigma_batch is.
  struct StringPlacementCounts {
    uint64_t waves_per_workgroup = 0, slice_states = 0, workgroups = 0, packed_for_resident = 0, forced = 0;
  } string_placement;
  // The last wfst_rm_epsilon call; zeroed when rm_epsilon.hip's driver begins.
  struct RmEpsilonStats {
    uint64_t batches = 0, thread_launches = 0, wave_launches = 0, states_thread = 0, states_wave = 0, max_closure_cap = 0;
  } rm_eps;
  // The last wfst_top_sort call: tallied on the host by top_sort.hip from its launches, the level bounds and the three words it
  // reads back anyway.  Zeroed when top_sort.hip's driver begins.
  struct TopSortStats {
    uint64_t levels = 0, narrow_launches = 0, wide_launches = 0, narrow_levels = 0, max_level_width = 0, max_tree_depth = 0;
    uint64_t lift_rows = 0, states_compared = 0, wave_states = 0, cyclic = 0;
  } top_sort;
  // Which route answered the compositions of the last wfst_compose_lookahead / wfst_compose_lookahead_batch call: tallied on the
  // host by compose_lookahead.hip from the LaResult words its kernel already reports and from what the wide driver returns.
  // handed_over_states / _width: LA_SWITCH_WIDE with n_states above the state limit in force / otherwise; wave_regrows: arena
  // attempts under WFST_LOOKAHEAD_PATH=wave; one_limits: 1 when the limits of a call with ONE composition applied.  Zeroed when
  // the driver begins.
  struct LookaheadStats {
    uint64_t items = 0, items_no_start = 0, wave_answered = 0, handed_over_states = 0, handed_over_width = 0;
    uint64_t overflow_arcs = 0, overflow_states = 0, wide_items = 0, wave_regrows = 0, wide_grows = 0, wide_hinted = 0;
    uint64_t hint_fallbacks = 0, one_limits = 0;
  } lookahead;
  // The last wfst_replace call: the driver's level and size figures, the counters of replace.hip's policy block, and the two
  // kinds of growth (the driver's arena in place, the prefix table by a rerun).  Zeroed when replace.hip's driver begins.
  struct ReplaceStats {
    uint64_t levels = 0, states = 0, arcs = 0, prefixes = 0, max_depth = 0, call_arcs = 0, dropped_calls = 0, return_arcs = 0;
    uint64_t arena_grows = 0, prefix_reruns = 0, level_launches = 0;
  } replace;
  // The last wfst_compose_with_matchers call that had a matcher config: the driver's level and size figures, then the counters
  // of compose_sigma.hip's policy block — composed states whose side-1 / side-2 state carries a sigma arc, items of a sigma
  // side that the sorted matcher answered, that the sigma arcs answered, the arcs those emitted, items the allowed set refused
  // (a level that is emitted again after an overflow counts its items again) — and the arena's growths.  Zeroed when
  // compose_sigma.hip's driver begins; all 0 after a KO, except the growths.
  struct ComposeSigmaStats {
    uint64_t levels = 0, states = 0, arcs = 0, require1_states = 0, require2_states = 0, exact_items = 0, sigma_items = 0;
    uint64_t sigma_arcs = 0, refused_items = 0, arena_grows = 0, level_launches = 0;
  } compose_sigma;
  // The last wfst_compose_shortest_path_batch_with_matchers call that had a matcher config (compose_sigma_batch.hip): launches
  // of string_sigma_sp_kernel, items it answered, items it handed back (a level wider than one wave, or more composed states
  // than its slice of LDS holds), items that were never sent to it, the four item counters of ComposeSigmaStats summed over
  // the items the kernel answered, and the widest level among those.  Zeroed when the call begins.
  struct SigmaBatchCounters {
    uint64_t launches = 0, items_in_kernel = 0, items_handed_back = 0, items_loop = 0, exact_items = 0, sigma_items = 0;
    uint64_t sigma_arcs = 0, refused_items = 0, max_level_width = 0;
  } sigma_batch;
  // The last wfst_compose_batch call (compose.hip; wfst_ctx_get_compose_batch_counters): batch_driver.h's three counts, then
  // the items without a start state on either side (they are among items_in_kernel), and per item and attempt the overflows
  // that reopened an item with four times the capacities.  Zeroed when the call begins, behind every check that needs no launch.
  struct ComposeBatchCounters : wfst::BatchStats {
    uint64_t items_no_start = 0, regrown_states = 0, regrown_arcs = 0, regrown_hash = 0;
  } compose_batch;
  // The last wfst_isomorphic call (isomorphic.hip; wfst_ctx_get_isomorphic_counters): levels of the search that ran, launches of
  // the one-workgroup kernel and of the device-wide phase kernels, levels the former ran, the widest level, pairs and arc
  // slots of the levels that ran, pairs walked by a wave, states of both operands sorted by the radix route, mark atomics.
  // Zeroed when the call has passed its checks.
  struct IsomorphicCounters {
    uint64_t levels = 0, narrow_launches = 0, wide_launches = 0, narrow_levels = 0, max_level_width = 0, pairs = 0, events = 0;
    uint64_t wave_pairs = 0, big_states_sorted = 0, nondet_marks = 0;
  } isomorphic;
  wfst::PathsCounters paths;
  int n_cus = 256;
  wfst::RearmRecord rearm;  // the parked scratch of this context's last predicted mailbox solve
  // ... and what became of such scratch; never zeroed (counts since the context's creation)
  struct RearmStats {
    uint64_t armed = 0, adopted = 0, dropped = 0;
  } rearm_stats;
  // The bounded head of the single-shortest-path relaxation (wfst_ctx_get_bounded_stats, with bounded_last_refusal as its
  // last_reason): queries it ended and queries that ran the full solve; never zeroed.  bounded_last_refusal: why the last of
  // those did (a string literal); bounded_hold: the query being repeated may not stop
  struct BoundedStats {
    uint64_t stops = 0, full_solves = 0;
  } bounded;
  const char* bounded_last_refusal = "";
  bool bounded_hold = false;
  // The solo query (sssp_solo.h; wfst_ctx_get_solo_query, defined in sssp.hip): launches of its kernel, those that answered,
  // those that gave the query up, why the last of those did (0 = none yet, 1 BAND, 2 GREW, 3 LOG, 4 OTHER), and the keys the
  // last launch put back; never zeroed.  solo_hold: the query being repeated by the ordinary route behind such an abort;
  // solo_log: the kernel's log of the keys it wrote (device memory, allocated by the first attempt)
  struct SoloQueryCounts {
    uint64_t attempts = 0, answered = 0, aborted = 0, last_abort = 0, cleaned = 0;
  } solo_query;
  bool solo_hold = false;
  wfst::DBuf<uint32_t> solo_log;
};

// Device-resident CSR. All arrays live in one arena allocation that may be
// shared between several FSTs (wfst_fst_upload_many).
struct DeviceArena {
  std::shared_ptr<wfst::DevicePool> pool;
  void* base = nullptr;
  size_t bytes = 0;
  ~DeviceArena();
};

struct DeviceCsr {
  std::shared_ptr<DeviceArena> arena;
  const uint32_t* offsets = nullptr;  // [n+1]
  const wfst_tr* arcs = nullptr;      // [E] AoS 16 B == CTr == on-disk arc
  const float* finals = nullptr;      // [n], +inf = non-final
  const uint32_t* noeps = nullptr;    // [n] number of output-epsilon arcs (VectorFstState.noepsilons)
  const uint2* wn = nullptr;          // [E] packed {weight bits, nextstate}: the 8 B the relaxation needs
  const uint4* srec = nullptr;        // [n] {arc begin, arc count, final bits, SREC_* epsilon facts}: one 16-B load per state in compose
};

namespace wfst {
// reverse(fst) (reverse.rs:33-87) for the n-best search: state 0 = super-initial (one eps arc per final state of fst, in
// state order, kept on the host), state t+1 = the in-arcs of t in reverse()'s order.  The in-arc segments live on the
// host for small FSTs; for large ones they STAY in HBM and the host search fetches the few segments it visits.
struct RevFst {
  uint32_t n = 0;                 // states of the original FST
  std::vector<wfst_tr> super;     // arcs of state 0
  std::vector<float> finals;      // [n+1] final weights of rfst (+inf = none)
  bool on_host = true;
  std::vector<uint32_t> h_roff;   // [n+1] segment offsets (on_host)
  std::vector<wfst_tr> h_arcs;    // [E]
  DBuf<uint32_t> d_roff;          // same on the device (!on_host)
  DBuf<wfst_tr> d_arcs;
  uint64_t fetched_segments = 0;  // statistics
};
struct RevCsr {
  DBuf<uint32_t> off;  // [n+1]
  DBuf<uint4> arc;     // [E] {source state, position of the arc in the source's arc list, weight bits, 0}
  // The final states as {state, final weight bits}, in state order: what the tail of a query reads instead of all of
  // `finals`.  Only for a small, sparse final set (sssp.hip final_list_build); has_fin false = none, the tail scans.
  // Independent of the start state, like the transpose: wfst_fst_set_start keeps both.
  DBuf<uint2> fin;
  uint32_t n_fin = 0;
  bool has_fin = false;
  bool fin_nonneg = false;  // no final weight of the list is negative (what the early tail of a query needs)
};
// Message-region plan of the mailbox relaxation sweeps (sssp_mailbox.h): offsets of the region reserved for every
// (source block, destination block) pair, sized by the number of arcs between the two blocks.
struct MboxPlan {
  uint32_t nb = 0;         // blocks of 1 << log states
  uint32_t log = 12;
  DBuf<uint32_t> roff;     // [nb*nb + 1] destination-major
  DBuf<uint32_t> roff_t;   // [nb*nb]     source-major copy
  // regions of the resident kernel (sssp_resident.h): 16-byte header + one slot per arc, 64-byte aligned, in 8-byte units
  DBuf<uint32_t> roffh;    // [nb*nb + 1] destination-major
  DBuf<uint32_t> roffh_t;  // [nb*nb]     source-major copy
  uint64_t res_units = 0;  // units of one parity buffer
  uint32_t lps = 8;        // lanes per listed state of the resident kernel's expansion rounds (from the out-degrees)
  float mean_min_w = 0.0f; // mean over the states of their cheapest finite arc weight (0: unknown)
};
// Region plan of the binned levels of the atomic sweeps (sssp_binned.h): source states in G contiguous ranges of `sg`
// states, destination states in `nbin` bins of 1 << logd; region (g -> b) holds one slot per arc from range g to bin b.
struct BinPlan {
  uint32_t nbin = 0, G = 0, sg = 0, logd = 13;
  uint64_t slots = 0;     // message slots in all (regions rounded up to whole 128-byte lines)
  DBuf<uint32_t> roff;    // [nbin*G + 1] destination-major
  DBuf<uint32_t> roff_t;  // [G*nbin]     source-major copy
};
}  // namespace wfst

namespace wfst {
// 4th word of a device state record (DeviceCsr::srec): what the compose filters' set_state needs to know
constexpr uint32_t SREC_NO_OEPS = 1u;   // no arc with olabel 0
constexpr uint32_t SREC_ALL_OEPS = 2u;  // every arc has olabel 0 (vacuously true without arcs)
constexpr uint32_t SREC_NO_IEPS = 4u;   // no arc with ilabel 0
constexpr uint32_t SREC_ALL_IEPS = 8u;  // every arc has ilabel 0
}  // namespace wfst

struct HostCsr {
  std::vector<uint32_t> offsets;
  std::vector<wfst_tr> arcs;
  std::vector<float> finals;
};

struct wfst_fst {
  // (first member = destroyed last: the caches below release their buffers into it)
  std::shared_ptr<wfst::DevicePool> owner_pool;
  int device = 0;
  wfst_ctx* ctx = nullptr;  // the creating context: only dereferenced inside API calls, which need it alive anyway
  uint32_t n_states = 0;
  uint64_t n_arcs = 0;
  int64_t start = -1;
  uint64_t props = 0;
  bool has_host = false, has_dev = false;
  // arc-weight statistics gathered at upload (steer the near-far schedule of the relaxation)
  float mean_weight = 0.0f;   // mean of the finite arc weights
  bool has_negative = false;  // some arc weight < 0
  HostCsr host;
  DeviceCsr dev;
  // A linear path whose host arrays have not been built (has_host and has_dev both false): the result of a fused batch.
  // Its n_arcs arcs sit at path_arcs inside path_block — the pinned block the kernel wrote the whole batch's results into,
  // shared by them — and path_final is the final weight of the path's end (state 0 of the path FST, shortest_path.rs:257-272).
  // ensure_host() builds the three arrays on first use and lets go of the block.
  std::shared_ptr<wfst::PinnedBlock> path_block;
  const wfst_tr* path_arcs = nullptr;
  float path_final = 0.0f;
  bool path_form = false;
  // reverse(fst) (reverse.rs:33-87) as host CSR: built on the GPU on first use by the n>1 shortest-path search
  mutable std::shared_ptr<wfst::RevFst> rev_host;
  // transpose (in-arcs as {source state, arc position}) for the shortest-path backtrace; built on the second
  // shortest_path query of a large FST (sssp.hip reverse_csr)
  mutable std::shared_ptr<wfst::RevCsr> rev_dev;
  // reverse(fst) as a device handle of its own (push.hip: reverse distances, co-reachability): built on first use, its
  // mailbox plan with it; independent of the start state (the reversed FST always starts at 0), so set_start keeps it
  mutable std::shared_ptr<wfst_fst> rev_fst;
  mutable std::mutex rev_mu;
  // region plan of the mailbox relaxation sweeps; depends on (source, target) pairs only, built on first use
  mutable std::shared_ptr<wfst::MboxPlan> mbox;
  mutable std::shared_ptr<wfst::MboxPlan> mbox13;  // the same with blocks of 8192 states (resident launches of 1M .. 2M-state FSTs)
  mutable std::shared_ptr<wfst::BinPlan> binplan;  // region plan of the binned levels (FSTs beyond the mailbox range)
  // a linear, epsilon-free, single-final acceptor ("string": utils::acceptor, labels_to_fst.rs:111-132), detected at
  // upload from the host arrays; such an fst1 takes the specialised string o T kernel of the fused batch
  bool is_string = false;
  // per-arc {arc begin, arc count} of the destination state (8 B per arc) and whether any arc has ilabel 0: derived
  // lazily when the FST first serves as fst2 of the string o T kernel (compose.hip), cached under cache_mu
  mutable std::shared_ptr<wfst::DBuf<uint2>> anext;
  mutable int ieps_state = 0;  // 0 unknown, 1 no input epsilons, 2 has input epsilons
  mutable std::atomic<uint32_t> sp_queries{0};
  mutable std::atomic<uint32_t> last_sweeps{0};  // sweeps the last relaxation of this FST needed (sizes the first batch of the next)
  // mailbox sweeps: bit k set = launch k of the last solve was NOT a busy wide sweep (idle, hand-over or narrow launch):
  // the next solve gates that launch's bulk loads behind its mode / sleep decision
  mutable std::atomic<uint64_t> last_hint_mask{~0ull};
  // consecutive single-path queries of this FST that the bounded head ended in launch 0 (sssp_mailbox.h): while it lasts the
  // next eligible query is queued as that launch (plus a spare one until three in a row).  last_sweeps keeps the count of the
  // last FULL solve, which is what a solve that cannot stop is sized from.
  mutable std::atomic<uint32_t> bounded_streak{0};
  mutable std::atomic<uint32_t> stable_sweeps{0};  // consecutive solves that needed exactly last_sweeps launches
  // single-path queries of the large-FST route begun on this FST, from any context (shortest_path_n1_begin): what a context's
  // parked scratch remembers of it tells whether anybody else has queried the handle since (RearmRecord::epoch)
  mutable std::atomic<uint64_t> sp_epoch{0};
  // the lazily built caches above may be requested from several contexts (threads) at once: built under this lock,
  // with buffers taken from the OWNER context's pool (this->ctx), which outlives the handle
  mutable std::mutex cache_mu;
};

// The table of paths of one call of paths.hip, in HBM: the paths of item i are rows item_off[i] .. item_off[i + 1], in the
// reference's order.  A table without paths holds no device array.
struct wfst_paths {
  // (first member = destroyed last: the buffers below go back to it)
  std::shared_ptr<wfst::DevicePool> pool;
  int device = 0;
  uint64_t n_paths = 0, n_il = 0, n_ol = 0;
  std::vector<uint64_t> item_off;      // [items + 1]
  wfst::DBuf<float> weights;           // [n_paths]
  wfst::DBuf<uint64_t> iloff, oloff;   // [n_paths + 1]
  wfst::DBuf<uint32_t> il, ol;         // [n_il], [n_ol]
};

namespace wfst {
// an intermediate FST handle of an operation: destroyed on every exit, with its device current
struct HandleDeleter {
  void operator()(wfst_fst* p) const {
    if (!p) return;
    (void)hipSetDevice(p->device);
    delete p;
  }
};
using Handle = std::unique_ptr<wfst_fst, HandleDeleter>;
// 64-bit finalizer (MurmurHash3 fmix64) of the device hash tables, and the odd word (2^64 / phi) that spreads a second key
// word before it
constexpr uint64_t GOLDEN64 = 0x9E3779B97F4A7C15ull;
__device__ inline uint64_t mix64(uint64_t x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}
// device_ops.hip: the host-side plumbing every operation repeats (all of it on ctx->stream)
// out[i] = in[0] + .. + in[i - 1] for i < count.  The scan runs asynchronously in the returned scratch: keep it alive until
// the caller's next synchronisation of the stream.
[[nodiscard]] DBuf<uint8_t> exclusive_scan_u32(wfst_ctx* ctx, const uint32_t* in, uint32_t* out, size_t count);
uint32_t read_u32(wfst_ctx* ctx, const uint32_t* d);  // one word back to the host; synchronises the stream
// indeg[arcs[i].nextstate] += 1 over the n_arcs arcs (indeg zeroed by the caller; nothing is launched without arcs)
void count_indegrees(wfst_ctx* ctx, const wfst_tr* arcs, uint64_t n_arcs, uint32_t* indeg);
// size of a hash table for v entries: the power of two >= max(v, 64); throws "<what>: ..." beyond 2^31
uint32_t pow2_at_least(uint64_t v, const char* what);
// fst_store.hip
void ensure_device(wfst_fst* f);             // upload host copy if needed (mutates cache only)
void ensure_host(const wfst_fst* f);         // download if needed
wfst_fst* make_host_fst(wfst_ctx* ctx, uint32_t n_states, int64_t start, uint64_t props, HostCsr&& csr);
wfst_fst* upload_from_host(wfst_ctx* ctx, uint32_t n_states, int64_t start, const uint32_t* offsets,
                           const wfst_tr* arcs, const float* finals, uint64_t props);
wfst_fst* upload_from_device(wfst_ctx* ctx, uint32_t n_states, int64_t start, const uint32_t* d_offsets,
                             const wfst_tr* d_arcs, const float* d_finals, uint64_t props);
void upload_many(wfst_ctx* ctx, size_t n, const uint32_t* n_states, const int64_t* starts, const uint32_t* offsets_cat,
                 const wfst_tr* arcs_cat, const float* finals_cat, const uint64_t* props, wfst_fst** outs);
// adopt freshly produced device arrays (compose output) as a new FST; arrays are copied into one arena
wfst_fst* adopt_device(wfst_ctx* ctx, uint32_t n_states, uint64_t n_arcs, int64_t start, uint64_t props,
                       const uint32_t* d_offsets, const wfst_tr* d_arcs, const float* d_finals);
// ... of the m results of one batch in one allocation and one synchronisation (fst_store.hip)
struct AdoptDesc {
  uint32_t n_states;
  uint64_t n_arcs;
  int64_t start;
  uint64_t props;
  const uint32_t* off;
  const wfst_tr* arcs;
  const float* fin;
};
void adopt_device_many(wfst_ctx* ctx, size_t m, const AdoptDesc* descs, wfst_fst** outs);
// openfst_io.cpp
wfst_fst* fst_from_openfst_bytes(wfst_ctx* ctx, const uint8_t* data, size_t len);
void fst_to_openfst_bytes(const wfst_fst* f, std::vector<uint8_t>& out);
void fst_to_openfst_const_bytes(const wfst_fst* f, std::vector<uint8_t>& out);
// api.cpp: gives the parked scratch of ctx back to the pool (nothing parked: nothing happens).  The re-arm launch may still be
// writing it, so the stream is waited for first — a rare path: a solve that matches the record adopts it instead.
void rearm_drop(wfst_ctx* ctx);
// sssp.hip
wfst_fst* shortest_path_n1(wfst_ctx* ctx, const wfst_fst* f);
wfst_sp_job* shortest_path_n1_begin(wfst_ctx* ctx, const wfst_fst* f);
wfst_fst* shortest_path_n1_end(wfst_sp_job* job);
void shortest_path_n1_abandon(wfst_sp_job* job);
void sp_host_timing_report(wfst_ctx* ctx);  // (prints under WFST_SP_HOST_TIMING; called when the context is destroyed)
wfst_ctx* sp_job_ctx(wfst_sp_job* job);
// the last solve that finished on `device` in this process ran WIDE levels in a resident launch (never solved: false)
bool resident_grid_at_work(int device);
void shortest_distance(wfst_ctx* ctx, const wfst_fst* f, float* distance, uint32_t* hops);
void shortest_distance_device(wfst_ctx* ctx, const wfst_fst* f, float* d_distance);
// nshortest.hip
wfst_fst* shortest_path_nbest(wfst_ctx* ctx, const wfst_fst* f, uint64_t nshortest, float delta, bool unique = false);
// nbest_batch.hip
void shortest_path_nbest_batch(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, uint64_t nshortest, float delta, wfst_fst** outs);
wfst_fst* reverse_fst(wfst_ctx* ctx, const wfst_fst* f);
// per-arc destination ranges / input-epsilon check of an FST used as fst2 of the string o T kernel (cached on the handle)
const uint2* ensure_anext(wfst_ctx* ctx, const wfst_fst* f);
bool has_input_epsilons(wfst_ctx* ctx, const wfst_fst* f);
bool detect_string(uint32_t n_states, int64_t start, const uint32_t* offsets, const wfst_tr* arcs, const float* finals);
// tr_sort.hip
void tr_sort_device(wfst_ctx* ctx, wfst_fst* f, bool ilabel_cmp);
// fst_store.hip
void project_device(wfst_ctx* ctx, wfst_fst* f, bool project_output);
void invert_device(wfst_ctx* ctx, wfst_fst* f);
// isomorphic.hip: isomorphic_with_config for two handles of ctx (both left as they are); throws the reference's error
bool isomorphic_fsts(wfst_ctx* ctx, const wfst_fst* f1, const wfst_fst* f2, float delta);
// paths.hip: paths_iter of one handle or a list of handles of ctx as a table (a NEW table; the operands are left as they are),
// and the number of paths alone (saturated at UINT64_MAX); an accessible cycle throws
uint64_t count_paths_fst(wfst_ctx* ctx, const wfst_fst* f);
wfst_paths* paths_fst(wfst_ctx* ctx, const wfst_fst* f, uint64_t max_paths);
wfst_paths* paths_batch(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, uint64_t max_paths, uint8_t* in_kernel);
void paths_download(wfst_ctx* ctx, const wfst_paths* t, uint64_t* item_off, float* weights, uint64_t* ilabel_off, uint32_t* ilabels,
                    uint64_t* olabel_off, uint32_t* olabels);
// compose.hip
wfst_fst* compose(wfst_ctx* ctx, const wfst_fst* f1, const wfst_fst* f2, bool connect, uint32_t filter = 0);
// ... the match mode its operands' property words leave (0 both, 1 input, 2 output), or the reference's error
uint32_t decide_match_mode(uint64_t p1, uint64_t p2);
// ... of n = max(n1, n2) pairs in one call (a list of one serves every item); on a throw every outs[i] is null
void compose_batch(wfst_ctx* ctx, const wfst_fst* const* f1s, size_t n1, const wfst_fst* const* f2s, size_t n2, bool connect,
                   uint32_t filter, wfst_fst** outs, uint8_t* in_kernel);
void compose_shortest_path_batch(wfst_ctx* ctx, const wfst_fst* const* accs, size_t n, const wfst_fst* t, bool connect,
                                 wfst_fst** outs, uint64_t* composed_arcs, uint32_t filter = 0);
wfst_batch_job* compose_shortest_path_batch_begin(wfst_ctx* ctx, const wfst_fst* const* accs, size_t n, const wfst_fst* t,
                                                  uint32_t filter = 0);
// `sink`: the results as fixed-size records (layout of wfst_fst_pack_paths) instead of handles (outs may then be null)
struct PackedSink {
  uint32_t max_arcs;
  uint32_t* out;
};
void compose_shortest_path_batch_end(wfst_batch_job* job, wfst_fst** outs, uint64_t* composed_arcs, const PackedSink* sink = nullptr);
// one record of wfst_fst_pack_paths: [n_arcs, final-weight bits, valid, 0] + max_arcs arcs, zero padded
void pack_path_record(uint32_t* rec, uint32_t max_arcs, bool valid, uint32_t n_arcs, float final_weight, const wfst_tr* arcs);
void pack_path_record(uint32_t* rec, uint32_t max_arcs, const wfst_fst* path);
wfst_fst* make_path_fst(wfst_ctx* ctx, bool has_path, uint32_t hops, float final_weight, const wfst_tr* path_arcs);  // fst_store.hip
// nbest_batch.hip: nshortest == 1 for many small FSTs in one launch (one wavefront each); the others one after the other
void shortest_path_n1_batch(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, wfst_fst** outs, bool lone = false);
bool shortest_path_n1_tiny(wfst_ctx* ctx, const wfst_fst* f, wfst_fst** out);  // a lone tiny FST: one wavefront (false: not applicable)
// nbest_batch.hip: distances + CSR of many small device FSTs in one launch (for host-side stages over a batch)
struct SmallFstExport {
  bool ok = false;
  std::vector<float> dist;
  HostCsr csr;
};
constexpr uint32_t SMALL_FST_MAX_STATES = 4096, SMALL_FST_MAX_ARCS = 16384;
void export_small_with_distances(wfst_ctx* ctx, const wfst_fst* const* fsts, const std::vector<size_t>& idx,
                                 std::vector<SmallFstExport>& out);
// nshortest.hip: nshortest > 1 with unique = true for a batch (small inputs: one launch + host threads)
void shortest_path_nbest_unique_batch(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, uint64_t nshortest, float delta, wfst_fst** outs);
void compose_shortest_path_batch_abandon(wfst_batch_job* job);
wfst_ctx* batch_job_ctx(const wfst_batch_job* job);
// compose_wide.hip
wfst_fst* connect_fst(wfst_ctx* ctx, const wfst_fst* f);
wfst_fst* connect_and_adopt(wfst_ctx* ctx, uint32_t n, int64_t start, const uint32_t* off, const wfst_tr* arcs, const float* fin,
                            bool all_accessible, uint64_t out_props);
// rm_epsilon.hip
wfst_fst* rm_epsilon_fst(wfst_ctx* ctx, const wfst_fst* f);
// ... its property word from the input's stored word and the facts of the added arcs (1 ilabel != olabel | 2 nextstate <=
// its state | 4 an arc was added), and its result when connect leaves nothing
uint64_t rm_epsilon_word(uint64_t in, uint32_t facts);
wfst_fst* rm_epsilon_empty(wfst_ctx* ctx, uint64_t word);
// rm_epsilon_batch.hip: n FSTs in one call, one workgroup each (new handles; on a throw every outs[i] is null)
void rm_epsilon_batch(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, wfst_fst** outs, uint8_t* in_kernel);
// push.hip: shortest_distance(fst, reverse) with the reference's Vec length, reweight, push_weights (new handles)
void shortest_distance_ex(wfst_ctx* ctx, const wfst_fst* f, bool reverse, float* distance, uint32_t* len);
wfst_fst* reweight_fst(wfst_ctx* ctx, const wfst_fst* f, const float* potentials, uint64_t n_potentials, uint32_t reweight_type);
wfst_fst* push_weights_fst(wfst_ctx* ctx, const wfst_fst* f, uint32_t reweight_type, bool remove_total_weight);
// push.hip: the four DFS pairs compute_and_update_properties(INITIAL_ACYCLIC) fills in (props::merge_dfs), searched on the device
uint64_t structural_bits(wfst_ctx* ctx, const wfst_fst* f);
// push.hip: WFST_PUSH_MAX_BLOCKS (tests), the cap on the grids of push.hip's three strided kernels: 0 when unset or empty,
// throws on anything but a positive integer.  Read per call; the three entry points call it before anything else runs.
uint32_t push_max_blocks_knob();
// determinize.hip: determinize_with_config of an acceptor (a NEW handle); det_type in the ffi numbering
wfst_fst* determinize_fst(wfst_ctx* ctx, const wfst_fst* f, float delta, uint32_t det_type);
// ... of a label-encoded machine (optimize.hip): no "the word must say ACCEPTOR" check, the gallic call's word
wfst_fst* determinize_encoded_fst(wfst_ctx* ctx, const wfst_fst* f, float delta, uint32_t det_type);
// determinize.hip: n acceptors in one call, one workgroup each (new handles; on a throw every outs[i] is null); with
// out_dist != null also determinize_with_distance's vector per item, concatenated, and its n + 1 offsets
void determinize_batch(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, float delta, uint32_t det_type, wfst_fst** outs,
                       uint8_t* in_kernel, const float* const* in_dist = nullptr, const uint64_t* n_in_dist = nullptr,
                       std::vector<float>* out_dist = nullptr, std::vector<uint64_t>* out_off = nullptr);
wfst_fst* determinize_with_distance_fst(wfst_ctx* ctx, const wfst_fst* f, const float* in_dist, uint64_t n_in_dist, float delta,
                                        std::vector<float>& out_dist);
// tr_sum.hip: tr_sum / tr_unique (a NEW handle)
wfst_fst* tr_sum_fst(wfst_ctx* ctx, const wfst_fst* f, bool unique);
// ... of n FSTs in one call, one workgroup each (new handles; on a throw every outs[i] is null)
void tr_sum_batch(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, bool unique, wfst_fst** outs, uint8_t* in_kernel);
// rational.hip: union / concat / closure and the list forms (NEW handles; the operands are left as they are)
wfst_fst* union_fst(wfst_ctx* ctx, const wfst_fst* a, const wfst_fst* b);
wfst_fst* concat_fst(wfst_ctx* ctx, const wfst_fst* a, const wfst_fst* b);
wfst_fst* closure_fst(wfst_ctx* ctx, const wfst_fst* f, bool star);
wfst_fst* union_list_fst(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n);
wfst_fst* concat_list_fst(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n);
// the size rule of the five calls above, which each of them calls first, on bare counts (op: 0 union, 1 concat, 2 closure
// star, 3 closure plus): throws "<op>: result too large: ..."
void rational_check_sizes(uint32_t op, const uint64_t* n_states, const uint64_t* n_arcs, size_t n);
// top_sort.hip: state_sort by an order given on the host and top_sort in the reference's DFS order (NEW handles)
wfst_fst* state_sort_fst(wfst_ctx* ctx, const wfst_fst* f, const uint32_t* order, size_t n_order);
wfst_fst* top_sort_fst(wfst_ctx* ctx, const wfst_fst* f);
// ... of n FSTs in one call, one workgroup each and one launch for all (new handles; on a throw every outs[i] is null)
void top_sort_batch(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, wfst_fst** outs, uint8_t* in_kernel);
// optimize.hip: optimize of an acyclic FST, acceptor or transducer (a NEW handle)
wfst_fst* optimize_fst(wfst_ctx* ctx, const wfst_fst* f);
// ... of n FSTs in one call over the four batch stages (new handles; on a throw every outs[i] is null)
void optimize_batch(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, wfst_fst** outs, uint8_t* in_kernel);
// minimize.hip: minimize_with_config of a deterministic acyclic acceptor (a NEW handle)
wfst_fst* minimize_fst(wfst_ctx* ctx, const wfst_fst* f, float delta, bool allow_nondet);
// ... of n acceptors in one call, one workgroup each and one launch for all (new handles; on a throw every outs[i] is null)
void minimize_batch(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, float delta, bool allow_nondet, wfst_fst** outs,
                    uint8_t* in_kernel);
// replace.hip: replace(fst_list, root, epsilon_on_replace) over (labels[i], fsts[i]) (a NEW handle; the items are left as they are)
wfst_fst* replace_fst(wfst_ctx* ctx, uint32_t root_label, const uint32_t* labels, const wfst_fst* const* fsts, size_t n,
                      bool epsilon_on_replace);
wfst_fst* compose_wide(wfst_ctx* ctx, const wfst_fst* f1, const wfst_fst* f2, uint32_t mode, uint32_t filter, bool connect,
                       uint64_t out_props, uint64_t est_s);
// compose_sigma.hip: compose_with_config with a SigmaMatcher on side 1 (m1), side 2 (m2) or both (a NEW handle); a null spec is
// the plain SortedMatcher.  rewrite_mode: 0 Auto, 1 Always, 2 Never; n_allowed == 0: no restriction
struct SigmaSpec {
  uint32_t sigma_label, rewrite_mode;
  const uint32_t* allowed;
  size_t n_allowed;
};
wfst_fst* compose_sigma(wfst_ctx* ctx, const wfst_fst* f1, const wfst_fst* f2, bool connect, uint32_t filter, const SigmaSpec* m1,
                        const SigmaSpec* m2);
// ... its set-up errors in the reference's order (nothing is launched), and the match mode (0 both, 1 input, 2 output)
uint32_t sigma_setup_mode(const wfst_fst* f1, const wfst_fst* f2, uint32_t filter, const SigmaSpec* m1, const SigmaSpec* m2);
// compose_sigma_batch.hip: outs[i] = shortest_path(compose_sigma(accs[i], t, ...)) for n acceptors (new handles; on a throw every
// outs[i] is null); strings against a sigma matcher on t run one wavefront each in one launch, the rest one by one
void compose_sigma_sp_batch(wfst_ctx* ctx, const wfst_fst* const* accs, size_t n, const wfst_fst* t, bool connect, uint32_t filter,
                            const SigmaSpec* m1, const SigmaSpec* m2, wfst_fst** outs, uint64_t* composed_arcs);
// compose.hip: the fused batch's path FST from a kernel's report (facts: the OR of props::path_arc_facts, or PATH_FACTS_NONE)
wfst_fst* batch_path_fst(wfst_ctx* ctx, bool has_path, uint32_t hops, float final_weight, uint32_t facts, const wfst_tr* path_arcs);
}  // namespace wfst
