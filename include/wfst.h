/*
 * wfst.h — C-ABI of the MI355X-native WFST compose + shortest-path engine (libwfst_amd.so).
 *
 * Drop-in boundary for rustfst's `algorithms::compose` and `algorithms::shortest_path` on
 * VectorFst<TropicalWeight>.  Conventions are the ones rustfst-ffi already uses, so a Rust shim
 *  can bind these with `extern "C"` exactly as it binds its own cdylib:
 *   - every call returns a status (0 = OK, 1 = KO)            rustfst-ffi/src/lib.rs:29-37
 *   - the error text is thread-local, fetched + freed by the caller
 *                                                               rustfst-ffi/src/lib.rs:39-85
 *   - objects are opaque heap handles written into an out-param and released by an explicit
 *     destroy; inputs are borrowed, outputs are owned by the caller
 *                                                               rustfst-ffi/src/algorithms/compose.rs:274-334
 *   - labels / state ids are `unsigned int`, an arc is CTr      rustfst-ffi/src/lib.rs:19-27, src/tr.rs:8-21
 * Plain pointers and sizes only; no torch / HIP types in any signature (a HIP stream crosses
 * as `void*`).
 *
 * Semantics are the reference's (file:line cited per entry point).  Two documented deviations,
 * both inside behaviour the reference itself leaves undefined or approximate:
 *   1. TropicalWeight `==` is exact here; the reference's is |a-b| <= 1/1024
 *      (rustfst/src/semirings/semiring.rs:159-168).  Identical results whenever weights lie on a
 *      grid coarser than 1/1024 (all fixtures / benchmarks); otherwise this engine returns the true
 *      (min,+) optimum.
 *   2. Among equal-weight shortest paths the winner is the canonical one (fewest arcs, then smallest
 *      (state,arc position) predecessor); the reference picks "first relaxer in queue order" and its
 *      own tests refuse to compare such outputs structurally
 *      (rustfst/src/tests_openfst/algorithms/shortest_path.rs:69-92).
 */
#ifndef WFST_AMD_H
#define WFST_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WFST_ABI_VERSION 7 /* 7: wfst_fst_set_start, then wfst_shortest_distance_with_config, wfst_push_weights, wfst_reweight, wfst_determinize, wfst_minimize, wfst_ctx_get_rm_epsilon_stats, wfst_ctx_get_rearm_stats, wfst_ctx_get_bounded_stats, wfst_ctx_trim_pool, wfst_ctx_get_small_path_stats, wfst_ctx_get_compose_path_stats, wfst_ctx_get_string_run_stats, wfst_ctx_get_string_pair_counts, wfst_ctx_get_string_placement, wfst_ctx_get_determinize_stats, wfst_ctx_get_minimize_stats, wfst_ctx_get_push_stats, wfst_tr_sum_batch, wfst_tr_unique_batch, wfst_ctx_get_tr_sum_batch_stats, wfst_optimize_batch, wfst_ctx_get_optimize_batch_stats, wfst_state_sort, wfst_top_sort, wfst_ctx_get_top_sort_stats, wfst_replace, wfst_ctx_get_replace_stats, wfst_compose_with_matchers, wfst_ctx_get_compose_sigma_counters, wfst_compose_shortest_path_batch_with_matchers, wfst_ctx_get_sigma_batch_counters, wfst_top_sort_batch, wfst_ctx_get_top_sort_batch_counters, wfst_ctx_get_lookahead_stats, wfst_compose_batch, wfst_ctx_get_compose_batch_counters, wfst_fst_invert, wfst_isomorphic, wfst_ctx_get_isomorphic_counters, wfst_fst_count_paths, wfst_fst_paths, wfst_fst_paths_batch, wfst_paths_info, wfst_paths_download, wfst_paths_destroy, wfst_ctx_get_paths_counters; 6: wfst_ctx_set_resident_share; 5: wfst_ctx_get_sweep_modes, relax_kernel may be 3, wfst_stats gained tied_choices;
                             * 2: wfst_stats gained relax_kernel; 3: wfst_comm_* / wfst_gather_paths_*, ..._batch_packed;
                             * 4: wfst_stats gained resident_aborts, relax_kernel may be 2; wfst_comm_create_host, wfst_gather_records_begin */

typedef enum { WFST_OK = 0, WFST_KO = 1 } wfst_status; /* RUSTFST_FFI_RESULT, rustfst-ffi/src/lib.rs:29-37 */

/* == rustfst-ffi CTr (src/tr.rs:8-21) == the 16-byte on-disk arc (parsers/bin_fst/utils_parsing.rs:28-44) */
typedef struct {
  uint32_t ilabel;
  uint32_t olabel;
  float weight; /* TropicalWeight: +inf = zero, 0.0 = one */
  uint32_t nextstate;
} wfst_tr;

#define WFST_EPS_LABEL 0u             /* rustfst/src/lib.rs:236 */
#define WFST_NO_LABEL 0xFFFFFFFFu     /* rustfst/src/lib.rs:292 */
#define WFST_NO_STATE_ID 0xFFFFFFFFu  /* rustfst/src/lib.rs:298 */

typedef struct wfst_ctx wfst_ctx; /* one per (host thread, GPU); owns a HIP stream + device pools */
typedef struct wfst_fst wfst_fst; /* an FST resident in HBM as CSR (and/or on the host for small results) */

/* ---- errors: rustfst_ffi_get_last_error / rustfst_destroy_string (rustfst-ffi/src/lib.rs:58-85) ---- */
wfst_status wfst_last_error(char** msg); /* takes the message (thread-local); caller frees */
wfst_status wfst_string_destroy(char* msg);
uint32_t wfst_abi_version(void);

/* ---- context ---- */
wfst_status wfst_ctx_create(int device, wfst_ctx** out);
/* use an existing HIP stream (e.g. torch.cuda.current_stream().cuda_stream); not owned */
wfst_status wfst_ctx_create_on_stream(int device, void* hip_stream, wfst_ctx** out);
/* context whose (own) stream may only use the compute units set in cu_mask (bit i of word i/32 = CU i;
 * hipExtStreamCreateWithCUMask).  For serving several request classes on one GPU: the fused batch is a handful of
 * long single-wave workgroups whose dependent loads slow down ~40 % when bandwidth-hungry kernels of another context
 * share their CUs; giving each context disjoint CUs removes that interference. */
wfst_status wfst_ctx_create_with_cu_mask(int device, const uint32_t* cu_mask, uint32_t mask_words, wfst_ctx** out);
wfst_status wfst_ctx_destroy(wfst_ctx* ctx);
wfst_status wfst_ctx_synchronize(wfst_ctx* ctx);
wfst_status wfst_ctx_stream(wfst_ctx* ctx, void** hip_stream);

/* ---- FST handles.  What the Rust shim produces by walking the trait surface
 * (start / num_states / get_trs / final_weight / properties: rustfst/src/fst_traits/fst.rs:18-226):
 *   offsets[n_states+1], arcs[offsets[n]] in per-state stored order, finals[n] with +inf = None
 *   (same sentinel as on disk, vector_fst/serializable_fst.rs:78-80), props = FstProperties bits
 *   (rustfst/src/fst_properties/properties.rs:22-103), start = -1 for None. ---- */
wfst_status wfst_fst_upload(wfst_ctx* ctx, uint32_t n_states, int64_t start, const uint32_t* offsets,
                            const wfst_tr* arcs, const float* finals, uint64_t props, wfst_fst** out);
/* same, but the three arrays already live in HBM on ctx's device (e.g. torch tensors); copied */
wfst_status wfst_fst_upload_device(wfst_ctx* ctx, uint32_t n_states, int64_t start, const uint32_t* d_offsets,
                                   const wfst_tr* d_arcs, const float* d_finals, uint64_t props, wfst_fst** out);
/* n FSTs in one shot (one device arena, one copy): arrays are concatenated; state_base[i] /
 * arc_base[i] give FST i's first state / arc; offsets are per-FST relative (each has n_i+1 entries,
 * concatenated: FST i's offsets start at state_base[i] + i). */
wfst_status wfst_fst_upload_many(wfst_ctx* ctx, size_t n, const uint32_t* n_states, const int64_t* starts,
                                 const uint32_t* offsets_cat, const wfst_tr* arcs_cat, const float* finals_cat,
                                 const uint64_t* props, wfst_fst** outs);
/* OpenFST binary, arc type "standard": vec_fst_from_bytes / vec_fst_to_bytes
 * (rustfst-ffi/src/fst/vector_fst.rs:319-354; format rustfst/src/parsers/bin_fst/fst_header.rs:71-112,
 * rustfst/src/fst_impls/vector_fst/serializable_fst.rs:45-168). Symbol tables are skipped.
 * The reader accepts fst_type "vector" (version >= 2) and "const" (version 1 = 16-byte aligned blocks, version 2;
 * rustfst/src/fst_impls/const_fst/serializable_fst.rs:176-237: const_fst_from_bytes, rustfst-ffi/src/fst/const_fst.rs).
 * _to_openfst_bytes writes "vector" v2, _to_openfst_const_bytes writes "const" v2 (ConstFst::store, :41-89). */
wfst_status wfst_fst_from_openfst_bytes(wfst_ctx* ctx, const uint8_t* data, size_t len, wfst_fst** out);
wfst_status wfst_fst_to_openfst_bytes(const wfst_fst* fst, uint8_t** data, size_t* len);
wfst_status wfst_fst_to_openfst_const_bytes(const wfst_fst* fst, uint8_t** data, size_t* len);
wfst_status wfst_bytes_destroy(uint8_t* data);

wfst_status wfst_fst_info(const wfst_fst* fst, uint32_t* n_states, uint64_t* n_arcs, int64_t* start,
                          uint64_t* props);
/* copy out: offsets[n_states+1], arcs[n_arcs], finals[n_states] (any pointer may be NULL) */
wfst_status wfst_fst_download(const wfst_fst* fst, uint32_t* offsets, wfst_tr* arcs, float* finals);
wfst_status wfst_fst_destroy(wfst_fst* fst);
/* destroys fsts[0..n) (NULL entries are skipped): the outs[] of a fused batch in one call */
wfst_status wfst_fst_destroy_many(wfst_fst* const* fsts, size_t n);

/* ---- compose: fst_compose / fst_compose_with_config (rustfst-ffi/src/algorithms/compose.rs:308-372)
 *      = rustfst::algorithms::compose::{compose, compose_with_config}
 *        (rustfst/src/algorithms/compose/compose_static.rs:166-306).
 * compose_filter uses the ffi numbering (compose.rs:20-33): 0 Auto (= Sequence, compose_fst.rs:58-92), 1 Null,
 * 2 Trivial, 3 Sequence, 4 AltSequence, 5 Match, 6 NoMatch — all with the default SortedMatcher pair
 * (rustfst/src/algorithms/compose/compose_filters/{null,trivial,sequence,alt_sequence,match,no_match}_compose_filter.rs);
 * matcher configs (the sigma matcher) go through wfst_compose_with_matchers below, wfst_compose_config keeps its layout.
 * cfg == NULL means ComposeConfig::default() = {Auto, connect = true} (compose_static.rs:56-65).
 * KO with the reference's message when neither side is known label-sorted
 * (compose/compose_fst_op.rs:169-197).  Output state ids / arc order are the reference's
 * (FIFO BFS discovery order, then stable trim: lazy/lazy_fst.rs:226-269, connect.rs:51-66). ---- */
typedef struct {
  uint32_t compose_filter;
  uint32_t connect; /* bool */
} wfst_compose_config;
wfst_status wfst_compose(wfst_ctx* ctx, const wfst_fst* fst1, const wfst_fst* fst2,
                         const wfst_compose_config* cfg, wfst_fst** out);

/* ---- compose of a list: n = max(n1, n2) compositions in one call; each of n1, n2 is n or 1, and a list of one serves every
 *      item (one grammar against n lattices, one lattice against n grammars).  outs[i] (new handles, each owning its memory)
 *      is bit for bit what wfst_compose(ctx, fst1s[i or 0], fst2s[i or 0], cfg) returns — state numbering, arc order, finals,
 *      start and property word — for every compose_filter 0..6, connect on and off, and cfg == NULL.  The inputs are left as
 *      they are; a handle may appear more than once.  n == 0: OK, nothing is touched.
 *      Routing, decided from sizes alone (in_kernel: uint8_t[n], may be NULL):
 *      - an item with no start state on either side is the empty FST with the single call's word: it occupies no workgroup,
 *        in_kernel[i] == 1, counted in items_no_start and in items_in_kernel;
 *      - with exactly ONE item that has both start states, that item IS the single call, limits and all: in_kernel[i] == 0,
 *        items_single;
 *      - otherwise every such item takes one wavefront of compose_batch_kernel, <<<open items, 64>>>, with its OWN second
 *        operand, capacities and arena, carved from the launch's slab (a 20-state item beside a 4 000-state item pays for 20
 *        states).  Attempt k of an item has the single call's capacities: S_k = (4 * max(min(n_states1, n_states2), 64)
 *        + 1024) * 4^k composed states, A_k = 4 * S_k arcs, H_k = the power of two at or above 2 * S_k + 128 hash slots.  An
 *        overflow of states, arcs or hash reopens the item with k + 1 in the next launch and counts once, per item and
 *        attempt, in regrown_states, regrown_arcs or regrown_hash; `launches` therefore follows the deepest regrowth among
 *        the items, not n.  An item whose next S_k exceeds 16384 leaves the kernel — at k = 0 when min(n_states1, n_states2)
 *        > 3840 — for the wide driver with that estimate: in_kernel[i] == 0, items_single;
 *      - the width hand-over of the single call is OFF in a list: while other waves are busy, a BFS level of more than 64 new
 *        states stays with its wave on the arena route (the single call would redo such a pair on the wide driver, and a list
 *        of lattices would then run one by one).  The result is the same FST.
 *      The slices of one launch may take 8 GiB together: beyond that the call is KO before that launch ("split the list").
 *      WFST_COMPOSE_BATCH_ARENA=min (tests) starts every item at the kernel's minimum, S = 64 and A = 128, so that every item
 *      grows.
 *      KO, decided before any GPU work and in this order: a NULL pointer "null pointer"; "compose_batch: the lists hold {n1}
 *      and {n2} FSTs (equal lengths, or one of them 1)"; "unknown compose_filter"; a NULL entry ("item <i>: null FST in
 *      batch"); an entry of another device or context ("item <i>: compose_batch: the FST lives on another device" / "...
 *      belongs to another context").  Then, per item in index order and before anything is launched, the single call's own
 *      errors behind "item <i>: " (the "(sort?)" messages, "compose: the 1st FST has more than 2^30 states"): the lowest
 *      failing index wins.  After a KO every outs[i] is NULL, no handle leaks and the context works on. ---- */
wfst_status wfst_compose_batch(wfst_ctx* ctx, const wfst_fst* const* fst1s, size_t n1, const wfst_fst* const* fst2s, size_t n2,
                               const wfst_compose_config* cfg, wfst_fst** outs, uint8_t* in_kernel);
/* the last wfst_compose_batch call of ctx that passed the checks above (reset when such a call begins; a call that is KO
 *      before anything is launched, and one with n == 0, leaves them alone): launches of compose_batch_kernel, items with in_kernel
 *      == 1, items that went through the single call or the wide driver, items without a start state, and the regrowths by
 *      cause.  Any pointer after ctx may be NULL. */
wfst_status wfst_ctx_get_compose_batch_counters(wfst_ctx* ctx, uint64_t* launches, uint64_t* items_in_kernel,
                                                uint64_t* items_single, uint64_t* items_no_start, uint64_t* regrown_states,
                                                uint64_t* regrown_arcs, uint64_t* regrown_hash);

/* ---- compose with matcher configs: fst_compose_with_config with a non-empty matcher1_config / matcher2_config
 *      (rustfst-ffi/src/algorithms/compose.rs:183-250) = compose_with_config with SigmaMatcher<SortedMatcher> on side 1 (m1),
 *      side 2 (m2) or both (compose_static.rs:78-109, 166-266; compose/matchers/sigma_matcher.rs): an arc labelled
 *      sigma_label on the matched tape (olabel of fst1, ilabel of fst2) stands for "any other label".  m1 == m2 == NULL is
 *      wfst_compose, call for call.  Otherwise the call runs on the wide driver whatever its size, and returns bit for bit
 *      what the reference returns, the property word (that of the plain call) included.
 *      iter(state, label) of a sigma side (sigma_matcher.rs:190-239): whatever the sorted matcher yields for `label`, if it
 *      yields anything (for label 0 the epsilon loop, so always), unrewritten; otherwise the state's sigma arcs, in order and
 *      rewritten, iff `label` is neither 0 nor NO_LABEL and sigma_allowed_matches is unrestricted or holds it.  Exhausted exact
 *      matches do NOT fall through to the sigma arcs (the branch of :270-284 is dead; OpenFst's matcher differs).
 *      Rewriting (:246-266): rewrite_mode 0 Auto = 1 iff the sigma operand's word says ACCEPTOR, else 2; 1 Always: each of
 *      ilabel / olabel that equals sigma becomes the matched label; 2 Never: only the matched tape's label is set.
 *      n_allowed == 0 means no restriction (rustfst-ffi compose.rs:199-211); order and duplicates do not matter.
 *      sigma_label == WFST_NO_LABEL: no state has a sigma arc, the result is wfst_compose's (on the wide driver).
 *      KO, in this order: rewrite_mode > 2 "unknown rewrite_mode"; sigma_label 0 "SigmaMatcher: 0 cannot be used as
 *      sigma_label" (sigma_matcher.rs:64-66); compose_filter 0 "Custom MatcherConfig not supported with AutoFilter"
 *      (compose_static.rs:186-191); a side with a real sigma that is not known sorted on its matched tape "ComposeFst: 1st
 *      [2nd] argument cannot perform required matching (sort?)" (compose_fst_op.rs:169-180; an unknown bit pair: "...
 *      label-sortedness properties are not known (sort?)"); then the mode errors of wfst_compose.  While composing: the first
 *      offending composed state in id order, and within it first "Both sides can't require match" (both states carry a sigma
 *      arc and both sides are sorted, compose_fst_op.rs:207-209), then per item of the iterated side "SigmaMatcher::Find: bad
 *      label (sigma)" (its label IS the searched side's sigma, sigma_matcher.rs:199-201).  The context works on after a KO.
 *      wfst_stats.compose_states / compose_arcs are set; arena growths go to compose_retries and to arena_grows below. ---- */
typedef struct {
  uint32_t sigma_label;
  uint32_t rewrite_mode; /* 0 Auto, 1 Always, 2 Never (MatcherRewriteMode) */
  const uint32_t* sigma_allowed_matches;
  size_t n_allowed; /* 0 = unrestricted */
} wfst_matcher_config;
wfst_status wfst_compose_with_matchers(wfst_ctx* ctx, const wfst_fst* fst1, const wfst_fst* fst2, const wfst_compose_config* cfg,
                                       const wfst_matcher_config* m1, const wfst_matcher_config* m2, wfst_fst** out);
/* the last wfst_compose_with_matchers call of ctx that had a config (reset when it begins; all 0 after a KO or an empty
 * result, except arena_grows): levels of the search, states and arcs before connect, composed states whose fst1 / fst2 state
 * carries a sigma arc, items (loop item included) of a sigma side that its sorted matcher answered, that its sigma arcs
 * answered, the arcs those emitted, items the allowed set refused, growths of the arena, level launches queued.  A level
 * that is emitted again after an overflow counts its items again.  Any out-pointer may be NULL.  (Not one of the
 * wfst_ctx_get_*_stats route-counter families: it is read through the same helper, outside their table.) */
wfst_status wfst_ctx_get_compose_sigma_counters(wfst_ctx* ctx, uint64_t* levels, uint64_t* states, uint64_t* arcs,
                                             uint64_t* require1_states, uint64_t* require2_states, uint64_t* exact_items,
                                             uint64_t* sigma_items, uint64_t* sigma_arcs, uint64_t* refused_items,
                                             uint64_t* arena_grows, uint64_t* level_launches);

/* ---- shortest path: fst_shortest_path / fst_shortest_path_with_config
 *      (rustfst-ffi/src/algorithms/shortest_path.rs:44-83) = rustfst::algorithms::shortest_path
 *      (rustfst/src/algorithms/shortest_path.rs:76-133).  cfg == NULL means
 *      ShortestPathConfig::default() = {delta 1e-6, nshortest 1, unique false} (:31-39).
 *      nshortest == 0 -> empty FST (:118-120).  nshortest == 1 (unique ignored, as in the reference):
 *      relaxation + backtrace on the GPU; output = linear FST numbered backwards, state 0 final (:241-282).
 *      nshortest > 1, unique = false (:135-170): shortest_distance and reverse() on the GPU, the sequential
 *      n_shortest_path heap search (:409-518) + connect on the host; output = the reference's path tree.
 *      nshortest > 1 with unique = true (:157-165): the reversed FST is determinized first (determinize_with_distance,
 *      determinize/determinize_static.rs:24-39; host code, input must be an ACCEPTOR by its property word or the call is
 *      KO "DeterminizeFsaImpl : expected acceptor as argument", as in the reference), then the same search: the n best
 *      DISTINCT strings.  Where the reference keeps a weighted subset in HashMap order (unspecified, and part of a
 *      state's identity there) this library keeps it in ascending state order. ---- */
typedef struct {
  float delta;
  uint64_t nshortest;
  uint32_t unique; /* bool */
} wfst_shortest_path_config;
wfst_status wfst_shortest_path(wfst_ctx* ctx, const wfst_fst* fst, const wfst_shortest_path_config* cfg,
                               wfst_fst** out);
/* single-source (min,+) distances from the start state (what single_shortest_path computes into
 * `distance`, shortest_path.rs:173-239) copied to host arrays of n_states entries; hops may be NULL. */
wfst_status wfst_shortest_distance(wfst_ctx* ctx, const wfst_fst* fst, float* distance, uint32_t* hops);

/* ---- shortest_distance(fst, reverse) / shortest_distance_with_config (rustfst/src/algorithms/shortest_distance.rs:307-336).
 *      cfg == NULL: {reverse 0, delta KSHORTESTDELTA = 1e-6} (ShortestDistanceConfig::default, :260-266).
 *      reverse == 0: exactly wfst_shortest_distance.  reverse != 0: reverse(fst), distances from its super-initial state,
 *      entry 0 dropped (:322-334); defined without a start state too (the reversed FST always starts at 0).  The reversed
 *      FST is built on the GPU once and cached on the handle (set_start keeps it).
 *      distance[n_states]; entries past the reference's Vec length are +inf; *len (may be NULL) = that Vec length: one plus
 *      the largest state id the reference's search touches (every state reachable from its source).
 *      delta must be finite and >= 0; like wfst_shortest_distance the device returns the exact fixed point, the reference
 *      ignores improvements of at most delta (identical on weights of a grid coarser than delta). ---- */
typedef struct {
  uint32_t reverse; /* bool */
  float delta;
} wfst_shortest_distance_config;
wfst_status wfst_shortest_distance_with_config(wfst_ctx* ctx, const wfst_fst* fst, const wfst_shortest_distance_config* cfg,
                                               float* distance, uint32_t* len);

/* ---- push_weights / push_weights_with_config (rustfst/src/algorithms/push.rs:76-170): distances (reverse ones for
 *      ReweightToInitial), reweight, then with remove_total_weight remove_weight of the total (push.rs:120-170).
 *      reweight_type: 0 = ReweightToInitial, 1 = ReweightToFinal (reweight.rs enum order); anything else is KO.
 *      cfg == NULL: PushWeightsConfig::default() = {KDELTA, false} (push.rs:41-48); delta as in
 *      wfst_shortest_distance_with_config.  The reference works in place; here a NEW handle is returned (it may have one
 *      state more than fst: reweight.rs:129-138).  Weights and property word follow the reference bit for bit. ---- */
typedef struct {
  float delta;
  uint32_t remove_total_weight; /* bool */
} wfst_push_weights_config;
wfst_status wfst_push_weights(wfst_ctx* ctx, const wfst_fst* fst, uint32_t reweight_type, const wfst_push_weights_config* cfg,
                              wfst_fst** out);

/* ---- reweight (rustfst/src/algorithms/reweight.rs:29-154): reweight(fst, potentials[0..n_potentials), reweight_type);
 *      potentials on the host, +inf = zero, a state >= n_potentials has potential zero.  NULL potentials with
 *      n_potentials > 0 is KO; reweight_type as in wfst_push_weights.  A NEW handle. ---- */
wfst_status wfst_reweight(wfst_ctx* ctx, const wfst_fst* fst, const float* potentials, uint64_t n_potentials,
                          uint32_t reweight_type, wfst_fst** out);

/* ---- connect: fst_connect (rustfst-ffi/src/algorithms/connect.rs:14-23) = rustfst::algorithms::connect
 *      (rustfst/src/algorithms/connect.rs:51-66): the states that are accessible from the start state and can reach a
 *      final state, renumbered stably (del_states, vector_fst/mutable_fst.rs:132-189), arcs into deleted states dropped.
 *      The reference trims in place; here a NEW handle is returned (the caller destroys the old one). ---- */
wfst_status wfst_connect(wfst_ctx* ctx, const wfst_fst* fst, wfst_fst** out);

/* ---- determinize / determinize_with_config (rustfst/src/algorithms/determinize/determinize_static.rs:149-190) of an
 *      ACCEPTOR: DeterminizeFsa with DefaultCommonDivisor (determinize_fsa_op.rs:43-196) in LazyFst::compute's FIFO
 *      first-touch order (lazy/lazy_fst.rs:226-269).  The reference branches on the stored property word: without
 *      ACCEPTOR in it (a transducer, or an acceptor whose word does not say so) it takes the gallic transducer path,
 *      which is not supported here: KO "transducers are not supported" (callers keep rustfst's own call).
 *      det_type: 0 Functional, 1 NonFunctional, 2 Disambiguate (rustfst-ffi/src/algorithms/determinize.rs:17-25),
 *      anything else is KO; for an acceptor it changes only the property word (determinize_properties,
 *      mutate_properties.rs:247-279, through NO_EPSILONS).  cfg == NULL: DeterminizeConfig::default() = {KDELTA,
 *      Functional}.  delta must be finite and > 0 (the reference quantizes to NaN with 0).
 *      Subset order: after merging duplicate destinations the reference collects a subset from a HashMap, an
 *      unspecified order that takes part in its identity; here elements stay in ascending state order (as in the
 *      `unique` n-best branch), so every weighted subset is one state.  A subset joins the LOWEST-id state with the same
 *      states and pairwise approx_eq weights (|a - b| <= KDELTA, whatever delta is).  No start state: the empty FST.
 *      A cyclic weighted acceptor without the twins property does not determinize: KO beyond 16 M states / 256 M
 *      subset elements.  A NEW handle; fst is left as it is. ---- */
typedef struct {
  float delta;
  uint32_t det_type;
} wfst_determinize_config;
wfst_status wfst_determinize(wfst_ctx* ctx, const wfst_fst* fst, const wfst_determinize_config* cfg, wfst_fst** out);

/* ---- determinize_with_config (determinize_static.rs:176-190) of n ACCEPTORS in one call: outs[i] is a NEW handle,
 *      bit-identical (arrays, start state, property word) to what wfst_determinize(ctx, fsts[i], cfg, ..) returns.  cfg is
 *      shared by all items, NULL = the default as above.  The same handle may appear more than once in fsts.  n == 0: OK.
 *      One workgroup per item, one launch for every item that is still open: an item whose arena slice (sized on the host
 *      from its n_states and n_arcs) proves too small is run again in the next launch of the same call with a larger one.
 *      in_kernel (uint8_t[n], may be NULL): in_kernel[i] == 1 exactly when NO breadth-first level of item i has more than
 *      256 states or more than 8192 raw candidates (the sum of the out-degrees of the level's subset elements): the batch
 *      kernel constructed it (an item without start state or states counts as such: the empty FST).  in_kernel[i] == 0:
 *      the item went through the single-FST path of wfst_determinize.
 *      KO — every argument and every item's stored word is checked before anything is launched — when an item's word lacks
 *      ACCEPTOR or an item exceeds the state / element limit: the single call's message prefixed by "item <i>: ".  On
 *      any KO every outs[i] is NULL, nothing is leaked and the context works afterwards.
 *      WFST_DETERMINIZE_BATCH_SCRATCH=lds|global (environment) places the scratch of levels of at most 496 candidates in
 *      LDS or in the item's slice. ---- */
wfst_status wfst_determinize_batch(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, const wfst_determinize_config* cfg,
                                   wfst_fst** outs, uint8_t* in_kernel);

/* ---- determinize_with_distance (determinize/determinize_static.rs:24-39): the construction above with det_type
 *      Functional, and out_dist[s] = plus over the elements (q, w) of subset s, in stored (ascending state) order, of
 *      w (x) in_dist[q]; a state q >= n_in_dist counts as +inf (state_table.rs:25-39,79-96).  *out_dist is allocated by the
 *      library (release it with wfst_bytes_destroy), *n_out_dist is the result's state count.  in_dist == NULL with
 *      n_in_dist > 0 is KO; delta as above. ---- */
wfst_status wfst_determinize_with_distance(wfst_ctx* ctx, const wfst_fst* fst, const float* in_dist, uint64_t n_in_dist,
                                           float delta, wfst_fst** out, float** out_dist, uint64_t* n_out_dist);
/* ... of n acceptors in one call (as wfst_determinize_batch): in_dists[i] / n_in_dists[i] per item; *out_dist is ONE
 *      buffer (wfst_bytes_destroy) holding the items' vectors one after the other, item i at
 *      [out_offsets[i], out_offsets[i + 1]); out_offsets is the caller's uint64_t[n + 1]. */
wfst_status wfst_determinize_with_distance_batch(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n,
                                                 const float* const* in_dists, const uint64_t* n_in_dists, float delta,
                                                 wfst_fst** outs, float** out_dist, uint64_t* out_offsets, uint8_t* in_kernel);
/* the last wfst_determinize_batch / wfst_determinize_with_distance_batch call of ctx: launches of the batch kernel, items it
 *      constructed (in_kernel == 1), items that went through the single-FST path.  All 0 after a KO before any launch. */
wfst_status wfst_ctx_get_determinize_batch_stats(wfst_ctx* ctx, uint64_t* launches, uint64_t* items_in_kernel,
                                                 uint64_t* items_single);

/* ---- minimize / minimize_with_config (rustfst/src/algorithms/minimize.rs:77-176) of an input-deterministic ACYCLIC
 *      ACCEPTOR: the AcyclicMinimizer branch (:181-211, 306-387), whose result is a pure function of the input.
 *      ACCEPTOR, I_DETERMINISTIC and WEIGHTED / UNWEIGHTED come from the stored property word where it knows them and from
 *      the content otherwise (compute_and_update_properties, :101-106; "unweighted" = every weight within KDELTA of one
 *      or zero).  Weighted: push_weights(ToInitial), QuantizeMapper(delta), encode(weights and labels), acceptor_minimize,
 *      decode: the result carries the pushed AND quantized weights and its arcs come in the first-occurrence order of
 *      their (label, weight) tuples over the untrimmed input, not in label order.  Unweighted: acceptor_minimize on the
 *      original labels (arcs in label order).  Of every class of equivalent states one member survives: at each height
 *      (longest path to a state without arcs) the class holding the height's highest state id keeps its highest id,
 *      every other class its lowest; survivors keep their relative order.
 *      Tuple identity: the reference's encode table hashes the weight's bits but compares with KDELTA, so two tuples with
 *      equal labels and weights within 1/1024 merge there only when they meet in one probe group of a randomly seeded
 *      table.  Here identity is EXACT: equal labels and equal quantized value (-0.0 == +0.0).
 *      KO (callers keep rustfst's own call): a non-deterministic input, "Refusing to minimize a non-deterministic FST with
 *      allow_nondet = false", or with allow_nondet != 0 "non-deterministic inputs are not supported"; "transducers are
 *      not supported" (the gallic path); "cyclic inputs are not supported" (Hopcroft with a LIFO queue: the survivors
 *      depend on the order of its splits) — for a cycle anywhere, also one that connect would remove; an unweighted input
 *      whose merged states carry arc weights more than KDELTA apart (the reference keeps both arcs).
 *      No start state, or nothing left after connect: the empty FST.  A WEIGHTED input without a start state is pushed
 *      all the same (reweight.rs skips only the start-state step) while every tr_map returns at once, so the reference's
 *      acceptor_minimize sees the pushed weights: the empty FST when none of them is left, else the reference's own error
 *      "FST is not an unweighted acceptor" (rustfst fails on that input as well).  cfg == NULL: MinimizeConfig::default() = {KSHORTESTDELTA = 1e-6,
 *      false}.  delta must be finite and > 0.  A NEW handle; fst is left as it is (the reference works in place). ---- */
typedef struct {
  float delta;
  uint32_t allow_nondet;
} wfst_minimize_config;
wfst_status wfst_minimize(wfst_ctx* ctx, const wfst_fst* fst, const wfst_minimize_config* cfg, wfst_fst** out);

/* ---- minimize_with_config of n acceptors in one call: outs[i] is a NEW handle, bit-identical (offsets, arcs with their
 *      weights' bit patterns, finals, start state, property word) to what wfst_minimize(ctx, fsts[i], cfg, ..) returns.
 *      cfg is shared by all items, NULL = the default as above.  The same handle may appear more than once in fsts.
 *      n == 0: OK.  The inputs are left exactly as they are, their cached derived data and property words included.
 *      One workgroup per item and ONE launch for the whole list: the workgroup runs every stage of the single call (facts
 *      of the content, acyclicity and reverse distances by peeling sinks, push_weights(ToInitial), quantize + encode,
 *      connect, the per-state sort, heights fused with the refinement, survivors, emit) on its item inside the item's
 *      slice of one slab.  The slices are sized on the host from n_states and n_arcs alone (minimization never grows its
 *      input: the encoded machine has at most n_states + 1 states and n_arcs + n_states arcs), so nothing is run twice.
 *      Launches and host synchronisations of a call depend neither on n nor on any item's depth: one launch of the batch
 *      kernel, one read-back of the items' control blocks, and one adoption of all results out of the slab (one
 *      allocation, a gather and a derive launch with a block per result, one synchronisation).
 *      A slice takes about 230 KB for an item of 500 states and 1500 arcs and 2.5 MB at the rule's limit below; the slices
 *      of one call may take 8 GiB together (some 35 000 lattices of that size, 3 000 items at the limit): a list that
 *      needs more is KO before anything is launched ("split the list").
 *      in_kernel (uint8_t[n], may be NULL): in_kernel[i] == 1 exactly when item i has at most 4096 states and at most
 *      16384 arcs: the batch kernel minimized it (an item without states never occupies a workgroup and counts as such;
 *      so does an item without a start state that meets the rule).  in_kernel[i] == 0: the item went through
 *      wfst_minimize unchanged.
 *      One exception to the rule: an item whose stored word says INITIAL_CYCLIC is handed to wfst_minimize as well and
 *      has in_kernel[i] == 0 whatever its size.  Such an input is cyclic, which is KO, or its word contradicts ACYCLIC,
 *      and then reweight's start-state step adds a state, which a slice has no room for.
 *      KO — every argument is checked before anything is launched: NULL pointers, NULL list entries ("item <i>: null FST
 *      in batch"), a handle of another device or context, delta not finite or <= 0 — and whenever wfst_minimize would be
 *      KO for an item, whether the stored word says so or the kernel finds it: the message is the single call's for the
 *      LOWEST failing index, prefixed by "item <i>: "; within an item the checks come in the single call's order.  On
 *      any KO every outs[i] is NULL, nothing is leaked and the context works afterwards. ---- */
wfst_status wfst_minimize_batch(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, const wfst_minimize_config* cfg,
                                wfst_fst** outs, uint8_t* in_kernel);
/* the last wfst_minimize_batch call of ctx: launches of the batch kernel (0 or 1), items it minimized (in_kernel == 1), items
 *      that went through the single-FST path.  All 0 after a KO before any launch. */
wfst_status wfst_ctx_get_minimize_batch_stats(wfst_ctx* ctx, uint64_t* launches, uint64_t* items_in_kernel,
                                              uint64_t* items_single);

/* ---- tr_sum (rustfst/src/algorithms/tr_sum.rs:7-22, sum_trs_unchecked: fst_impls/vector_fst/mutable_fst.rs:380-405) and
 *      tr_unique (tr_unique.rs:8-51, unique_trs_unchecked: mutable_fst.rs:358-377).  Per state a STABLE sort by tr_compare:
 *      (ilabel, olabel, nextstate), unsigned, the weight not in the key.  tr_sum: of a run of equal keys the first arc
 *      survives, its weight folded with plus_assign over the run in sorted order (`if rhs < self`: a tie keeps the earlier
 *      arc's bits, -0.0 / +0.0 included, and NaN never replaces).  tr_unique: Vec::dedup on Tr's ==, i.e. an arc goes when
 *      its key equals that of the last KEPT arc and the two weights are within KDELTA (TropicalWeight's PartialEq,
 *      semiring.rs:161-168): weights 0, 0.0009, 0.0018 under one key keep the first and the third.
 *      Property word: props & arcsort_properties & delete_arcs_properties, for tr_sum also & weight_invariant_properties;
 *      | null_properties when the FST has no states.  No KO of their own beyond NULL pointers.
 *      The reference works in place; here a NEW handle is returned and fst is left as it is. ---- */
wfst_status wfst_tr_sum(wfst_ctx* ctx, const wfst_fst* fst, wfst_fst** out);
wfst_status wfst_tr_unique(wfst_ctx* ctx, const wfst_fst* fst, wfst_fst** out);

/* ---- tr_sum / tr_unique of n FSTs in one call: outs[i] is a NEW handle, bit-identical (offsets, arcs with their weights'
 *      bit patterns, finals, start state, property word) to what wfst_tr_sum / wfst_tr_unique(ctx, fsts[i], ..) returns.
 *      The same handle may appear more than once in fsts.  n == 0: OK.  The inputs are left exactly as they are, their
 *      cached derived data and property words included.
 *      One workgroup per item and ONE launch for the whole list: the workgroup runs the passes of the single call (the
 *      rank sort with 16 lanes per state, keep flags and survivors per state, a workgroup scan of the counts, the write
 *      pass with the serial fold of tr_sum / the KDELTA chain of tr_unique) on its item inside the item's slice of one
 *      slab.  The slices are sized on the host from n_states and n_arcs alone (the result never has more arcs than the
 *      input), so nothing is run twice.  Launches and host synchronisations of a call do not depend on n: one launch of
 *      the batch kernel, one read-back of the items' control blocks, and one adoption of all results out of the slab.
 *      A slice takes 33 bytes per arc and 8 per state (about 50 KB for an item of 500 states and 1500 arcs, 560 KB at the
 *      rule's limit below); the slices of one call may take 8 GiB together: a list that needs more is KO before anything
 *      is launched ("split the list").
 *      in_kernel (uint8_t[n], may be NULL): in_kernel[i] == 1 exactly when item i has at most 4096 states, at most
 *      16384 arcs and no state with more than 256 arcs (the limit of the rank sort; the kernel finds such a state itself
 *      and leaves the item).  An item without states and an item with at most one arc never occupy a workgroup, are
 *      produced as the single call produces them and count as in_kernel[i] == 1.  in_kernel[i] == 0: the item went
 *      through wfst_tr_sum / wfst_tr_unique unchanged.
 *      KO — every argument is checked before anything is launched: NULL pointers, NULL list entries ("item <i>: null FST
 *      in batch"), a handle of another device or context.  On any KO every outs[i] is NULL, nothing is leaked and the
 *      context works afterwards. ---- */
wfst_status wfst_tr_sum_batch(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, wfst_fst** outs, uint8_t* in_kernel);
wfst_status wfst_tr_unique_batch(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, wfst_fst** outs, uint8_t* in_kernel);
/* the last wfst_tr_sum_batch / wfst_tr_unique_batch call of ctx: launches of the batch kernel (0 or 1), items with
 *      in_kernel == 1, items that went through the single-FST path.  All 0 after a KO before any launch. */
wfst_status wfst_ctx_get_tr_sum_batch_stats(wfst_ctx* ctx, uint64_t* launches, uint64_t* items_in_kernel, uint64_t* items_single);

/* ---- optimize: fst_optimize (rustfst-ffi) = rustfst::algorithms::optimize (rustfst/src/algorithms/optimize.rs:11-128) for
 *      the tropical semiring (IDEMPOTENT), one call over device-resident stages.  Every branch is taken on the STORED
 *      property word:
 *        1. ACCEPTOR in the word: acceptor path, else transducer path
 *        2. rm_epsilon unless the word holds NO_EPSILONS (wfst_rm_epsilon)
 *        3. tr_sum (wfst_tr_sum); its mask leaves neither UNWEIGHTED nor UNWEIGHTED_CYCLES
 *        4. on the word after 3:
 *           I_DETERMINISTIC                        minimize (MinimizeConfig::default()); every KO of wfst_minimize passes
 *                                                  through with its message unchanged (transducers, cyclic inputs)
 *           no I_DETERMINISTIC, ACYCLIC, acceptor  determinize (DeterminizeConfig::default()), minimize
 *           no I_DETERMINISTIC, ACYCLIC, transd.   encode(EncodeLabels), determinize, minimize, decode
 *                                                  (encode/encode_static.rs, decode_static.rs, table.rs)
 *           no I_DETERMINISTIC, no ACYCLIC         KO "optimize: inputs whose property word does not hold ACYCLIC are not
 *                                                  supported" (the reference encodes the weights and ends in the minimizer
 *                                                  for cyclic machines, which wfst_minimize does not support)
 *      encode: both labels of an arc become 1 + the index of the first occurrence of its (ilabel, olabel) pair in tr_map's
 *      scan order (state by state, arcs in stored order); weights and final weights stay, no superfinal state; the word is
 *      masked by i_label_invariant & o_label_invariant.  decode: the pair back through the table, the same mask, then
 *      rm_final_epsilon, which on a machine without eps:eps arcs is its closing connect (a transducer whose word holds
 *      NO_EPSILONS while its arcs do not is KO "eps:eps arcs under a property word that holds NO_EPSILONS are not supported").
 *      Differs from the reference in ONE respect: the encoded machine's word has lost ACCEPTOR, so the reference determinizes
 *      it by the gallic construction; here the acceptor construction runs, with the word of the gallic call
 *      (determinize_properties on the word without ACCEPTOR).  The two results are identical on a label-encoded machine
 *      (DESIGN.md 3.10).  So upload lattices with ACYCLIC in the word: step 4 branches on it.
 *      No start state: rm_epsilon returns its input, tr_map (encode, decode) returns at once, determinize yields the empty
 *      FST.  An input that trims to nothing ends as the empty FST.  A NEW handle; fst is left as it is. ---- */
wfst_status wfst_optimize(wfst_ctx* ctx, const wfst_fst* fst, wfst_fst** out);

/* ---- optimize of n FSTs in one call: outs[i] is a NEW handle, bit-identical to what wfst_optimize(ctx, fsts[i], ..)
 *      returns.  The same handle may appear more than once; n == 0: OK; the inputs are left exactly as they are.  Every
 *      branch is taken on the stored word, as in wfst_optimize, and every stage is ONE batch call over the items that take it:
 *        1. wfst_rm_epsilon_batch over the items whose word lacks NO_EPSILONS
 *        2. wfst_tr_sum_batch over every item
 *        3. on the word after 2: I_DETERMINISTIC -> 4; no I_DETERMINISTIC and no ACYCLIC -> KO with wfst_optimize's message;
 *           otherwise an item whose INPUT word holds ACCEPTOR goes through wfst_determinize_batch (KDELTA, Functional) and
 *           on to 4; any other item is a transducer and takes the single call's encode, determinize, minimize, decode on
 *           its own (there is no batch form of the label encoding)
 *        4. wfst_minimize_batch (KSHORTESTDELTA, allow_nondet = false)
 *      Launches: those of the four batch calls (the rule, the slab limit of 8 GiB with "split the list" and the growth of
 *      each are described with them), whatever n is, plus the single-call launches of every transducer and of every
 *      item that a stage hands to its single path.  Intermediate handles are destroyed on every exit.
 *      in_kernel (uint8_t[n], may be NULL): in_kernel[i] == 1 exactly when every stage item i went through ran it in that
 *      stage's batch kernel (for wfst_tr_sum_batch: at most 4096 states, 16384 arcs, no state with more than 256 arcs).
 *      A transducer has in_kernel[i] == 0.
 *      KO — NULL pointers, NULL list entries ("item <i>: null FST in batch") and handles of another device or context are
 *      checked before anything is launched.  Otherwise the answer is that of the loop `for i: wfst_optimize(fsts[i])`: the
 *      single call's message for the LOWEST failing index, prefixed by "item <i>: ".  The stages run on sublists, so when
 *      one reports item i, the call drops its intermediates and runs wfst_optimize's steps over items 0..i in index order
 *      to find the first failing one (a cold path).  Errors that belong to no item ("split the list", "did not converge")
 *      pass through unchanged.  On any KO every outs[i] is NULL, nothing is leaked and the context works afterwards. ---- */
wfst_status wfst_optimize_batch(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, wfst_fst** outs, uint8_t* in_kernel);
/* the last wfst_optimize_batch call of ctx: launches[4] = launches of the batch kernels of rm_epsilon, tr_sum, determinize
 *      and minimize; items by their in_kernel flag; and the transducers among the items_single.  Any pointer may be NULL.
 *      The per-stage getters (wfst_ctx_get_{rm_epsilon,tr_sum,determinize,minimize}_batch_stats) read as the last call of
 *      that stage, whoever made it. */
wfst_status wfst_ctx_get_optimize_batch_stats(wfst_ctx* ctx, uint64_t* launches /* [4]: rm_epsilon, tr_sum, determinize, minimize */,
                                              uint64_t* items_in_kernel, uint64_t* items_single, uint64_t* items_transducer);

/* ---- union, concat, closure: fst_union / fst_concat (rustfst-ffi/src/algorithms/{union,concat}.rs) =
 *      rustfst::algorithms::{union::union, concat::concat, closure::closure} (union/union_static.rs:55-118,
 *      concat/concat_static.rs:53-109, closure/closure_static.rs:25-73).  The reference changes its first operand in place;
 *      here *out is a NEW handle equal, bit for bit (state numbering, arc order, weights, start, property word), to what the
 *      reference leaves in that operand, and the inputs are left as they are (cached transposes, plans and words included).
 *      Results are in general NOT label-sorted (eps arcs are appended last): tr_sort before compose.
 *      union   compute_and_update_properties(INITIAL_ACYCLIC) on a first (a word that does not know the pair gets the four
 *              DFS pairs replaced by the searched ones; an arc into the start from a state the start cannot reach is a cross
 *              arc and leaves it INITIAL_ACYCLIC).  b without start state: a with that word.  Otherwise b's states follow
 *              a's (nextstate + n_states(a)) and: a without start state -> start(b) WITHOUT the offset, as the reference
 *              writes it, and b's word; a initial-acyclic -> 0:0/One -> start(b) + n(a) appended last to the start's row;
 *              else one new state behind b's, with 0:0/One -> start(a), 0:0/One -> start(b) + n(a), becomes the start.  Word:
 *              union_properties(props1, props2, false) (fst_properties/mutate_properties.rs:692-748).
 *      concat  a without start state: a.  Otherwise b's states follow a's; every state of a with Some(final weight w) gets
 *              0:0/w -> start(b) + n(a) appended last if b has a start state, and loses its final weight either way.  Word:
 *              concat_properties (:186-245) if b has a start state, else what add_state / set_final / add_tr /
 *              set_final(None) leave.
 *      closure closure_type 0 = ClosureStar, 1 = ClosurePlus (closure/mod.rs:9-12), anything else KO.  With a start state
 *              every final state gets 0:0/final weight -> start appended last (the weight stays).  Star: one new state, final
 *              with One, with 0:0/One -> old start if there was one, becomes the start.  Word: closure_properties (:114-145).
 *      union_list / concat_list: the left fold over fsts[0..n) (rustfst-python union_list / concat_list) in ONE call — the
 *              number of kernel launches does not depend on n.  n == 0: KO "fsts must be at least of len 1"; n == 1: a copy.
 *      KO before anything is launched: a NULL operand or list entry, an operand of another device or context, a result
 *      that could exceed 2^31 - 2 states or 2^32 - 1 arcs (the rule: wfst_rational_check_sizes below). ---- */
wfst_status wfst_union(wfst_ctx* ctx, const wfst_fst* a, const wfst_fst* b, wfst_fst** out);
wfst_status wfst_concat(wfst_ctx* ctx, const wfst_fst* a, const wfst_fst* b, wfst_fst** out);
wfst_status wfst_closure(wfst_ctx* ctx, const wfst_fst* f, uint32_t closure_type, wfst_fst** out);
wfst_status wfst_union_list(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, wfst_fst** out);
wfst_status wfst_concat_list(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, wfst_fst** out);

/* ---- replace: fst_replace (rustfst-ffi/src/algorithms/replace.rs) = rustfst::algorithms::replace::replace(fst_list, root,
 *      epsilon_on_replace) (replace/replace_static.rs:44-58): the recursive transition network over pairs[0..n), expanded from
 *      the FST whose label is `root`.  *out is a NEW handle equal, bit for bit (state numbering, arc order, labels, weights,
 *      start, final weights, property word), to what the reference returns; the inputs are left as they are (cached
 *      transposes, plans and words included).  Only the two-argument options of the reference's FFI exist:
 *      epsilon_on_replace != 0 makes call arcs 0:0, epsilon_on_replace == 0 makes them ilabel:0; return arcs are 0:0.
 *      The list  fst_id is the list position.  Of two entries with one label the LAST is the one that is called, and the
 *              root is the last entry whose label is `root`; the list length n is what a label is compared with for the
 *              "dense range" of the word.  No entry with label `root` (an empty list included): KO "ReplaceFstImpl: No FST
 *              corresponding to root label {root} in the input tuple vector".
 *      States  tuples (call stack, fst_id, state) in the first-touch order of the reference's FIFO search.  A state's arcs:
 *              first, if the stack is not empty and the state has Some(final weight w), the return arc 0:0/w into the
 *              caller's (fst_id, nextstate) under the popped stack; then its stored arcs in order.  An arc is a CALL iff its
 *              olabel is not 0, lies within [least label, greatest label] of the list and is a label of the list; it becomes
 *              (ilabel or 0):0/weight into the callee's start state under the stack + (this fst_id, the arc's nextstate), or
 *              is dropped when the callee has no start state.  Every other arc is copied.  A label-0 entry can be the root
 *              but is never called.  Only states of the root instance (empty stack) are final, with the root's weights.
 *              A root without a start state: the empty FST with the word of VectorFst::new().
 *      Word    replace_properties (replace_fst_op.rs:120-186, fst_properties/mutate_properties.rs:496-620) of the inputs'
 *              STORED words, stored as it is; never computed from the content.  The result is in general NOT label-sorted
 *              unless the word says so: tr_sort before compose.
 *      Cycles  the reference does not terminate on a grammar whose expansion reaches a recursive call.  Here such a call is
 *              KO "replace: cyclic dependency between the FSTs: the reference does not terminate on this input", found when
 *              a call stack holds more frames than the list has distinct labels; a recursive arc the expansion never reaches is harmless.
 *      KO before anything is launched: a NULL ctx or out, NULL pairs with n > 0 ("null pointer"), a NULL entry ("item {i}:
 *      null FST in list"), an entry of another device or context ("replace: item {i} lives on another device" / "belongs
 *      to another context"), the root error above.  A result beyond what the search's arena can hold (2^31 - 16 states or
 *      arcs; the reference's own limits are 2^31 - 2 states and 2^32 - 1 arcs) is KO "replace: result too large" or
 *      "replace: arena overflow after retries" from the driver's overflow path.  A recursive grammar that fans out may reach
 *      that limit before a stack is deep enough to prove the recursion: it is KO either way, with whichever message comes
 *      first.  Tropical weights only.
 *      WFST_REPLACE_PREFIX_SLOTS (tests): slots of the call-stack table at the first attempt, a power of two. ---- */
typedef struct {
  uint32_t label;
  const wfst_fst* fst;
} wfst_label_fst_pair; /* CLabelFstPair, rustfst-ffi/src/algorithms/replace.rs:11-16 */
wfst_status wfst_replace(wfst_ctx* ctx, uint32_t root, const wfst_label_fst_pair* pairs, size_t n, uint32_t epsilon_on_replace,
                         wfst_fst** out);
/* the last wfst_replace call of ctx (reset when the call begins; all 0 after a KO or an empty result, except the two growth
 *      counters): levels of the search, states and arcs of the result, distinct non-empty call stacks interned (prefixes), the
 *      deepest of them (max_depth), call arcs emitted, call arcs dropped for a callee without a start state, return arcs
 *      emitted, times the search's arena grew (arena_grows), times the expansion ran again with a call-stack table twice
 *      the size (prefix_reruns), and the level kernels queued over all attempts (level_launches: three per level, the levels
 *      queued behind the last one included).  The three arc counters are tallied while levels are emitted: a level that did not fit the
 *      arena and was emitted again counts twice (arena_grows tells; growth AHEAD of a level, the usual kind, does not).
 *      Any pointer after ctx may be NULL. */
wfst_status wfst_ctx_get_replace_stats(wfst_ctx* ctx, uint64_t* levels, uint64_t* states, uint64_t* arcs, uint64_t* prefixes,
                                       uint64_t* max_depth, uint64_t* call_arcs, uint64_t* dropped_calls, uint64_t* return_arcs,
                                       uint64_t* arena_grows, uint64_t* prefix_reruns, uint64_t* level_launches);

/* ---- state_sort, top_sort: fst_top_sort (rustfst-ffi/src/algorithms/top_sort.rs) = rustfst::algorithms::{state_sort,
 *      top_sort} (state_sort.rs:16-78, top_sort.rs:76-94).  The reference works in place; here a NEW handle is returned and
 *      fst, its cached derived data and its property word are left as they are.
 *      state_sort: state order[s] of the result holds state s's arcs in their stored order, nextstate = order[nextstate],
 *              and s's final weight; the start is order[start]; the word is word(fst) & statesort_properties()
 *              (fst_properties/properties.rs:319-348).  n_order != the number of states: KO "StateSort : Bad order vector
 *              size : {n_order}. Expected {n_states}".  An order that is not a permutation of the states (a debug_assert in
 *              the reference): KO "state_sort: order is not a permutation of the states", found on the device before
 *              anything is written.  No start state: a copy, word unchanged.
 *      top_sort: decided on the CONTENT, never on the stored word.  Acyclic: state_sort by the reference's order — the
 *              reverse finishing order of the depth-first search of dfs_visit.rs:97-187, roots the start state, then 0, 1,
 *              2, .., arcs in stored order — then ACYCLIC | INITIAL_ACYCLIC | TOP_SORTED set in the word and nothing
 *              cleared (set_properties_with_mask(p, p), vector_fst/mutable_fst.rs:411-414).  A cycle anywhere (a self loop,
 *              a cycle the start cannot reach): a copy with CYCLIC | NOT_TOP_SORTED set the same way — a stored ACYCLIC,
 *              INITIAL_ACYCLIC or TOP_SORTED stays.  No start state: without states a copy with the three acyclic bits, with
 *              states KO "StateSort : Bad order vector size : 0. Expected {n_states}" (the search returns an empty order).
 *              The order is computed level by level over the Kahn levels of the DAG: consecutive levels
 *              of at most 256 states inside one launch of one workgroup, a wider level by one device-wide launch per phase;
 *              WFST_TOP_SORT_PATH=auto|narrow|wide (tests) pins a regime, any other value is KO.  Every route returns the
 *              same FST. ---- */
wfst_status wfst_state_sort(wfst_ctx* ctx, const wfst_fst* fst, const uint32_t* order, size_t n_order, wfst_fst** out);
wfst_status wfst_top_sort(wfst_ctx* ctx, const wfst_fst* fst, wfst_fst** out);
/* the last wfst_top_sort call of ctx (reset when the call begins): Kahn levels peeled (levels; a cyclic input: those peeled
 *      before the peel ran dry), launches of the one-workgroup and of the device-wide level kernels over the four level
 *      phases peel, select, sizes, pre (narrow_launches, wide_launches; a cyclic input: the peel's only), levels peeled
 *      inside one-workgroup launches (narrow_levels), the widest level, the depth of the deepest state in the search forest
 *      (max_tree_depth: a root has 1), rows of the ancestor table (lift_rows: the least J >= 1 with 2^J > levels), states
 *      whose in-arcs come from at least two different states (states_compared: they needed a lifted comparison), states
 *      with 32 in-arcs or more, which a whole wave took (wave_states), and cyclic = 1 for the CYCLIC exit, after which
 *      max_tree_depth, lift_rows, states_compared and wave_states are 0.  Any pointer after ctx may be NULL. */
wfst_status wfst_ctx_get_top_sort_stats(wfst_ctx* ctx, uint64_t* levels, uint64_t* narrow_launches, uint64_t* wide_launches,
                                        uint64_t* narrow_levels, uint64_t* max_level_width, uint64_t* max_tree_depth,
                                        uint64_t* lift_rows, uint64_t* states_compared, uint64_t* wave_states, uint64_t* cyclic);

/* ---- top_sort of n FSTs in one call: outs[i] is a NEW handle, bit-identical (offsets, arcs with their weights' bit
 *      patterns, finals, start state, property word) to what wfst_top_sort(ctx, fsts[i], ..) returns: an acyclic item in
 *      the reference's depth-first order, an item with a cycle anywhere as a copy with CYCLIC | NOT_TOP_SORTED set (not an
 *      error), an item without states and without a start state as the empty FST with the three acyclic bits.  The same
 *      handle may appear more than once in fsts.  n == 0: OK.  The inputs are left exactly as they are, their cached
 *      derived data and property words included.
 *      One workgroup per item and ONE launch for the whole list, whatever its length and the items' depths: the
 *      workgroup stages the item's nextstate column and offsets in LDS as 16-bit words, ONE lane runs the reference's
 *      sequential search on them (explicit stack, white / grey / black, the first grey target ends it; a step bound of
 *      2 * states + arcs + 2 makes a search that does not end impossible), and all lanes apply the order as state_sort
 *      does (row lengths and finals scattered, a workgroup scan, arcs copied as 16-byte words with nextstate renamed) into
 *      the item's slice of one slab.  The slices are sized on the host from n_states and n_arcs alone, so nothing is run
 *      twice: one launch, one read-back of the items' control blocks, one adoption of all results out of the slab.  A
 *      slice takes 16 bytes per arc and 12 per state; the slices of one call may take 8 GiB together: a list that needs
 *      more is KO before anything is launched ("split the list").  The launch asks for the LDS of its largest item, at
 *      most 58 KB.
 *      in_kernel (uint8_t[n], may be NULL): in_kernel[i] == 1 exactly when item i has a start state, at most 4096 states
 *      and at most 16384 arcs, or has neither states nor a start state (such an item occupies no workgroup).
 *      in_kernel[i] == 0: the item went through wfst_top_sort unchanged — anything larger, which gives the same FST, and
 *      an item with states but no start state, which is that call's KO.  wfst_ctx_get_top_sort_stats keeps describing
 *      the last single call, one made for such an item included.
 *      KO — every argument is checked before anything is launched: NULL pointers, NULL list entries ("item <i>: null FST
 *      in batch"), a handle of another device or context ("item <i>: top_sort_batch: the FST belongs to another context").
 *      An item with states but no start state: "item <i>: StateSort : Bad order vector size : 0. Expected {n_states}", the
 *      lowest such i, as a loop of single calls would stop.  On any KO every outs[i] is NULL, nothing is leaked and the
 *      context works afterwards. ---- */
wfst_status wfst_top_sort_batch(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, wfst_fst** outs, uint8_t* in_kernel);
/* the last wfst_top_sort_batch call of ctx: launches of the batch kernel (0 when no item occupied a workgroup, else 1),
 *      items with in_kernel == 1, items that went through the single-FST path.  All 0 after a KO before any launch.  Any
 *      pointer after ctx may be NULL. */
wfst_status wfst_ctx_get_top_sort_batch_counters(wfst_ctx* ctx, uint64_t* launches, uint64_t* items_in_kernel, uint64_t* items_single);

/* ---- rm_epsilon: fst_rm_epsilon (rustfst-ffi/src/algorithms/rm_epsilon.rs) = rustfst::algorithms::rm_epsilon
 *      (rustfst/src/algorithms/rm_epsilon/rm_epsilon_static.rs:50-163) with its default configuration (connect, no
 *      thresholds): every epsilon:epsilon arc removed, the weighted relation kept, the result connected.  The reference
 *      works in place; here a NEW handle is returned.  An FST without a start state is returned unchanged. ---- */
wfst_status wfst_rm_epsilon(wfst_ctx* ctx, const wfst_fst* fst, wfst_fst** out);
/* the last wfst_rm_epsilon call of ctx (reset when the call begins; all 0 for an FST without a start state): batches of
 *      mutually independent states that were scheduled, launches of the one-thread-per-state and of the one-wave-per-state
 *      rewrite kernel, states that finished in either, and the largest closure capacity any launch was given.  Read-only
 *      diagnostics of how the scratch sizes were climbed; any pointer after ctx may be NULL. */
wfst_status wfst_ctx_get_rm_epsilon_stats(wfst_ctx* ctx, uint64_t* batches, uint64_t* thread_launches, uint64_t* wave_launches,
                                          uint64_t* states_thread, uint64_t* states_wave, uint64_t* max_closure_cap);
/* ---- rm_epsilon of n FSTs in one call: outs[i] is a NEW handle, bit-identical (offsets, arcs with their weights' bit
 *      patterns, finals, start state, property word) to what wfst_rm_epsilon(ctx, fsts[i], ..) returns.  The same handle may
 *      appear more than once in fsts.  n == 0: OK.  The inputs are left exactly as they are, their cached derived data and
 *      property words included.  An item without a start state is returned as the single call returns it (a copy), and an
 *      item without states never occupies a workgroup; both count as in_kernel == 1.
 *      One workgroup per item: it runs every stage of the single call on its item inside the item's slice of one slab —
 *      noneps_in, the epsilon depths by peeling the sinks of the epsilon graph, the rewrites depth by depth (one thread per
 *      state, a barrier between depths), the CSR of the result with the facts for the property word, connect.
 *      in_kernel (uint8_t[n], may be NULL): in_kernel[i] == 1 exactly when
 *        - item i has at most 4096 states and at most 16384 arcs,
 *        - its epsilon graph (the 0:0 arcs) has no cycle, a self loop being one, and
 *        - every state the reference rewrites (the start state and every state with a non-epsilon incoming arc) fits the
 *          last rung of the single call's one-thread kernel: a closure of at most 64 states, at most 128 entries on the
 *          depth-first stack, at most 128 arcs after combining (64 / 128 / 128).
 *      The kernel finds whichever condition fails and leaves an exit code; in_kernel[i] == 0: the item went through
 *      wfst_rm_epsilon unchanged.
 *      Launches: ONE launch for every item that is still open.  The first launch's slices are sized on the host from
 *      n_states and n_arcs alone (nothing is read from the device): an arc arena of 2 * n_arcs + 64 arcs, so every item whose
 *      result before connect has no more arcs than its input (and up to twice as many) finishes in the first launch.  An item whose arena proves too small
 *      reports what it needed and runs again in the next launch of the same call with an arena at least twice as large; at
 *      most 64 launches.  The number of launches depends neither on n nor on any item's epsilon depth.  Per launch: the
 *      kernel and one read-back of the control blocks; per call one adoption of all kernel results out of the slabs.
 *      The slices of one launch may take 8 GiB together: a list that needs more is KO before that launch ("split the list").
 *      WFST_RM_EPSILON_BATCH_ARENA=min (tests) makes the first launch's arenas as small as the kernel allows, so that every
 *      item with arcs grows; any other value is KO.
 *      KO — every argument is checked before anything is launched: NULL pointers, NULL list entries ("item <i>: null FST
 *      in batch"), a handle of another device or context — and whenever wfst_rm_epsilon would be KO for an item: that
 *      call's message for the LOWEST failing index, prefixed by "item <i>: ".  On any KO every outs[i] is NULL, nothing is
 *      leaked and the context works afterwards.  The counters of wfst_ctx_get_rm_epsilon_stats are not specified after a
 *      batch call. ---- */
wfst_status wfst_rm_epsilon_batch(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, wfst_fst** outs, uint8_t* in_kernel);
/* the last wfst_rm_epsilon_batch call of ctx: launches of the batch kernel, items it finished (in_kernel == 1), items that
 *      went through the single-FST path.  All 0 after a KO before any launch. */
wfst_status wfst_ctx_get_rm_epsilon_batch_stats(wfst_ctx* ctx, uint64_t* launches, uint64_t* items_in_kernel,
                                                uint64_t* items_single);

/* ---- the re-armed scratch of the single-shortest-path relaxation: a predicted mailbox solve has its scratch
 *      cleaned on the device BEHIND its result and parks it on the context; the next solve with the same graph structure and
 *      schedule on that context adopts it and starts without a set-up launch.  Counters of ctx since its creation: solves that
 *      parked their scratch (armed), solves that started from parked scratch (adopted), and parked scratch that was given back
 *      unused (dropped).  Any pointer after ctx may be NULL.  WFST_SSSP_REARM=0 switches the mechanism off. ---- */
wfst_status wfst_ctx_get_rearm_stats(wfst_ctx* ctx, uint64_t* armed, uint64_t* adopted, uint64_t* dropped);
/* ---- the bounded head of the single-shortest-path relaxation: where no arc or final weight is negative, the
 *      first launch of a repeated wfst_shortest_path(nshortest = 1) query ends the search as soon as the best final state is
 *      settled and nothing pending can come in at or below its total (the textbook early stop); the returned path, weight and
 *      tied_choices are those of the full solve.  Counters of ctx since its creation: queries the head ended (stops), queries of
 *      the large-FST route that ran the full solve (full_solves), and why the last of those did (last_reason: a static string,
 *      "" before the first; not to be freed).  Any pointer after ctx may be NULL.  WFST_SSSP_BOUNDED=0 switches it off;
 *      wfst_shortest_distance, n-best queries, reweight and push_weights never use it. ---- */
wfst_status wfst_ctx_get_bounded_stats(wfst_ctx* ctx, uint64_t* stops, uint64_t* full_solves, const char** last_reason);
/* ---- the solo query: once three queries in a row on ctx have been ended by the bounded head (or by this
 *      route) and the cleaned scratch of the last is parked on ctx for the same graph structure, first band and knobs, the next
 *      such query is ONE launch of one workgroup that searches, finds the path, writes it to pinned memory and puts the keys it
 *      wrote back, so that the parked scratch is armed as before.  A launch that cannot answer (a best total beyond the first
 *      band, a level wider than its workgroup, a full log of written keys) gives the query up: it is asked again by the
 *      ordinary route, and the next queries are ordinary until three stop in a row again.  Results and the other counters
 *      (wfst_stats.sweeps == 1, stops, armed, adopted, tied_choices) are those of the bounded stop it replaces.  Counters of
 *      ctx since its creation: launches (attempts), those that answered, those that gave up (aborted), why the last of those
 *      did (last_abort: 0 none yet, 1 band, 2 level outgrown, 3 log full, 4 other), and the keys the last launch put back
 *      (cleaned).  Any pointer after ctx may be NULL.  WFST_SSSP_SOLO=0 switches the route off; =2 tries it whatever the
 *      streak and makes the call KO, after the query, with the reason unless the solo launch answered. ---- */
wfst_status wfst_ctx_get_solo_query(wfst_ctx* ctx, uint64_t* attempts, uint64_t* answered, uint64_t* aborted, uint64_t* last_abort,
                                    uint64_t* cleaned);
/* tests: the words of ctx's parked key array that are not +inf — an armed scratch has none.  Synchronises the context's
 *      stream.  KO, and 0 words, when nothing is parked on ctx. */
wfst_status wfst_ctx_parked_key_check(wfst_ctx* ctx, uint64_t* not_inf);
/* hipFree of every block the context's device pool holds without an owner: cached blocks and parked scratch (the pool does
 *      the same by itself when an allocation fails).  Synchronises the device.  Live buffers are not touched. */
wfst_status wfst_ctx_trim_pool(wfst_ctx* ctx);

/* ---- project: fst_project (rustfst-ffi/src/algorithms/project.rs:45-70) = rustfst::algorithms::project
 *      (rustfst/src/algorithms/projection.rs:65-95), in place on the device-resident arcs.  project_output == 0:
 *      ProjectType::ProjectInput (olabel := ilabel), != 0: ProjectOutput (ilabel := olabel); the property word follows
 *      project_properties (fst_properties/mutate_properties.rs:365-445).  The usual recipe around the hot path is
 *      compose -> project -> shortest_path (rustfst/src/lib.rs:70-82). ---- */
wfst_status wfst_fst_project(wfst_ctx* ctx, wfst_fst* fst, int project_output);

/* ---- invert: rustfst::algorithms::invert (rustfst/src/algorithms/inversion.rs:32-48), in place on the device-resident
 *      arcs like wfst_fst_project: every arc's ilabel and olabel change places (one grid-stride kernel), and the property
 *      word becomes invert_properties(word) (fst_properties/mutate_properties.rs:302-363): the tape-neutral pairs stay,
 *      every input-side pair (deterministic, epsilons, label-sorted) changes places with its output-side pair — so a
 *      handle that wfst_fst_tr_sort sorted on one tape is known to be sorted on the other afterwards.  Everything the
 *      handle derives from the labels follows: the per-state epsilon facts are derived again, the host mirror and the
 *      cached host reverse are dropped, the input-epsilon answer and the string shape are asked again.  An FST without
 *      arcs only gets the new word.  Inverting twice restores arrays and word bit for bit.
 *      KO: NULL pointers ("null pointer"); a handle of another device or context ("invert: the FST lives on another
 *      device", "invert: the FST belongs to another context"). ---- */
wfst_status wfst_fst_invert(wfst_ctx* ctx, wfst_fst* fst);

/* ---- isomorphic: rustfst::algorithms::isomorphic_with_config (rustfst/src/algorithms/isomorphic.rs:134-158, 200-212)
 *      for two handles of ctx.  cfg == NULL: IsomorphicConfig::default(), delta = KDELTA = 1/1024.  OK with
 *      *is_isomorphic = 0 or 1, or KO with the reference's message "Isomorphic: Non-determinism as an unweighted
 *      automaton. state1 = {s1} state2 = {s2}".  Both operands, their cached derived data and their property words are
 *      left as they are.
 *      The reference's semantics, reproduced and not improved:
 *        - both operands without a start state: 1; exactly one without: 0 (both before any GPU work);
 *        - no comparison of state counts and no injectivity check: only states of fst1 are recorded as paired, so two
 *          states of fst1 may pair with one state of fst2, the call is NOT symmetric in its operands, and states the
 *          search does not reach are never looked at;
 *        - per pair popped from the FIFO queue, in this order: final weights (none / none equal, both present by
 *          approx_equal), arc counts, then both arc lists sorted by tr_compare = (ilabel, olabel, weight, nextstate) and
 *          walked index by index: ilabel, olabel, approx_equal of the weights, pair_state(next1, next2) — the first
 *          pairing of a state of fst1 wins — and only after a successful pairing the non-determinism mark, set when arc i
 *          and arc i - 1 of fst1 agree in labels and approx-equal weight;
 *        - approx_equal(a, b) is |a - b| <= delta with IEEE semantics: two +inf arc weights are NOT approx-equal, so an
 *          FST with an infinite arc weight is not isomorphic to itself;
 *        - the sort compares weights in OrderedFloat's total order on the exact bits (-0.0 == +0.0, NaN greatest and
 *          equal to itself); only the walk compares approximately;
 *        - the first failure in queue order gives the KO above, naming that pair, iff a mark was set strictly before
 *          it in sequential order, otherwise 0.
 *      Final weights are what the handle stores: +inf is "not final", as everywhere in this library, so the reference's
 *      (Some(inf), Some(inf)) case (two final states with weight zero(), not approx-equal) cannot be expressed: such
 *      states count as not final on both sides, which is equal.
 *      The search runs level by level over two temporary copies of the arcs in tr_compare order: every
 *      arc slot of a level has its position in the reference's sequential order, pairings, marks and failures are
 *      decided by atomic minima on positions, and the next level is written in that order.  Two regimes: consecutive
 *      levels of at most WFST_ISOMORPHIC_NARROW_PAIRS pairs and WFST_ISOMORPHIC_NARROW_EVENTS arc slots run inside one
 *      launch of one workgroup; a larger level takes one device-wide launch per phase and one read-back.  A pair whose
 *      fst1 state has 64 arcs or more is walked by a whole wave in both.  WFST_ISOMORPHIC_PATH=auto|narrow|wide (tests)
 *      pins a regime.  Every route gives the same verdict and the same message.
 *      Scratch comes from the context's pool and goes back at the end, also on KO: 16 bytes per arc of each operand,
 *      32 bytes per state and 8 bytes per arc of fst1 (pairings, two queues, slot offsets and counts, one level's flags
 *      and their scan).  A refused allocation is an ordinary KO and the context works afterwards.  An operand with
 *      2^32 - 2 arcs or more is KO (positions are 32-bit).
 *      KO before any GPU work, in this order: NULL pointers ("null pointer"); a handle of another device or context
 *      ("isomorphic: fst1 lives on another device", "isomorphic: fst2 belongs to another context"); a value of
 *      WFST_ISOMORPHIC_PATH other than auto, narrow or wide. ---- */
#define WFST_ISOMORPHIC_NARROW_PAIRS 256
#define WFST_ISOMORPHIC_NARROW_EVENTS 2048
typedef struct { float delta; } wfst_isomorphic_config;   /* NULL = IsomorphicConfig::default() = KDELTA */
wfst_status wfst_isomorphic(wfst_ctx* ctx, const wfst_fst* fst1, const wfst_fst* fst2, const wfst_isomorphic_config* cfg,
                            int* is_isomorphic);
/* the last wfst_isomorphic call of ctx (reset when a call has passed its checks): levels of the search that ran, the
 *      failing one included; launches of the one-workgroup kernel and of the device-wide phase kernels (four per wide
 *      level); levels that ran inside one-workgroup launches; the widest level in pairs; pairs and arc slots of the
 *      levels that ran; pairs that a whole wave walked; states of both operands with more than 256 arcs, which the
 *      segmented radix passes sorted; non-determinism marks made (those of the failing level behind the failure
 *      included).  All 0 for a call decided by the start states.  Any pointer after ctx may be NULL. */
wfst_status wfst_ctx_get_isomorphic_counters(wfst_ctx* ctx, uint64_t* levels, uint64_t* narrow_launches, uint64_t* wide_launches,
                                             uint64_t* narrow_levels, uint64_t* max_level_width, uint64_t* pairs, uint64_t* events,
                                             uint64_t* wave_pairs, uint64_t* big_states_sorted, uint64_t* nondet_marks);

/* ---- paths: Fst::paths_iter (rustfst/src/fst_traits/paths_iterator.rs:24-62, under rustfst-python's string_paths) of
 *      one handle or of a list of handles of ctx, as a table in HBM: every successful path from the start state to a
 *      final state, in the order the reference's iterator yields them, bit for bit.  The operands are left as they are.
 *        - a path is its input labels and its output labels with label 0 dropped per tape (fst_path.rs:35-45: the two
 *          lists may differ in length) and weight = ((one (x) w1) (x) w2 ...) (x) final, left to right: f32 additions
 *          in path order, +inf absorbing;
 *        - the order is (number of arcs, arc positions read lexicographically): the reference's FIFO of prefixes is
 *          always sorted that way.  Parallel arcs to one state are distinct paths;
 *        - no states or no start state: no paths, OK.  A final start state: the empty path with its final weight;
 *        - a cycle that is ACCESSIBLE from the start state, whether or not it reaches a final state: KO "paths: a
 *          cycle is accessible from the start state: the reference's paths_iter never returns" (the reference would
 *          push prefixes for ever).  A cycle among states the start does not reach is no error.  The stored property
 *          word is not consulted: the peel that counts the paths decides from the content;
 *        - counts are u64 with saturating addition.  A count above max_paths — a saturated one always — is KO "paths:
 *          the FST has <N> paths, more than max_paths (<M>)", decided before any per-path memory is allocated; for a
 *          saturated count N is 18446744073709551615 and the same text goes on ": the count is saturated".  A
 *          table holds at most 2^32 - 2 paths; a refused allocation is an ordinary KO.
 *      wfst_fst_count_paths: the count alone, saturated at UINT64_MAX; KO on an accessible cycle.
 *      wfst_fst_paths: one FST of any size — accessibility and the count take one launch per level of the graph.
 *      wfst_fst_paths_batch: n FSTs into ONE table, max_paths applying per item.  The items of at most
 *      WFST_PATHS_BATCH_MAX_STATES states and WFST_PATHS_BATCH_MAX_ARCS arcs are counted by one launch, one workgroup
 *      each (in_kernel[i] = 1; items without states or start state too, they need no launch); an item beyond either
 *      limit is counted as wfst_fst_paths counts it (in_kernel[i] = 0).  The unranking, the sort and the emission run
 *      once over all paths of all items, so the call's launch count depends neither on n nor on the items' depths.
 *      Item for item the rows are those of the single call.  in_kernel may be NULL.  n == 0: OK, a table of no items.
 *      KO — checked before anything is launched: NULL ctx, fst / fsts or out ("null pointer"), NULL list entries ("item
 *      <i>: null FST in batch"), a handle of another device or context ("paths: the FST belongs to another context",
 *      "item <i>: paths_batch: the FST lives on another device").  The KOs of an item carry "item <i>: " in front, the
 *      lowest failing i first, as a loop of single calls would stop.  On any KO *out is left as it was.
 *      A wfst_paths lives until wfst_paths_destroy, independent of the FSTs it came from.  wfst_paths_info: items,
 *      paths, and the total numbers of input and output labels (any pointer may be NULL).  wfst_paths_download copies
 *      out item_off[n_items + 1] (rows of item i: item_off[i] .. item_off[i + 1]), weights[n_paths],
 *      ilabel_off[n_paths + 1] with ilabels[n_ilabels], olabel_off[n_paths + 1] with olabels[n_olabels]; any pointer
 *      may be NULL. ---- */
#define WFST_PATHS_BATCH_MAX_STATES 4096
#define WFST_PATHS_BATCH_MAX_ARCS 16384
typedef struct wfst_paths wfst_paths;
wfst_status wfst_fst_count_paths(wfst_ctx* ctx, const wfst_fst* fst, uint64_t* count);
wfst_status wfst_fst_paths(wfst_ctx* ctx, const wfst_fst* fst, uint64_t max_paths, wfst_paths** out);
wfst_status wfst_fst_paths_batch(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, uint64_t max_paths, wfst_paths** out,
                                 uint8_t* in_kernel);
wfst_status wfst_paths_info(const wfst_paths* paths, uint64_t* n_items, uint64_t* n_paths, uint64_t* n_ilabels, uint64_t* n_olabels);
wfst_status wfst_paths_download(wfst_ctx* ctx, const wfst_paths* paths, uint64_t* item_off, float* weights, uint64_t* ilabel_off,
                                uint32_t* ilabels, uint64_t* olabel_off, uint32_t* olabels);
wfst_status wfst_paths_destroy(wfst_paths* paths);
/* the last wfst_fst_count_paths / wfst_fst_paths / wfst_fst_paths_batch call of ctx (reset when a call begins, also when
 *      an argument is refused): kernel launches and library calls (a rocPRIM sort or scan counts as one) of the call;
 *      items counted by the one-workgroup kernel (those without a start state among them) and by the device-wide
 *      route; the deepest peel of an item, in levels; the paths counted, saturating, up to and including a refused
 *      item; the arcs of the table's longest path; items whose count saturated.  Any pointer after ctx may be NULL. */
wfst_status wfst_ctx_get_paths_counters(wfst_ctx* ctx, uint64_t* launches, uint64_t* items_in_kernel, uint64_t* items_single,
                                        uint64_t* levels, uint64_t* paths, uint64_t* max_path_arcs, uint64_t* saturated);

/* ---- look-ahead composition: the configuration rustfst-cli/src/cmds/compose.rs:77-181 (ComposeType::LookAhead) and
 *      rustfst/src/tests_openfst/algorithms/compose.rs:118-254 build by hand — there is no single reference entry point:
 *        graph1look = MatcherFst::new_with_relabeling(fst1, &mut fst2, true)        (compose/matcher_fst.rs:73-94)
 *        M1 = LabelLookAheadMatcher<SortedMatcher> with OUTPUT_LOOKAHEAD_MATCHER | LOOKAHEAD_WEIGHT | LOOKAHEAD_PREFIX |
 *             LOOKAHEAD_EPSILONS | LOOKAHEAD_NON_EPSILON_PREFIX, M2 = SortedMatcher
 *        filter = PushLabels(PushWeights(LookAhead(AltSequence))) with SMatchOutput  (compose/lookahead_filters/...)
 *        ComposeFst::new_with_options(..).compute()                                   (no connect)
 *      wfst_lookahead_create  = MatcherFst::new on fst1: LabelReachable::compute_data(fst1, reach_input = false)
 *        (compose/label_reachable.rs:135-273, host) + fst1's olabels relabelled and re-sorted (:63-93); the relabelled FST
 *        and the per-state reachable-label intervals live in HBM.  KO "StateReachable: Final state contained in a cycle"
 *        like the reference (state_reachable.rs:62-64).
 *      wfst_lookahead_relabel = LabelLookAheadRelabeler::relabel(fst2, .., relabel_input = true) + tr_sort(ILabelCompare)
 *        (lookahead_matchers/label_lookahead_relabeler.rs:27-41, cmds/compose.rs:151): a NEW handle; labels fst1 never
 *        emits get fresh indices, the map inside `la` grows as the reference's does.
 *      wfst_compose_lookahead = the composition itself on the GPU; output numbered like LazyFst::compute, not connected.
 *      The handle owns the relabelled fst1 (wfst_lookahead_fst1 lends it: it must not be edited in place with
 *      wfst_fst_tr_sort, wfst_fst_project or wfst_fst_set_start, the reachability data describes it as it is). ---- */
typedef struct wfst_lookahead wfst_lookahead;
wfst_status wfst_lookahead_create(wfst_ctx* ctx, const wfst_fst* fst1, wfst_lookahead** out);
wfst_status wfst_lookahead_relabel(wfst_lookahead* la, const wfst_fst* fst2, wfst_fst** out);
wfst_status wfst_lookahead_fst1(const wfst_lookahead* la, const wfst_fst** out);
wfst_status wfst_compose_lookahead(wfst_ctx* ctx, const wfst_lookahead* la, const wfst_fst* relabeled_fst2, wfst_fst** out);
/* n independent look-ahead compositions against the same first operand in ONE launch (one wavefront per problem, like
 * wfst_compose_shortest_path_batch); outs[i] == wfst_compose_lookahead(ctx, la, relabeled_fst2s[i]).  On KO no output is
 * left allocated. */
wfst_status wfst_compose_lookahead_batch(wfst_ctx* ctx, const wfst_lookahead* la, const wfst_fst* const* relabeled_fst2s,
                                         size_t n, wfst_fst** outs);
/* which route answered the compositions of the last wfst_compose_lookahead / wfst_compose_lookahead_batch call of ctx (reset
 * when the call begins; every route returns the same FST).  With m = the items that have a start state: one launch of the
 * single-wave kernel takes the m compositions, one wave each, in arenas of S = 2 * 2048 + 256 = 4352 states, A = 4 * S =
 * 17408 arcs and H = pow2(2 * S + 128) = 16384 table slots.  A wave gives up once its result passes 2048 states at the end
 * of a level that found new states, or a level adds more than 256 states; with m == 1 the limits are 512 and 48
 * (one_limits = 1).  items: n; items_no_start: items without a start state (the empty FST, nothing launched);
 * wave_answered: compositions the single-wave kernel finished; handed_over_states: it gave up with more states than the state
 * limit in force; handed_over_width: it gave up otherwise (a level wider than the width limit); overflow_arcs /
 * overflow_states: its arena's arcs / states were full; wide_items: compositions the wide driver ran (the four before it
 * summed; all m under WFST_LOOKAHEAD_PATH=wide, where nothing else counts); wave_regrows: under WFST_LOOKAHEAD_PATH=wave
 * (no hand-over, one_limits = 0) the lone launches that redo a composition whose arena was full, S = 16 * 2048 and four times
 * that per attempt, the successful one included; wide_grows: growths of the wide driver's arena; wide_hinted: compositions
 * whose wide arena was raised by the size the handle's last wide result left (applies when the arcs of the two second
 * operands are within a factor of two); hint_fallbacks: such an allocation was refused and the unhinted estimate used.  Any
 * out-pointer may be NULL. */
wfst_status wfst_ctx_get_lookahead_stats(wfst_ctx* ctx, uint64_t* items, uint64_t* items_no_start, uint64_t* wave_answered,
                                         uint64_t* handed_over_states, uint64_t* handed_over_width, uint64_t* overflow_arcs,
                                         uint64_t* overflow_states, uint64_t* wide_items, uint64_t* wave_regrows,
                                         uint64_t* wide_grows, uint64_t* wide_hinted, uint64_t* hint_fallbacks,
                                         uint64_t* one_limits);
wfst_status wfst_lookahead_destroy(wfst_lookahead* la);
/* LabelReachableData of a look-ahead handle: sizes, then the arrays (interval_offsets[n_states + 1], intervals[2 *
 * n_intervals] = half-open [begin, end) pairs over relabelled labels, labels[n_labels] ascending with their indices;
 * the NO_LABEL entry is the final label).  Any output may be NULL. */
wfst_status wfst_lookahead_info(const wfst_lookahead* la, uint32_t* n_states, uint64_t* n_intervals, uint32_t* n_labels,
                                uint32_t* final_label);
wfst_status wfst_lookahead_download(const wfst_lookahead* la, uint32_t* interval_offsets, uint32_t* intervals,
                                    uint32_t* labels, uint32_t* indices);
/* host-only handle (no GPU, no relabelled FST): LabelReachable::compute_data on flat CSR arrays (offsets[n_states + 1],
 * arcs, finals with +inf = not final).  Serves wfst_lookahead_info / _download / _destroy only. */
wfst_status wfst_label_reachable_compute(uint32_t n_states, const uint32_t* offsets, const wfst_tr* arcs, const float* finals,
                                         int reach_input, wfst_lookahead** out);

/* asynchronous form of wfst_shortest_path for nshortest == 1: _begin queues the relaxation (and, from the second
 * query of an FST on, the final-state search, backtrace and read-back behind it) on ctx's stream and returns; _end
 * waits, continues the relaxation if it needed more sweeps than the previous query, and returns the same FST the
 * synchronous call returns, freeing the job (also on error; out == NULL abandons it).  One job in flight per context
 * and no other call on that context between _begin and _end; fst must stay alive until _end.  cfg as in
 * wfst_shortest_path; nshortest != 1 -> KO "unsupported". */
typedef struct wfst_sp_job wfst_sp_job;
wfst_status wfst_shortest_path_begin(wfst_ctx* ctx, const wfst_fst* fst, const wfst_shortest_path_config* cfg,
                                     wfst_sp_job** job);
wfst_status wfst_shortest_path_end(wfst_sp_job* job, wfst_fst** out);

/* asynchronous form of the fused batch: _begin enqueues the whole pipeline on ctx's stream and returns at once
 * (so that the caller can issue other work, e.g. wfst_shortest_path on ANOTHER context, which then overlaps on
 * the GPU); _end waits, fills outs[0..n) / composed_arcs exactly like the synchronous call and frees the job
 * (also on error).  One job in flight per context; acceptors and t must stay alive until _end.
 * The outs[] of a batch of up to a few thousand strings are views into the batch's pinned result block: complete FST
 * handles whose arrays are built on first access (download, an algorithm, a writer); see INTEGRATION.md. */
typedef struct wfst_batch_job wfst_batch_job;
wfst_status wfst_compose_shortest_path_batch_begin(wfst_ctx* ctx, const wfst_fst* const* acceptors, size_t n,
                                                   const wfst_fst* t, const wfst_compose_config* ccfg,
                                                   const wfst_shortest_path_config* scfg, wfst_batch_job** job);
wfst_status wfst_compose_shortest_path_batch_end(wfst_batch_job* job, wfst_fst** outs, uint64_t* composed_arcs);

/* ---- reverse (rustfst/src/algorithms/reverse.rs:33-87; FFI fst_reverse): state 0 of the result is a new super-initial
 *      state with one eps:eps arc per final state of fst (weight = its final weight), state s + 1 holds the arcs INTO s
 *      turned around, in (source state, arc position) order; start + 1 is final with weight one.  The transpose is built
 *      on the GPU and cached on the handle (the n > 1 shortest-path search uses the same one). ---- */
wfst_status wfst_reverse(wfst_ctx* ctx, const wfst_fst* fst, wfst_fst** out);

/* ---- tr_sort (rustfst/src/algorithms/tr_sort.rs:13-62; FFI fst_tr_sort, rustfst-ffi/src/algorithms/tr_sort.rs:15):
 *      in-place, stable, per-state sort of the device-resident arcs by ilabel (ilabel_cmp != 0, ILabelCompare)
 *      or olabel (OLabelCompare), followed by the reference's property update.  This is what makes an FST
 *      acceptable to wfst_compose (SortedMatcher needs the sorted bit). ---- */
wfst_status wfst_fst_tr_sort(wfst_ctx* ctx, wfst_fst* fst, int ilabel_cmp);

/* ---- set_start on a device-resident handle (MutableFst::set_start, rustfst/src/fst_impls/vector_fst/mutable_fst.rs:35-44;
 *      FFI vec_fst_set_start, rustfst-ffi/src/fst/vector_fst.rs:26-33): KO "The state {state} doesn't exist" for a state beyond
 *      the FST, otherwise the start state and the property word change as the reference's do (set_start_properties,
 *      fst_properties/mutate_properties.rs:7-13); the arcs stay where they are in HBM and everything cached on the handle that
 *      does not depend on the start state (region plan, transpose, packed arcs) is kept — a shortest_path query per source on
 *      one resident FST is this call + wfst_shortest_path (ABI 7).  Like every mutation of a handle: not while a query on it
 *      is in flight on any context. ---- */
wfst_status wfst_fst_set_start(wfst_ctx* ctx, wfst_fst* fst, uint32_t state);

/* ---- fused batch: for each acceptor i: shortest_path(compose(acceptors[i], t)) — the loop a
 * caller writes around the two reference entry points; here one device-resident pipeline.
 * outs[i] are small host-resident FSTs. composed_arcs (may be NULL) receives the total number of
 * arcs emitted by the n compositions before trimming. ---- */
wfst_status wfst_compose_shortest_path_batch(wfst_ctx* ctx, const wfst_fst* const* acceptors, size_t n,
                                             const wfst_fst* t, const wfst_compose_config* ccfg,
                                             const wfst_shortest_path_config* scfg, wfst_fst** outs,
                                             uint64_t* composed_arcs);

/* ---- fused batch with matcher configs: for each acceptor i, outs[i] is bit for bit what
 *      wfst_shortest_path(wfst_compose_with_matchers(acceptors[i], t, ccfg, m1, m2), scfg) returns, property word included;
 *      m1 is the matcher of every acceptors[i] (side 1), m2 the matcher of t (side 2).  With m1 == m2 == NULL the call is
 *      wfst_compose_shortest_path_batch.  Otherwise outs[0..n) are zeroed before anything is looked at, and composed_arcs (may be
 *      NULL) receives the sum of the compositions' arc counts before trimming.
 *      Routes: items that are linear epsilon-free acceptors of at most 2048 states, against a t that has arcs, is known
 *      ilabel-sorted and has no input epsilons, with compose_filter 3 (Sequence) and m1 == NULL, run one wavefront each in ONE
 *      launch whatever n is; an item whose composition has a BFS level of more than 64 states or more states than its
 *      wavefront's slice of LDS holds is handed back.  Handed-back items and all others go one by one through the two calls
 *      above on ctx, in item order.
 *      KO: a null pointer "null pointer" (no GPU is touched); "unknown compose_filter"; nshortest != 1 "unsupported: nshortest !=
 *      1 in the fused batch"; then the set-up errors of wfst_compose_with_matchers in its order (unknown rewrite_mode, sigma_label
 *      0, AutoFilter with a matcher config, "cannot perform required matching (sort?)", the mode errors), decided for item 0
 *      first, then item 1 and so on, all before anything is launched; while composing, per item, "SigmaMatcher::Find: bad label
 *      (sigma)" and "Both sides can't require match": the call is KO with the message of the lowest failing item.  After a KO
 *      every outs[i] is NULL and the context works on. ---- */
wfst_status wfst_compose_shortest_path_batch_with_matchers(wfst_ctx* ctx, const wfst_fst* const* acceptors, size_t n, const wfst_fst* t,
                                                           const wfst_compose_config* ccfg, const wfst_matcher_config* m1,
                                                           const wfst_matcher_config* m2, const wfst_shortest_path_config* scfg,
                                                           wfst_fst** outs, uint64_t* composed_arcs);
/* the last wfst_compose_shortest_path_batch_with_matchers call of ctx that had a matcher config (reset when it begins): launches
 * of the wave-per-item kernel, items it answered, items it handed back, items never sent to it, then — summed over the items
 * the kernel answered — items of t's matcher that its sorted matcher answered, that its sigma arcs answered, the arcs those
 * emitted, items the allowed set refused, and the widest BFS level among them.  Any out-pointer may be NULL.  (Like
 * wfst_ctx_get_compose_sigma_counters: outside the table of the wfst_ctx_get_*_stats families.) */
wfst_status wfst_ctx_get_sigma_batch_counters(wfst_ctx* ctx, uint64_t* launches, uint64_t* items_in_kernel, uint64_t* items_handed_back,
                                              uint64_t* items_loop, uint64_t* exact_items, uint64_t* sigma_items, uint64_t* sigma_arcs,
                                              uint64_t* refused_items, uint64_t* max_level_width);

/* ---- host-side mutable VectorFst<TropicalWeight> mirror.  What rustfst-ffi exposes as vec_fst_* /
 * fst_* (rustfst-ffi/src/fst/vector_fst.rs:13-354, src/fst/mod.rs:128-216, src/algorithms/tr_sort.rs:15)
 * for callers that have no Rust VectorFst of their own (the Python mirror, C/C++ programs).  Semantics
 * incl. the property bookkeeping follow rustfst/src/fst_impls/vector_fst/mutable_fst.rs:25-281 and
 * rustfst/src/fst_properties/mutate_properties.rs.  A Rust shim does NOT need these: it flattens its own
 * VectorFst through the trait surface and calls wfst_fst_upload. ---- */
typedef struct wfst_vec_fst wfst_vec_fst;
wfst_status wfst_vec_fst_new(wfst_vec_fst** out);                                   /* vec_fst_new :13 */
wfst_status wfst_vec_fst_destroy(wfst_vec_fst* f);                                  /* fst_destroy mod.rs:376 */
wfst_status wfst_vec_fst_copy(const wfst_vec_fst* f, wfst_vec_fst** out);           /* vec_fst_copy :285 */
wfst_status wfst_vec_fst_add_state(wfst_vec_fst* f, uint32_t* state);               /* vec_fst_add_state :56 */
wfst_status wfst_vec_fst_add_tr(wfst_vec_fst* f, uint32_t state, const wfst_tr* tr); /* vec_fst_add_tr :83 */
wfst_status wfst_vec_fst_set_start(wfst_vec_fst* f, uint32_t state);                /* vec_fst_set_start :26 */
wfst_status wfst_vec_fst_set_final(wfst_vec_fst* f, uint32_t state, float weight);  /* vec_fst_set_final :39 */
wfst_status wfst_vec_fst_del_final_weight(wfst_vec_fst* f, uint32_t state);         /* vec_fst_del_final_weight :101 */
wfst_status wfst_vec_fst_num_states(const wfst_vec_fst* f, uint32_t* n);            /* vec_fst_num_states :248 */
wfst_status wfst_vec_fst_start(const wfst_vec_fst* f, int64_t* start);              /* fst_start mod.rs:128; -1 = None */
/* fst_final_weight mod.rs:143: *is_some = 0 for None */
wfst_status wfst_vec_fst_final_weight(const wfst_vec_fst* f, uint32_t state, float* weight, int* is_some);
wfst_status wfst_vec_fst_num_trs(const wfst_vec_fst* f, uint32_t state, uint64_t* n); /* fst_num_trs mod.rs:162 */
/* fst_get_trs mod.rs:179: copies the state's arcs into out[cap]; *n receives the count */
wfst_status wfst_vec_fst_get_trs(const wfst_vec_fst* f, uint32_t state, wfst_tr* out, uint64_t cap, uint64_t* n);
wfst_status wfst_vec_fst_properties(const wfst_vec_fst* f, uint64_t* props);
wfst_status wfst_vec_fst_tr_sort(wfst_vec_fst* f, int ilabel_cmp);                  /* fst_tr_sort tr_sort.rs:15 */
wfst_status wfst_vec_fst_equals(const wfst_vec_fst* a, const wfst_vec_fst* b, int* equal); /* vec_fst_equals :265 */
/* flatten through the trait surface + upload == the shim's input step */
wfst_status wfst_vec_fst_to_device(wfst_ctx* ctx, const wfst_vec_fst* f, wfst_fst** out);
/* download + rebuild (add_states / set_start / set_trs_unchecked / set_final / set_properties) == the shim's output step */
wfst_status wfst_vec_fst_from_device(const wfst_fst* fst, wfst_vec_fst** out);

/* shortest_path_with_config (shortest_path.rs:76-171) of n FSTs in one call; outs[i] = a new handle each.  With nshortest > 1
 * (unique = false) small inputs — the composed lattices of a decoding batch: BASELINE configs[4] — are searched by ONE
 * launch, one wavefront per input (distances, reverse, the reference's heap search, connect); with nshortest == 1 small
 * inputs (<= 4096 states) are likewise solved by one launch (keys in LDS, the canonical predecessor rule, the walk); larger
 * ones go through the single-FST paths one after the other; with unique = true the distances and arrays of all small inputs
 * come to the host in one launch and the host stages (reversal, determinization, search) run on host threads.  Same
 * results as n calls of wfst_shortest_path. */
wfst_status wfst_shortest_path_batch(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, const wfst_shortest_path_config* cfg,
                                     wfst_fst** outs);
/* ---- which path answered the small shortest-path queries of ctx: the counters of the two one-wavefront-per-FST kernels.
 *      An item that a kernel does not take, or hands back, goes through the general path and gives the same FST.
 *      nshortest == 1 (sp1_wave_kernel).  Offered to the kernel: an item of a wfst_shortest_path_batch list of at least two
 *      FSTs with at most 4096 states and at most 16384 arcs and no negative arc weight; a lone wfst_shortest_path (or a list
 *      of one) with at most 4096 states and at most 2048 arcs and no negative arc weight; with unique = true and
 *      nshortest > 1 (the kernel then exports distances and arrays) an item with a start state of a list of at least two,
 *      at most 4096 states and at most 16384 arcs.  Never with WFST_SP1_DEVICE=0 (except the export), with the reference
 *      tie order, or while a fused batch is in flight.  An item of at most 2048 states and at most 4096 arcs runs staged,
 *      offsets and arcs in LDS; a larger one reads them from memory.  The three n1 values describe the LAST launch of that
 *      kernel since the last wfst_shortest_path / wfst_shortest_path_batch call on ctx began — a batch, a lone call or an
 *      export; when an item is handed back, the lone call that then answers it may launch again —:
 *        n1_in_kernel    items the kernel answered (an item without states or start state included),
 *        n1_staged       those of them that ran with their arcs in LDS,
 *        n1_handed_back  items given to the kernel that came back with a non-zero status.
 *      nshortest > 1, unique = false (nbest_wave_kernel).  Offered: an item with a start state, at most 4096 states, at most
 *      8192 arcs, no negative arc weight, when nshortest <= 64 and WFST_NBEST_DEVICE is not 0.  The search tree of every item
 *      of the launch has room for T = min(16384, max(2048, 2 * nshortest * (max_n + 8))) entries, max_n = the most states of
 *      an offered item (WFST_NBEST_TREE overrides T in tests).  Dense inputs overflow T without help: the complete graph of 20
 *      states at nshortest = 32 creates several times the 2048 entries it is given.  The four nbest values describe the last
 *      wfst_shortest_path_batch call with nshortest > 1, unique = false:
 *        nbest_in_kernel      items the kernel answered (== wfst_stats.nbest_device_problems),
 *        nbest_tree_full      items that came back because the tree was full (or the distances did not settle),
 *        nbest_out_full       items that came back because the launch's 256 MB result area was full,
 *        nbest_tree_capacity  the T of the launch.
 *      All values are 0 when no launch was made.  Any pointer after ctx may be NULL.  KO: NULL ctx. ---- */
wfst_status wfst_ctx_get_small_path_stats(wfst_ctx* ctx, uint64_t* n1_in_kernel, uint64_t* n1_staged, uint64_t* n1_handed_back,
                                          uint64_t* nbest_in_kernel, uint64_t* nbest_tree_full, uint64_t* nbest_out_full,
                                          uint64_t* nbest_tree_capacity);

/* ---- which route answered the problems of the last wfst_compose / wfst_compose_shortest_path_batch[_begin/_end/_packed]
 *      call of ctx: the two kernels of compose.hip hand a problem from a fast route to a slower one that returns the same
 *      FST, so only these counters show which one ran.  They are tallied on the host from the status word every problem
 *      already reports; a call resets them when it begins.
 *      string_compose_sp_kernel takes a problem of the fused batch whose first operand is a string (linear, epsilon-free,
 *      one final state) of at most 2048 states, with filter Auto or Sequence, against a T without input epsilons
 *      (WFST_STRING_KERNEL=0: never).  Inside it: a level of ONE state whose arc block has at most 12 arcs, and lies at
 *      least 12 arcs before the end of T's arc array, is read through the scalar cache (on by default for batches of at most
 *      8; WFST_STRING_SCALAR=0/1); a lone match of a one-state level with a block of at most 64 arcs asks for the next
 *      level's first 64 rows early; blocks are read 64 arcs at a time, the string 64 labels at a time.  It hands back
 *      (ST_NOT_A_STRING_CASE) a problem with a level of more than 64 states or with as many composed states as its LDS slice
 *      holds: 2048, or for a batch of at least 16 without WFST_STRING_UNPACKED 512 / 1024 / 2048 = the least of them
 *      that is >= 2 * max_states + 64, max_states = the most states of a string of the batch.
 *      compose_wave_kernel stages a BFS level in LDS while it emits at most 64 arcs and redoes it through the arena when
 *      it does not; matches by ballot against a searched block of at most 64 arcs and by binary search beyond; takes the
 *      iterated side 64 items at a time (items = arcs + 1).  Its arena holds S states, A arcs and H hash slots:
 *      wfst_compose starts at S = 4 * max(min(n1, n2), 64) + 1024, A = 4 * S; the fused batch at S = 4 * max(max_states, 64)
 *      + 256, A = 2 * S; H = the power of two >= 2 * S + 128.  A level may hold hi + emitted + 64 <= H (hi = the states
 *      numbered before it).  An overflow relaunches the problem with 4 * S and 4 * A.  wfst_compose hands a level that
 *      adds more than 64 states (seen on the arena route only), or a relaunch beyond S = 16384, to the wide driver
 *      (WFST_COMPOSE_PATH=wave: never).  The fused path is redone as compose + shortest_path when a state of the path has
 *      no predecessor that is tight in the hop count (ST_TIE_ORDER).
 *        string_answered     problems the string kernel answered (== wfst_stats.string_problems),
 *        string_handed_back  problems it handed back to the wave kernel,
 *        wave_first          problems the wave kernel answered in their first launch on it,
 *        relaunch_states / relaunch_arcs / relaunch_hash / relaunch_path
 *                            launches that ended in that overflow (a problem relaunched twice counts twice),
 *        switched_wide       problems given to the wide driver by wfst_compose (either reason),
 *        two_step            problems of a fused batch redone as compose + shortest_path (that inner compose is not tallied),
 *        caps_states / caps_arcs / caps_hash   S, A and H of the last compose_wave_kernel launch (0: none was made).
 *      Any pointer after ctx may be NULL.  KO: NULL ctx. ---- */
wfst_status wfst_ctx_get_compose_path_stats(wfst_ctx* ctx, uint64_t* string_answered, uint64_t* string_handed_back,
                                            uint64_t* wave_first, uint64_t* relaunch_states, uint64_t* relaunch_arcs,
                                            uint64_t* relaunch_hash, uint64_t* relaunch_path, uint64_t* switched_wide,
                                            uint64_t* two_step, uint64_t* caps_states, uint64_t* caps_arcs, uint64_t* caps_hash);

/* ---- the chase runs of string_compose_sp_kernel in the last wfst_compose_shortest_path_batch[_begin/_end/_packed] call of
 *      ctx.  On its vector path (batches of more than 8 strings, or WFST_STRING_SCALAR=0) a level with ONE frontier state,
 *      a block of at most 64 arcs, exactly ONE arc that carries the string's label, a level behind it in the string and two
 *      free states in the problem's LDS slice is taken by a loop that only follows the matched arc to the next block; the
 *      distance, parent and arc weight of the level's one new state are filled in while that block's rows are on their
 *      way.  Every other level, and
 *      every level with WFST_STRING_RUN=0, is done one by one as before; the results are the same bit for bit, so only
 *      these counters show what ran.  Tallied on the host from two words every problem's result already carries, over the
 *      problems the string kernel answered; a call resets them when it begins.
 *        run_levels  levels taken inside runs,
 *        runs        runs of at least one level.
 *      Any pointer after ctx may be NULL.  KO: NULL ctx. ---- */
wfst_status wfst_ctx_get_string_run_stats(wfst_ctx* ctx, uint64_t* run_levels, uint64_t* runs);

/* ---- the pair levels of the same kernel in the same call.  The loop that takes the run levels also carries a frontier of
 *      one or two states (every block of at most 64 arcs) over a level whose matches, in (frontier state, arc position)
 *      order, are one or two with distinct destinations, where a level behind it in the string and the new states plus
 *      one fit the problem's LDS slice: match j makes state hi + j with its one way in, and the rows of the new states are
 *      asked for before they are settled.  A level of one state and one match is a run level and counted above, not here.
 *      WFST_STRING_PAIR=0 (and WFST_STRING_RUN=0) turns them off; same results bit for bit.  Tallied and reset like the run
 *      counters.
 *        pair_levels  levels carried that are not run levels,
 *        pair_splits  those of them with two matches.
 *      Either pointer after ctx may be NULL.  KO: NULL ctx. ---- */
wfst_status wfst_ctx_get_string_pair_counts(wfst_ctx* ctx, uint64_t* pair_levels, uint64_t* pair_splits);

/* ---- where the waves of the last string launch of ctx sat: string_compose_sp_kernel in a
 *      wfst_compose_shortest_path_batch[_begin/_end/_packed] call, string_sigma_sp_kernel in a
 *      wfst_compose_shortest_path_batch_with_matchers call with a matcher config.  One wave answers one string from its own
 *      slice of the workgroup's LDS; how many waves share a workgroup changes no result and no other counter, only which
 *      compute units work.  With cap = 64 KB / (16 * slice_states) = 8, 4 or 2: WFST_STRING_WPB=1|2|4|8 (other numbers: the
 *      next lower power of two; 0 and non-numbers are ignored) gives min(that, cap); WFST_STRING_UNPACKED gives 1 and the 2048-state slice, in either kernel; fewer
 *      than 16 strings give 1; while the last large-FST shortest-path solve that finished on the device in this process ran its
 *      levels in a resident launch, cap (such a launch needs nearly every compute unit whole); otherwise the least of 1, 2,
 *      4, 8 and cap that gives every workgroup a compute unit of the context (those of its mask) to itself.  Either call
 *      resets them when it begins.
 *        waves_per_workgroup  of that launch (0: the call made none),
 *        slice_states         composed states a wave's LDS slice holds: 512, 1024 or 2048,
 *        workgroups           of that launch,
 *        packed_for_resident  1: the resident launch decided, 0: not,
 *        forced               1: WFST_STRING_WPB or WFST_STRING_UNPACKED decided, 0: not.
 *      Any pointer after ctx may be NULL.  KO: NULL ctx. ---- */
wfst_status wfst_ctx_get_string_placement(wfst_ctx* ctx, uint64_t* waves_per_workgroup, uint64_t* slice_states, uint64_t* workgroups,
                                          uint64_t* packed_for_resident, uint64_t* forced);

/* ---- which route the levels of the last wfst_determinize / wfst_determinize_with_distance call of ctx took.  The result
 *      is built breadth-first level by level, and every route returns the same FST, so only these counters show which one
 *      ran.  They are tallied on the host from the control block the call already reads back (no launch, no read-back of
 *      their own); a call resets them when it begins.  After wfst_determinize_batch / wfst_determinize_with_distance_batch
 *      they are unspecified (an item handed to the single-FST path overwrites them).
 *      One workgroup (det_narrow_kernel) runs level after level inside one launch while a level has at most 256 states and
 *      at most 8192 raw candidates (WFST_DETERMINIZE_PATH=narrow: whatever their size), for at most 65536 levels per launch
 *      (WFST_DETERMINIZE_LEVEL_BUDGET=n, 0 < n < 65536, lowers that for tests); any other level runs as one device-wide launch
 *      per phase (WFST_DETERMINIZE_PATH=wide: every level), whose resolve rounds the host runs two at a time.  The arrays
 *      start with room for 1024 states, 4096 subset elements, 4096 arcs and 4096 candidates of one level.  A level of K raw
 *      candidates starts only when K <= candidates, hi + K <= states, elements + K <= element room and arcs + K <= arc room
 *      (hi = the states numbered before it, elements and arcs = those stored so far); otherwise nothing of it is written, the
 *      arrays short of hi + K + 1 states, elements + K, arcs + K or K candidates double until they hold them, the state
 *      table is re-hashed when the states grew, and the level starts again.
 *        levels            levels completed,
 *        wide_levels       those of them the device-wide launches completed (the others ran in the narrow kernel),
 *        narrow_launches   det_narrow_kernel launches,
 *        exit_wide_states / exit_wide_cands
 *                          launches that ended at a level of more than 256 states / of at most 256 states and more than 8192 raw
 *                          candidates,
 *        exit_budget       launches that ended after their budget of levels,
 *        exit_need         launches that ended at a level that needs more room,
 *        exit_done         launches that ended because no state was left (0 or 1),
 *        wide_need         device-wide levels whose check asked for more room,
 *        grow_states / grow_elts / grow_arcs / grow_cands
 *                          times that array was enlarged after the first allocation,
 *        rehashes          times the state table was re-hashed (== grow_states),
 *        cap_states / cap_elts / cap_arcs / cap_cands   the room at the end of the call,
 *        rounds_max        the most resolve rounds the host launched for one device-wide level (even; 0: no such level).
 *      All values are 0 for an input without states or start state.  Any pointer after ctx may be NULL.  KO: NULL ctx. ---- */
wfst_status wfst_ctx_get_determinize_stats(wfst_ctx* ctx, uint64_t* levels, uint64_t* wide_levels, uint64_t*
                                           narrow_launches, uint64_t* exit_wide_states, uint64_t* exit_wide_cands,
                                           uint64_t* exit_budget, uint64_t* exit_need, uint64_t* exit_done, uint64_t*
                                           wide_need, uint64_t* grow_states, uint64_t* grow_elts, uint64_t* grow_arcs,
                                           uint64_t* grow_cands, uint64_t* rehashes, uint64_t* cap_states, uint64_t*
                                           cap_elts, uint64_t* cap_arcs, uint64_t* cap_cands, uint64_t* rounds_max);

/* ---- which route the last wfst_minimize call of ctx took.  Every route returns the same FST, so only these counters show
 *      which one ran.  wfst_minimize resets them when it begins; they hold that call's
 *      values also when it ends KO.  They are tallied on the host from the control block the level loop already copies back
 *      once per host step (no launch, no read-back of their own).  After wfst_minimize_batch and wfst_optimize they are
 *      unspecified.
 *      The call peels the heights of a graph level by level, sinks first, at most twice: the cycle check on the untrimmed
 *      input when the stored word leaves ACYCLIC / CYCLIC unknown (check_*), then the refinement of the connected, sorted
 *      machine (no prefix; in the weighted branch the encoded machine with its superfinal state).  A level of at most 4096
 *      states runs in the one-workgroup narrow_kernel, which goes on level after level and leaves at an empty level or at
 *      one of more than 4096 states; any other level runs as device-wide launches, after which the host chooses again
 *      (WFST_MINIMIZE_PATH=narrow: one launch whatever the sizes; wide: every level device-wide).  A state of the refined
 *      machine with more than 64 arcs is refined by a wave, any other by a lane.
 *        levels            non-empty levels peeled,
 *        wide_levels       those of them the device-wide launches ran,
 *        narrow_launches   narrow_kernel launches,
 *        exit_wide         launches that ended at a level of more than 4096 states,
 *        exit_done         launches that ended at an empty level: every state was peeled, or a cycle holds the rest,
 *        branch            0 KO before any branch, or no states; 1 unweighted; 2 weighted; 3 weighted without a start
 *                          state; 4 nothing left after connect (either branch),
 *        wave_states       states a wave refined,
 *        unequal_compares  full signature compares that found a difference: two signatures shared a slot and the upper 32
 *                          bits of their hash (counted modulo 2^32).
 *      WFST_MINIMIZE_HASH_BITS=n (0 <= n <= 64, default 64; for tests) keeps only the low n bits of a signature's hash: with
 *      0 every state starts at slot 0 with tag 0 and is compared in full with every representative in front of it.  Anything
 *      else in the variable is KO.  The kernel of wfst_minimize_batch always keeps all 64 bits.
 *      All values are 0 for an input without states.  Any pointer after ctx may be NULL.  KO: NULL ctx. ---- */
wfst_status wfst_ctx_get_minimize_stats(wfst_ctx* ctx, uint64_t* check_levels, uint64_t* check_wide_levels,
                                        uint64_t* check_narrow_launches, uint64_t* check_exit_wide, uint64_t* check_exit_done,
                                        uint64_t* levels, uint64_t* wide_levels, uint64_t* narrow_launches, uint64_t* exit_wide,
                                        uint64_t* exit_done, uint64_t* branch, uint64_t* wave_states,
                                        uint64_t* unequal_compares);

/* ---- which route the last wfst_shortest_distance_with_config, wfst_reweight or wfst_push_weights call of ctx took.  Each
 *      of the three resets the counters when it begins, also when it refuses an argument; they hold that call's values also
 *      when it ends KO.  They are tallied on the host from launch geometry, the round loop's counter and values the call
 *      reads back anyway: no launch, no copy and no synchronisation of their own.  The structural passes are also entered
 *      from wfst_minimize, wfst_closure, wfst_concat and the list forms: after any call but the three above the counters
 *      are unspecified.
 *      A frontier search (the Vec length of a distance call; reachability, co-reachability on the reversed FST, in-degree
 *      peeling and the start-on-a-cycle search of the structural passes) over a graph of n states launches one
 *      bfs_round_kernel per round.  After round R = 1, 2, .. the host reads the size of frontier R when R is a multiple of
 *      16 or R = n + 1, and stops at the first read that finds it empty, or at R = n + 1 (the reversed FST has n + 1
 *      states).
 *        searches       frontier searches,
 *        rounds         bfs_round_kernel launches of all of them,
 *        reads          host reads of a frontier size,
 *        rounds_max     the most rounds of one search,
 *        bfs_blocks     blocks of the last bfs_round_kernel launch (16 lanes per frontier state, at most 8 blocks per
 *                       compute unit),
 *        arcs_blocks    ... of reweight_arcs_kernel (16 lanes per state, at most 32 per compute unit),
 *        total_blocks   ... of total_weight_kernel (a lane per state, at most 4 per compute unit); 0: the kernel did not run,
 *        structural     1: the four structural facts were searched (the start branch ran on a word that does not know
 *                       INITIAL_CYCLIC / INITIAL_ACYCLIC),
 *        start_branch   0 not taken, 1 the start state reweighted in place, 2 a new start state,
 *        removed        remove_total_weight: 0 not requested, 1 skipped because the total is one or zero, 2 applied.
 *      WFST_PUSH_MAX_BLOCKS=n (a positive integer; for tests) is an upper bound on those three grids, so that inputs of a
 *      few hundred states run the kernels' stride loops; read per call, unset or empty changes nothing, anything else is
 *      KO in the three calls above (before any other argument is looked at but reweight_type, potentials and delta).
 *      Any pointer after ctx may be NULL.  KO: NULL ctx. ---- */
wfst_status wfst_ctx_get_push_stats(wfst_ctx* ctx, uint64_t* searches, uint64_t* rounds, uint64_t* reads, uint64_t* rounds_max,
                                    uint64_t* bfs_blocks, uint64_t* arcs_blocks, uint64_t* total_blocks, uint64_t* structural,
                                    uint64_t* start_branch, uint64_t* removed);

/* wfst_compose_shortest_path_batch with the results as RECORDS (the layout of wfst_fst_pack_paths below) instead of handles:
 * out[i * (4 + 4 * max_arcs) ...] = path i, written straight from the kernel's result buffers — for hosts that read the
 * paths as a table (a decoder taking the output labels, the exchange between GPUs).  A path FST handle costs ~0.5 us of
 * host time to build and as much to destroy: beyond a few hundred acceptors per call that, not the GPU, is the batch's
 * time (bench.py `batch_sweep`).  KO if a path has more than max_arcs arcs. */
wfst_status wfst_compose_shortest_path_batch_packed(wfst_ctx* ctx, const wfst_fst* const* acceptors, size_t n, const wfst_fst* t,
                                                    const wfst_compose_config* compose_cfg,
                                                    const wfst_shortest_path_config* sp_cfg, uint32_t max_arcs, uint32_t* out,
                                                    uint64_t* composed_arcs);

/* Packs n linear path FSTs (outputs of the calls above) into fixed-size records for one all-gather:
 * record i = [n_arcs u32, final-weight bits u32, valid u32, 0] followed by max_arcs 16-byte arcs (zero padded),
 * i.e. (4 + 4*max_arcs) u32 words.  KO if a path has more than max_arcs arcs or is not linear. */
wfst_status wfst_fst_pack_paths(const wfst_fst* const* paths, size_t n, uint32_t max_arcs, uint32_t* out);

/* ---- several GPUs: one process or thread per GPU, acceptor i on GPU i mod G, T uploaded on every GPU, no
 * collective during compute; the finished results are all-gathered over RCCL / xGMI.  The reference is single-process
 * (no distributed code to mirror): these are the calls a Rust host adds next to compose / shortest_path (INTEGRATION.md,
 * "8 GPUs from Rust").  librccl is opened on first use; without it these calls return KO and everything else works. ---- */
typedef struct wfst_comm wfst_comm;
#define WFST_COMM_ID_BYTES 128
/* rank 0: a fresh rendezvous id (ncclGetUniqueId), to be handed to every rank by whatever channel the host has */
wfst_status wfst_comm_unique_id(uint8_t* id /* [WFST_COMM_ID_BYTES] */);
/* every rank, collectively (ncclCommInitRank): a communicator bound to ctx's GPU with a stream and pinned staging of its own */
wfst_status wfst_comm_create(wfst_ctx* ctx, const uint8_t* id, uint32_t rank, uint32_t world, wfst_comm** out);
/* The same communicator over a HOST transport: `fn` all-gathers `bytes` bytes per rank between host buffers (recv holds
 * world * bytes, rank-major) and returns 0 — an MPI_Allgather, a gloo group, a test harness.  No RCCL, no device staging,
 * the exchange completes inside _begin; staging sets, record layout and the ragged gather are the code of the RCCL path. */
typedef int (*wfst_allgather_fn)(void* user, const void* send, void* recv, size_t bytes);
wfst_status wfst_comm_create_host(uint32_t rank, uint32_t world, wfst_allgather_fn fn, void* user, wfst_comm** out);
wfst_status wfst_comm_info(const wfst_comm* comm, uint32_t* rank, uint32_t* world);
wfst_status wfst_comm_destroy(wfst_comm* comm);
/* All-gather of n linear path FSTs per rank as fixed-size records (layout of wfst_fst_pack_paths).  _begin packs into
 * pinned memory and queues H2D, ncclAllGather and D2H on the communicator's stream, then returns (the exchange overlaps
 * with whatever the caller does next: the next decoding step); _end waits and copies world * n records, rank-major, to out.
 * One exchange in flight per communicator. */
wfst_status wfst_gather_paths_begin(wfst_comm* comm, const wfst_fst* const* paths, size_t n, uint32_t max_arcs);
wfst_status wfst_gather_paths_end(wfst_comm* comm, uint32_t* out /* [world * n * (4 + 4 * max_arcs)] */);
/* _begin for records that exist already (the table wfst_compose_shortest_path_batch_packed filled): no handles, no packing */
wfst_status wfst_gather_records_begin(wfst_comm* comm, const uint32_t* records, size_t n, uint32_t max_arcs);
/* Orders the communicator's stream behind everything queued on ctx's stream so far: the next exchange then runs AFTER
 * that work (a step's relaxation sweeps need every compute unit; the all-gather kernel is better off beside the start of
 * the next step than in the middle of this one).  Optional; without it an exchange starts as soon as it is queued. */
wfst_status wfst_comm_order_after(wfst_comm* comm, wfst_ctx* ctx);
/* the same for `bytes` opaque bytes per rank */
wfst_status wfst_comm_allgather_begin(wfst_comm* comm, const void* send, size_t bytes);
wfst_status wfst_comm_allgather_end(wfst_comm* comm, void* recv /* [world * bytes] */);
/* ragged: every rank contributes `bytes` bytes (general FSTs in the OpenFST binary format: n-best trees, look-ahead
 * compositions); sizes[r] = bytes of rank r, *recv = one block holding the payloads back to back in rank order
 * (wfst_bytes_destroy), *total = their sum.  Two exchanges: the sizes, then the payloads padded to the largest. */
wfst_status wfst_comm_allgatherv(wfst_comm* comm, const void* send, size_t bytes, uint64_t* sizes /* [world] */, void** recv,
                                 size_t* total);

/* Tie order of shortest_path (nshortest = 1).  0 (default): the canonical rule — fewest arcs, then the smallest (source
 * state, arc position), the smallest final state; schedule-free, what every GPU path computes.  1: the REFERENCE's choice
 * where it is well defined cheaply, i.e. on ACYCLIC inputs (composed lattices): rustfst relaxes states in the topological
 * order of its depth-first visit (queues/auto_queue.rs:23-99 -> TopOrderQueue, top_sort.rs:12-61, dfs_visit.rs:97-187) and
 * keeps the FIRST arc, in (order of the source, arc position), that attains the final distance (shortest_path.rs:214-232),
 * and the first final state in that order.  The visit runs on the host (it is sequential by definition), distances and
 * the predecessor pass on the GPU.  On CYCLIC inputs (and inputs rustfst relaxes LIFO) its choice among tied optima is a
 * function of its whole relaxation history, which no rule reproduces: there, tie order 1 returns the path only when the
 * optimum is UNIQUE (wfst_stats.tied_choices == 0: no state of the path has a second optimal predecessor, one final state
 * attains the optimum) — then it is provably rustfst's path — and is KO ("ambiguous optimum") otherwise, so that a caller
 * that needs rustfst's structure falls back to rustfst (the convention for unsupported cases).  Tie order 0 never fails
 * and reports the same count in wfst_stats.tied_choices. */
wfst_status wfst_ctx_set_tie_order(wfst_ctx* ctx, int reference_order);

/* Share of the device a RESIDENT relaxation launch of this context may occupy (shortest_path on branching FSTs of <= 2M
 * states: sssp_mbox_resident_kernel keeps one 1024-thread workgroup on a compute unit of its own for every block of states,
 * for the whole wide phase of the solve — DESIGN.md §3.2 / §3.3).  0 (default) = the whole device: blocks of 4096 states, up to
 * 245 workgroups for a 1M-state FST — the fastest solve, and nothing else of any size fits beside it: a kernel that holds
 * more than a dozen compute units when the launch arrives makes it WAIT (a 512-string fused batch holds 64 of them for
 * ~0.3 ms).  1 = half the device: blocks of 8192 states where that brings the workgroup count to at most half the compute
 * units (1M states: 123), one launch per level where it does not — the solve alone is ~1.4 x slower (1M states: 0.32 vs
 * 0.22 ms of kernels) and runs BESIDE a batch of that size instead of behind it — or beside ANOTHER half-device query: the
 * device's resident lease has two units, a whole-device solve takes both, a half-device solve one, so two contexts set to 1
 * answer two queries at the same time (1M states: 4.8 k queries/s against 3.8 k one after the other; a third concurrent
 * query, or a whole-device one, takes one launch per level for that solve).  The request class decides: a server whose
 * shortest_path queries share the GPU with large fused batches, or that answers many queries at once, sets 1 on the contexts
 * that run the queries.
 * Same results either way (the keys are the fixed point whatever the block size).  The reference has no counterpart: its
 * algorithms run on one host thread (shortest_path.rs:173-239). */
wfst_status wfst_ctx_set_resident_share(wfst_ctx* ctx, uint32_t share);

/* ---- measurement hooks (bench.py / tests; not part of the reference surface) ---- */
/* the size rule of the five rational calls, the function each of them calls first, on bare counts and without a device (op: 0
 * union, 1 concat, 2 closure star, 3 closure plus; n operands in order).  States: the sum, + 1 for union and closure star.
 * Arcs by their upper bound: the sum, + n for union, + the states of every operand but the last for concat, + the states
 * (+ 1 for star) for closure.  KO "<op>: result too large: ..." beyond 2^31 - 2 states or 2^32 - 1 arcs. */
wfst_status wfst_rational_check_sizes(uint32_t op, const uint64_t* n_states, const uint64_t* n_arcs, size_t n);
typedef struct {
  /* relaxation kernel (sssp_relax_*): launches, total device time from HIP events on ctx's stream,
   * and the algorithmic units they processed */
  uint64_t relax_launches;
  double relax_ms;
  uint64_t relax_arcs;    /* arcs relaxed (sum over launches) */
  uint64_t relax_states;  /* frontier states expanded (sum over launches) */
  uint64_t sweeps;        /* relaxation sweeps of the last solve */
  /* compose */
  uint64_t compose_states; /* composed states created (pre-trim), last call */
  uint64_t compose_arcs;   /* composed arcs emitted (pre-trim), last call */
  uint64_t compose_retries; /* arena-overflow retries, cumulative */
  double compose_ms;       /* device time of the last compose / fused-batch kernel */
  uint64_t string_problems; /* problems of the last fused batch that took the string o T kernel (fst1 a linear,
                               epsilon-free acceptor, fst2 without input epsilons) */
  uint64_t relax_kernel;    /* kernel of the last relaxation: 0 sssp_relax_kernel (atomic sweeps), 1 sssp_mbox_kernel
                               (owner-computes mailbox launches: WIDE / COLLECT / NARROW, one level per launch), 2 the
                               same with the WIDE levels inside one sssp_mbox_resident_kernel launch, 3 atomic sweeps with
                               their dense levels as binned owner-computes passes (sssp_bin_expand / _apply_kernel) */
  uint64_t nbest_device_problems; /* inputs of the last wfst_shortest_path_batch (nshortest > 1) searched by the wave kernel
                                     (the others went through the host search) */
  uint64_t resident_aborts; /* resident relaxation launches that gave up waiting for their own workgroups (the solve was
                               then repeated with one launch per level; the context tries resident launches again after a
                               pause that doubles with every abort in a row), cumulative */
  uint64_t tied_choices;    /* last wfst_shortest_path (nshortest = 1): states of the returned path that had more than one optimal
                               predecessor, + 1 when several final states attain the optimum.  0 = the optimum is UNIQUE: the
                               path is what rustfst returns whatever its queue discipline.  > 0 = rustfst may return another path
                               of the same weight.  WFST_TIES_UNKNOWN when the call did not count (first query of an FST, FSTs
                               of < 2^18 arcs in the default tie order, tiny inputs, paths beyond 4096 arcs, acyclic inputs
                               under tie order 1 — exact there anyway) */
} wfst_stats;
#define WFST_TIES_UNKNOWN (~(uint64_t)0)
/* on = 1: every relaxation launch is bracketed by HIP events and followed by a synchronisation (per-launch trace below;
 * never on in timed runs).  on = 2: no per-launch events; the sweeps of a repeated shortest_path query (one pre-queued
 * batch) are timed as ONE chain between two events on the stream: relax_ms = that time, relax_launches = its sweeps
 * (0 when the query was not a single predicted batch).  on = 0: off. */
wfst_status wfst_ctx_set_profiling(wfst_ctx* ctx, int on);
wfst_status wfst_ctx_get_stats(wfst_ctx* ctx, wfst_stats* out);
wfst_status wfst_ctx_reset_stats(wfst_ctx* ctx);
/* per-launch trace of the last profiled relaxation (profiling on): launch k relaxed arcs[k] arcs leaving
 * states[k] frontier states in ms[k] milliseconds.  Copies min(cap, *n) entries; arrays may be NULL to query *n. */
wfst_status wfst_ctx_get_sweep_trace(wfst_ctx* ctx, double* ms, uint64_t* arcs, uint64_t* states, size_t cap, size_t* n);
/* ... and what ran launch k: 0 the atomic sweep, 7 a binned level (the same level as an owner-computes pass: expand +
 * apply kernels, chosen per level on the device), or the mailbox launches' mode (0 WIDE, 1 COLLECT, 2 NARROW). */
wfst_status wfst_ctx_get_sweep_modes(wfst_ctx* ctx, uint32_t* modes, size_t cap, size_t* n);

#ifdef __cplusplus
}
#endif
#endif /* WFST_AMD_H */
