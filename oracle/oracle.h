/*
 * oracle.h — C interface of the CPU ORACLE (test infrastructure, NOT product code).
 *
 * The oracle is a single-threaded C++17 restatement of rustfst 1.3.1's
 * algorithms::compose and algorithms::shortest_path for VectorFst<TropicalWeight>.
 * It exists only so that tests/, __graft_entry__.smoke() and bench.py's
 * cpu_baseline leg can check / time the reference algorithm on this box.
 * Nothing under rustfst_amd/ may include, link or dlopen it.
 *
 * PARITY PIN STATUS: pinned on the reference's in-repo known-answer tests
 * K1 (rustfst-python/tests/algorithms/test_compose.py:13-81), K2
 * (rustfst-python/tests/algorithms/test_shortest_path.py:5-51), K3 (doctest
 * compose/compose_static.rs:282-289) and the K4 loader fixtures
 * (rustfst-tests-data/sigma-matcher-2/{left,right}.fst), K7 project
 * (rustfst-python/tests/algorithms/test_project.py:5-97), K8 connect (test_connect.py:4-55),
 * K9 reverse (test_reverse.py:4-57), K10 tr_sort (test_tr_sort.py:4-97); the const-format loader on the
 * reference's own const files (rustfst-tests-data/fst_012, fst_014 hcl.fst.in: the stored
 * per-state epsilon counters must equal the recomputed ones).  The reference's large
 * OpenFST-generated goldens cannot be produced here (no rustc/cargo, no OpenFST,
 * no network), so parity AT SCALE is unpinned and rests on line-faithfulness
 * plus invariants (see tests/test_oracle.py).  UNPINNED restatements: the five
 * non-default compose filters (Null, AltSequence, Match, NoMatch; Trivial is pinned on the
 * reference's second K1 test, test_compose.py:84-154) and the n > 1 shortest-path search,
 * with and without `unique` — no reference output for them exists in the repository (the
 * determinization the `unique` branch rests on IS pinned: determinize_static.rs:210-270, K12); they are checked through invariants only (same best weight
 * under every epsilon filter, path membership, n = 1 agreement, the n lightest paths /
 * the n lightest DISTINCT strings against brute force).  Look-ahead composition (row A12:
 * LabelReachable, relabelling, LabelLookAheadMatcher, the PushLabels(PushWeights(
 * LookAhead(AltSequence))) filter stack as wired in rustfst-cli/src/cmds/compose.rs:77-181):
 * IntervalSet is pinned on the reference's unit tests (interval_set.rs:208-275), the rest
 * is UNPINNED (its goldens are OpenFST-generated) and checked through invariants: reachable
 * label sets against brute force, same multiset of weighted paths as plain composition.
 */
#ifndef WFST_ORACLE_H
#define WFST_ORACLE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  uint32_t ilabel, olabel;
  float weight;
  uint32_t nextstate;
} oracle_tr; /* == rustfst-ffi CTr (rustfst-ffi/src/tr.rs:8-21), == on-disk arc */

typedef struct oracle_fst oracle_fst; /* opaque VectorFst<TropicalWeight> */

/* equality mode of TropicalWeight `==` (semirings/semiring.rs:159-168) */
enum { ORACLE_EQ_REF_KDELTA = 0, ORACLE_EQ_EXACT = 1 };

/* status: 0 = OK, 1 = KO (message via oracle_last_error) */
const char* oracle_last_error(void);

/* ---- VectorFst surface (fst_impls/vector_fst/mutable_fst.rs) ---- */
oracle_fst* oracle_fst_new(void);
void oracle_fst_free(oracle_fst*);
uint32_t oracle_fst_add_state(oracle_fst*);
int oracle_fst_set_start(oracle_fst*, uint32_t s);
int oracle_fst_set_final(oracle_fst*, uint32_t s, float w);
int oracle_fst_add_tr(oracle_fst*, uint32_t s, uint32_t il, uint32_t ol, float w, uint32_t ns);
/* stable per-state sort by ilabel (olabel=0) or olabel (olabel=1): algorithms/tr_sort.rs:50-62 */
void oracle_fst_tr_sort(oracle_fst*, int by_olabel);

/* flat CSR interchange (same arrays the product C-ABI takes) */
oracle_fst* oracle_fst_from_flat(uint32_t n_states, int64_t start, const uint32_t* offsets,
                                 const oracle_tr* arcs, const float* finals, uint64_t props);
void oracle_fst_info(const oracle_fst*, uint32_t* n_states, uint64_t* n_arcs, int64_t* start,
                     uint64_t* props);
void oracle_fst_to_flat(const oracle_fst*, uint32_t* offsets, oracle_tr* arcs, float* finals);
/* per-state epsilon counters kept by VectorFstState (data_structure.rs:28-34) */
void oracle_fst_eps_counts(const oracle_fst*, uint32_t* nieps, uint32_t* noeps);

/* OpenFST binary vector/standard (parsers/bin_fst, vector_fst/serializable_fst.rs) */
oracle_fst* oracle_fst_load(const uint8_t* data, size_t len);
size_t oracle_fst_store(const oracle_fst*, uint8_t* out, size_t cap); /* returns needed size */
/* ConstFst::store, const_fst/serializable_fst.rs:41-89 (version 2, unaligned) */
size_t oracle_fst_store_const(const oracle_fst*, uint8_t* out, size_t cap);

/* ---- algorithms ---- */
/* compose_with_config(AutoFilter|SequenceFilter, connect): compose_static.rs:166-266 */
int oracle_compose(const oracle_fst* f1, const oracle_fst* f2, int connect, int eq_mode,
                   oracle_fst** out);
/* compose_with_config with an explicit ComposeFilterEnum value (compose_static.rs:19-33,166-266):
 * 0 Auto, 1 Null, 2 Trivial, 3 Sequence, 4 AltSequence, 5 Match, 6 NoMatch (default SortedMatchers) */
int oracle_compose_filter(const oracle_fst* f1, const oracle_fst* f2, int connect, int eq_mode, int filter,
                          oracle_fst** out);
/* look-ahead composition exactly as the reference wires it in rustfst-cli/src/cmds/compose.rs:77-181 and
 * tests_openfst/algorithms/compose.rs:118-254: MatcherFst::new_with_relabeling(fst1, &mut fst2, true),
 * LabelLookAheadMatcher (OUTPUT_LOOKAHEAD_MATCHER|LOOKAHEAD_WEIGHT|LOOKAHEAD_PREFIX|LOOKAHEAD_EPSILONS|
 * LOOKAHEAD_NON_EPSILON_PREFIX) on fst1, SortedMatcher on fst2, PushLabels(PushWeights(LookAhead(AltSequence))),
 * compute() without connect.  relabeled1/2 (may be NULL) receive the relabelled, re-sorted inputs.  UNPINNED. */
int oracle_compose_lookahead(const oracle_fst* f1, const oracle_fst* f2, oracle_fst** out, oracle_fst** relabeled1,
                             oracle_fst** relabeled2);
/* IntervalSet (compose/interval_set.rs): normalize n (begin,end) pairs in place, returns the new length (-1: empty
 * interval), *count = number of points; member() on a normalized set.  Pinned on interval_set.rs:208-275. */
int64_t oracle_interval_set_normalize(uint64_t* pairs, size_t n, uint64_t* count);
int oracle_interval_set_member(const uint64_t* pairs, size_t n, uint64_t value);
/* LabelReachable::compute_data(fst, reach_input) (compose/label_reachable.rs:135-273) */
typedef struct oracle_label_reachable oracle_label_reachable;
oracle_label_reachable* oracle_label_reachable_new(const oracle_fst* f, int reach_input);
void oracle_label_reachable_free(oracle_label_reachable*);
uint32_t oracle_label_reachable_final_label(const oracle_label_reachable*);
size_t oracle_label_reachable_num_labels(const oracle_label_reachable*);
void oracle_label_reachable_labels(const oracle_label_reachable*, uint32_t* labels, uint32_t* indices); /* by label */
size_t oracle_label_reachable_num_states(const oracle_label_reachable*);
size_t oracle_label_reachable_num_intervals(const oracle_label_reachable*, uint32_t state);
void oracle_label_reachable_intervals(const oracle_label_reachable*, uint32_t state, uint64_t* pairs);
/* project(): algorithms/projection.rs:65-95 (in place; project_output = 0: olabel := ilabel, 1: ilabel := olabel).
 * Pinned on rustfst-python/tests/algorithms/test_project.py:5-97. */
void oracle_fst_project(oracle_fst*, int project_output);
/* rm_epsilon() with the default config (connect, no thresholds): algorithms/rm_epsilon/rm_epsilon_static.rs:50-163,
 * rm_epsilon_state.rs:44-119 (in place).  Pinned on rustfst-python/tests/algorithms/test_rm_epsilon.py:4-54 (K11). */
int oracle_rm_epsilon(oracle_fst*);
/* connect(): connect.rs:51-66 */
int oracle_connect(oracle_fst*);
/* the word SccVisitor's depth-first visit leaves (visitors/scc_visitors.rs:29-37, 73-79, 97-102, 155-158): exactly one bit
 * of each of ACCESSIBLE, COACCESSIBLE, CYCLIC / ACYCLIC, INITIAL_CYCLIC / INITIAL_ACYCLIC; the stored word is not read.
 * Without a start state nothing is visited and all four positive bits come back. */
uint64_t oracle_fst_dfs_properties(const oracle_fst* f);
/* shortest_path_with_config(nshortest=1): shortest_path.rs:107-133,173-282.
 * Optional outputs (may be NULL): distance[n_states], total weight of the chosen path. */
int oracle_shortest_path(const oracle_fst* f, int eq_mode, oracle_fst** out, float* distance,
                         float* total_weight);
/* shortest_path_with_config(nshortest = n, unique = false): shortest_path.rs:107-170,284-518
 * (shortest_distance.rs:153-237 + reverse.rs:33-87 + n_shortest_path heap search + connect). */
int oracle_shortest_path_n(const oracle_fst* f, uint64_t nshortest, float delta, int eq_mode, oracle_fst** out);
/* the same with unique = true (shortest_path.rs:157-165: determinize_with_distance of the reversed FST first; acceptors only) */
/* determinize_fsa with the default common divisor (determinize_static.rs:41-53): acceptors only */
int oracle_determinize_fsa(const oracle_fst* f, float delta, int eq_mode, oracle_fst** out);
int oracle_shortest_path_n_unique(const oracle_fst* f, uint64_t nshortest, float delta, int eq_mode, oracle_fst** out);
/* shortest_distance_with_config(fst, reverse = false, delta): shortest_distance.rs:313-323.  Writes
 * min(cap, len) values (unreached = +inf beyond the reference's shorter vector); returns the reference length. */
uint64_t oracle_shortest_distance(const oracle_fst* f, float delta, float* distance, uint64_t cap);
/* reverse(): reverse.rs:33-87 (super-initial state 0, state i -> i+1) */
int oracle_reverse(const oracle_fst* f, oracle_fst** out);
/* name of the queue discipline AutoQueue picked for the last oracle_shortest_path call on
 * this thread (queues/auto_queue.rs:23-99): "state_order","top_order","lifo","top_order_scc","scc" */
const char* oracle_last_queue_kind(void);
/* after oracle_compose_lookahead on this thread: composed-state tuples created, and how many had a twin differing only by
 * a pushed weight one KDELTA step away (the pairs the reference's approximate PartialEq could merge) */
void oracle_last_lookahead_tuples(uint64_t* tuples, uint64_t* adjacent);
/* ... and the tuples themselves, in id order: five words per composed state (fst1 state, fst2 state, AltSequence state, bits
 * of the pushed weight, pushed label or NO_LABEL); writes at most `cap` tuples, returns how many there are */
size_t oracle_last_lookahead_tuple_list(uint32_t* out, size_t cap);

/* CANONICAL single shortest path: the deterministic tie rule the GPU engine implements
 * (DESIGN.md §Shortest path): (d,h)[t] = lexicographic min over paths of (left-fold f32 sum,
 * #arcs); final = min id among argmin d[s]+rho(s); parent[t] = min (s,pos) among arcs with
 * (d[s]+w, h[s]+1) == (d[t],h[t]).  Output numbered like shortest_path.rs:241-282.
 * n_tied_choices (may be NULL) = number of path positions where >1 candidate tied (0 => the
 * optimum found is the unique optimum along this path and must equal oracle_shortest_path). */
int oracle_shortest_path_canonical(const oracle_fst* f, oracle_fst** out, float* distance,
                                   uint32_t* hops, float* total_weight, uint32_t* n_tied_choices);

/* brute-force minimum path weight by exhaustive DFS up to max_len arcs (tiny FSTs only) */
float oracle_bruteforce_min_weight(const oracle_fst* f, uint32_t max_len);
/* is `path` (a linear FST as produced by shortest_path) a successful path of f? 1/0 */
int oracle_path_in_fst(const oracle_fst* path, const oracle_fst* f, float* weight_in_f);

/* batch: for each acceptor i: compose(a[i], t) -> shortest_path. n_threads >= 1 host threads,
 * one problem per thread at a time.  outs[i] receives the path FST (caller frees). Returns
 * wall seconds of the algorithm part in *seconds (may be NULL). */
int oracle_compose_shortest_path_batch(const oracle_fst* const* accs, size_t n,
                                       const oracle_fst* t, int n_threads, int eq_mode,
                                       oracle_fst** outs, uint64_t* composed_arcs_pre_trim,
                                       double* seconds);

#ifdef __cplusplus
}
#endif
#endif
