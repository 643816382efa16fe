// rational.hip — union, concat, closure and the list forms union_list / concat_list on the device: a NEW handle, the
// operands are left as they are.  Reference: rustfst/src/algorithms/union/union_static.rs:55-118,
// concat/concat_static.rs:53-109, closure/closure_static.rs:25-73; the list forms are the left folds of rustfst-python's
// union_list / concat_list (rustfst-python/rustfst/algorithms/union.py, concat.py).
//
// Every result is the states of m ITEMS laid one after the other, each item's nextstates shifted by its state base, plus
//   - per item a row-extension rule: every state with Some(final weight w) gets 0:0/w -> target appended last (concat: the
//     next item's start, the final weight goes; closure: the item's own start, the final weight stays);
//   - at most one state whose row ends with a prepared list of arcs (union: the root's 0:0/One arcs into the items' starts);
//   - at most one NEW state (union of an initial-cyclic first item, closure star) somewhere between the items.
// Two launches whatever m and the item sizes are (three with the scan):
//   state pass  one lane per input state: final weights, and either the output offset in closed form (union: input offset +
//               the item's arc base + the root's extra arcs for the states past the root) or the output degree (concat,
//               closure: + 1 per final state), which one exclusive scan turns into offsets;
//   copy pass   one lane per input arc: a 16-byte load, nextstate += state base, a 16-byte store at the row's new place
//               (the arc's state by binary search in the item's offsets: rows longer than a tile are split across tiles);
//               the prepared arc list is one more item of the same pass, the appended final arcs are its trailing state tiles.
// Tiles of TILE elements cover the concatenation of all items' states (arcs); tile_first[t] = the item holding the tile's
// first element, so a lane finds its item by a binary search between tile_first[t] and tile_first[t + 1]: one item may
// span many tiles, one tile may hold many tiny (or empty) items.
// Property words: on the host from the stored words (fst_props.h union_ / concat / closure); concat with a start-less second
// operand reduces the arc and final-weight facts of the per-mutation word on the device (rational_facts_kernel); union's
// compute_and_update_properties(INITIAL_ACYCLIC) is push.hip's structural_bits + props::merge_dfs.
#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

#include "common.h"
#include "fst_props.h"

namespace wfst {
namespace {

constexpr uint32_t TILE = 256;  // elements (states or arcs) per tile = threads per block (tests/test_rational_ops.py: TILE)
constexpr uint32_t NO_STATE = WFST_NO_STATE_ID;
constexpr uint32_t RULE_APPEND = 1u;  // a final state gets 0:0/final weight -> target appended last
constexpr uint32_t RULE_CLEAR = 2u;   // a final state loses its final weight
constexpr uint64_t MAX_STATES = 0x7FFFFFFEull;  // (fst_store.hip check_header: state ids fit in 31 bits)
constexpr uint64_t MAX_ARCS = 0xFFFFFFFFull;    // offsets are u32

struct Item {
  const uint32_t* off;  // nullptr: a prepared arc list (no states): copied as it is to the END of row `state_base`
  const wfst_tr* arcs;
  const float* fin;
  uint32_t n_states, n_arcs;
  uint32_t state_base;  // output id of state 0 = the shift of the nextstates
  uint32_t arc_base;    // closed form only: output position of arc 0
  uint32_t rule, target;
  uint32_t root, root_extra;  // closed form only: rows past `root` (a state of this item) start root_extra arcs later
};

struct Tables {
  const Item* items;
  const uint32_t* state_prefix;  // [m + 1] first global state index of item k
  const uint32_t* arc_prefix;    // [m + 1]
  const uint32_t* state_tile_first;  // [state tiles + 1]
  const uint32_t* arc_tile_first;    // [arc tiles + 1]
  uint32_t n_state_tiles, n_arc_tiles;
  uint32_t total_states, total_arcs;
};

struct NewState {
  uint32_t id;  // NO_STATE: none
  uint32_t deg, off;
  float fin;
};

// the largest k in [lo, hi] with a[k] <= v (a ascending, a[lo] <= v)
__device__ __forceinline__ uint32_t last_not_above(const uint32_t* __restrict__ a, uint32_t lo, uint32_t hi, uint32_t v) {
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo + 1) / 2;
    if (a[mid] <= v)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(TILE) void rational_state_kernel(Tables tb, NewState ns, int scan, uint32_t n_out, uint32_t e_out,
                                                              uint32_t* __restrict__ off_or_deg, float* __restrict__ fin_out) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (ns.id != NO_STATE) {
      off_or_deg[ns.id] = scan ? ns.deg : ns.off;
      fin_out[ns.id] = ns.fin;
    }
    off_or_deg[n_out] = scan ? 0u : e_out;
  }
  for (uint32_t t = blockIdx.x; t < tb.n_state_tiles; t += gridDim.x) {
    const uint64_t g64 = (uint64_t)t * TILE + threadIdx.x;
    if (g64 >= tb.total_states) continue;
    const uint32_t g = (uint32_t)g64;
    const uint32_t k = last_not_above(tb.state_prefix, tb.state_tile_first[t], tb.state_tile_first[t + 1], g);
    const Item it = tb.items[k];
    const uint32_t s = g - tb.state_prefix[k];
    const uint32_t o = it.state_base + s;
    const float f = it.fin[s];
    const bool is_final = f != INF;
    fin_out[o] = (is_final && (it.rule & RULE_CLEAR)) ? INF : f;
    const uint32_t b = it.off[s];
    if (scan)
      off_or_deg[o] = it.off[s + 1] - b + ((is_final && (it.rule & RULE_APPEND)) ? 1u : 0u) + (s == it.root ? it.root_extra : 0u);
    else
      off_or_deg[o] = b + it.arc_base + ((it.root != NO_STATE && s > it.root) ? it.root_extra : 0u);
  }
}

// blocks 0 .. n_arc_tiles - 1 (as tiles) move arcs; the tiles after them are state tiles that write the appended final arcs
__global__ __launch_bounds__(TILE) void rational_copy_kernel(Tables tb, uint32_t n_append_tiles, const uint32_t* __restrict__ off_out,
                                                             wfst_tr* __restrict__ arcs_out) {
  uint4* __restrict__ dst = reinterpret_cast<uint4*>(arcs_out);
  const uint32_t tiles = tb.n_arc_tiles + n_append_tiles;
  for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    if (t < tb.n_arc_tiles) {
      const uint64_t g64 = (uint64_t)t * TILE + threadIdx.x;
      if (g64 >= tb.total_arcs) continue;
      const uint32_t g = (uint32_t)g64;
      const uint32_t k = last_not_above(tb.arc_prefix, tb.arc_tile_first[t], tb.arc_tile_first[t + 1], g);
      const Item it = tb.items[k];
      const uint32_t j = g - tb.arc_prefix[k];
      uint4 a = reinterpret_cast<const uint4*>(it.arcs)[j];
      if (it.off == nullptr) {  // the prepared list: the last n_arcs places of its row
        dst[off_out[it.state_base + 1] - it.n_arcs + j] = a;
        continue;
      }
      const uint32_t s = last_not_above(it.off, 0u, it.n_states - 1u, j);
      a.w += it.state_base;
      dst[off_out[it.state_base + s] + (j - it.off[s])] = a;
    } else {
      const uint32_t ts = t - tb.n_arc_tiles;
      const uint64_t g64 = (uint64_t)ts * TILE + threadIdx.x;
      if (g64 >= tb.total_states) continue;
      const uint32_t g = (uint32_t)g64;
      const uint32_t k = last_not_above(tb.state_prefix, tb.state_tile_first[ts], tb.state_tile_first[ts + 1], g);
      const Item it = tb.items[k];
      if (!(it.rule & RULE_APPEND)) continue;
      const uint32_t s = g - tb.state_prefix[k];
      const float f = it.fin[s];
      if (f == INF) continue;
      dst[off_out[it.state_base + s + 1] - 1u] = make_uint4(0u, 0u, __float_as_uint(f), it.target);
    }
  }
}

// facts[0] |= arc_facts of every arc (with its predecessor in the row); facts[1] |= FINAL_ANY for a final weight,
// FINAL_WEIGHTED for one that is neither One nor Zero (concat with a start-less second operand: the per-mutation word)
constexpr uint32_t FINAL_ANY = 1u, FINAL_WEIGHTED = 2u;
__global__ __launch_bounds__(TILE) void rational_facts_kernel(const uint32_t* __restrict__ off, const wfst_tr* __restrict__ arcs,
                                                              const float* __restrict__ fin, uint32_t n, int with_arcs,
                                                              uint32_t* __restrict__ facts) {
  uint32_t af = 0, ff = 0;
  for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += gridDim.x * blockDim.x) {
    const float f = fin[s];
    if (f != INF) ff |= FINAL_ANY | (weighted(f) ? FINAL_WEIGHTED : 0u);
    if (!with_arcs) continue;
    const uint32_t b = off[s], e = off[s + 1];
    wfst_tr prev{};
    for (uint32_t i = b; i < e; ++i) {
      const wfst_tr a = arcs[i];
      af |= props::arc_facts(a, i > b ? &prev : nullptr, s);
      prev = a;
    }
  }
  if (af) atomicOr(&facts[0], af);
  if (ff) atomicOr(&facts[1], ff);
}

// ---------------------------------------------------------------- the host side
struct Operand {  // one real item of a plan
  const wfst_fst* f;
  uint32_t state_base;
  uint64_t arc_base = 0;  // closed form
  uint32_t rule = 0, target = 0;
  uint32_t root = NO_STATE, root_extra = 0;
};
struct Plan {
  std::vector<Operand> items;
  bool scan = false;            // some item appends final arcs: degrees + scan; otherwise the offsets are closed-form
  NewState ns{NO_STATE, 0, 0, INF};
  std::vector<wfst_tr> extra;   // the prepared arc list and the output state whose row it ends
  uint32_t extra_state = NO_STATE;
  uint64_t n_out = 0, e_closed = 0;  // states of the result; its arcs when !scan
  int64_t start = -1;
  uint64_t props = 0;
};

void check_operand(wfst_ctx* ctx, const wfst_fst* f, const char* op, const std::string& which) {
  if (f->device != ctx->device) throw Error(std::string(op) + ": " + which + " lives on another device");
  if (f->ctx != ctx) throw Error(std::string(op) + ": " + which + " belongs to another context");
}
// the first thing each of the five calls does: rational_check_sizes on its operands' counts
void check_sizes_of(uint32_t op, const wfst_fst* const* fsts, size_t n) {
  std::vector<uint64_t> ns(n), na(n);
  for (size_t i = 0; i < n; ++i) ns[i] = fsts[i]->n_states, na[i] = fsts[i]->n_arcs;
  rational_check_sizes(op, ns.data(), na.data(), n);
}

// blocks of a launch: at most 16 per compute unit, the rest of the tiles by striding.  WFST_RATIONAL_MAX_BLOCKS (tests)
// lowers the cap so that small inputs stride too.
uint32_t grid_cap(const wfst_ctx* ctx) {
  uint32_t cap = (uint32_t)ctx->n_cus * 16;
  if (const char* e = std::getenv("WFST_RATIONAL_MAX_BLOCKS")) {
    const long v = std::strtol(e, nullptr, 10);
    if (v >= 1 && (uint64_t)v < cap) cap = (uint32_t)v;
  }
  return cap;
}

wfst_fst* copy_with_props(wfst_ctx* ctx, const wfst_fst* f, int64_t start, uint64_t p) {
  if (f->n_states == 0) {
    HostCsr h;
    h.offsets.push_back(0);
    return make_host_fst(ctx, 0, start, p & props::ALL, std::move(h));
  }
  ensure_device(const_cast<wfst_fst*>(f));
  return adopt_device(ctx, f->n_states, f->n_arcs, start, p & props::ALL, f->dev.offsets, f->dev.arcs, f->dev.finals);
}

// tile_first[t] = the item that holds global element t * TILE (the largest k < m with prefix[k] <= t * TILE); one entry more
// closes the last tile's range
void tile_map(const std::vector<uint32_t>& prefix, uint32_t* out, uint32_t tiles) {
  const uint32_t m = (uint32_t)prefix.size() - 1;
  uint32_t k = 0;
  for (uint32_t t = 0; t < tiles; ++t) {
    const uint64_t first = (uint64_t)t * TILE;
    while (k + 1 < m && prefix[k + 1] <= first) ++k;
    out[t] = k;
  }
  out[tiles] = m ? m - 1 : 0;
}

wfst_fst* run_plan(wfst_ctx* ctx, const Plan& pl) {
  hipStream_t st = ctx->stream;
  DevicePool& pool = *ctx->pool;
  if (pl.n_out == 0) {
    HostCsr h;
    h.offsets.push_back(0);
    return make_host_fst(ctx, 0, -1, pl.props & props::ALL, std::move(h));
  }
  const uint32_t n_out = (uint32_t)pl.n_out;
  for (const Operand& o : pl.items) ensure_device(const_cast<wfst_fst*>(o.f));

  // ---- the tables: items (the prepared list last), prefixes, tile maps, the prepared arcs: one staging block, one copy
  const uint32_t m_real = (uint32_t)pl.items.size();
  const uint32_t m = m_real + (pl.extra.empty() ? 0u : 1u);
  std::vector<uint32_t> sp(m + 1, 0), ap(m + 1, 0);
  for (uint32_t k = 0; k < m; ++k) {
    const bool real = k < m_real;
    sp[k + 1] = sp[k] + (real ? pl.items[k].f->n_states : 0u);
    ap[k + 1] = ap[k] + (uint32_t)(real ? pl.items[k].f->n_arcs : pl.extra.size());
  }
  const uint32_t s_tiles = (sp[m] + TILE - 1) / TILE, a_tiles = (uint32_t)(((uint64_t)ap[m] + TILE - 1) / TILE);
  auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
  const size_t o_items = 0, o_sp = up16(o_items + (size_t)m * sizeof(Item)), o_ap = up16(o_sp + (m + 1) * 4ull),
               o_st = up16(o_ap + (m + 1) * 4ull), o_at = up16(o_st + (s_tiles + 1) * 4ull), o_ex = up16(o_at + (a_tiles + 1) * 4ull),
               bytes = o_ex + pl.extra.size() * sizeof(wfst_tr);
  DBuf<uint8_t> d_tab(pool, bytes);
  uint8_t* h_tab = (uint8_t*)ctx->pinned_big.get(bytes);
  Item* items = (Item*)(h_tab + o_items);
  for (uint32_t k = 0; k < m_real; ++k) {
    const Operand& o = pl.items[k];
    items[k] = Item{o.f->dev.offsets, o.f->dev.arcs, o.f->dev.finals, o.f->n_states, (uint32_t)o.f->n_arcs, o.state_base,
                    (uint32_t)o.arc_base, o.rule, o.target, o.root, o.root_extra};
  }
  if (m > m_real)
    items[m_real] = Item{nullptr, (const wfst_tr*)(d_tab.p + o_ex), nullptr, 0u, (uint32_t)pl.extra.size(), pl.extra_state, 0u, 0u, 0u,
                         NO_STATE, 0u};
  std::memcpy(h_tab + o_sp, sp.data(), (m + 1) * 4ull);
  std::memcpy(h_tab + o_ap, ap.data(), (m + 1) * 4ull);
  tile_map(sp, (uint32_t*)(h_tab + o_st), s_tiles);
  tile_map(ap, (uint32_t*)(h_tab + o_at), a_tiles);
  if (!pl.extra.empty()) std::memcpy(h_tab + o_ex, pl.extra.data(), pl.extra.size() * sizeof(wfst_tr));
  HIP_CHECK(hipMemcpyAsync(d_tab.p, h_tab, bytes, hipMemcpyHostToDevice, st));
  Tables tb{(const Item*)(d_tab.p + o_items), (const uint32_t*)(d_tab.p + o_sp), (const uint32_t*)(d_tab.p + o_ap),
            (const uint32_t*)(d_tab.p + o_st), (const uint32_t*)(d_tab.p + o_at), s_tiles, a_tiles, sp[m], ap[m]};

  // ---- state pass (+ scan)
  const uint32_t max_blocks = grid_cap(ctx);
  DBuf<uint32_t> off_out(pool, (size_t)n_out + 1), deg(pool, pl.scan ? (size_t)n_out + 1 : 1);
  DBuf<float> fin_out(pool, n_out);
  rational_state_kernel<<<std::max(1u, std::min(s_tiles, max_blocks)), TILE, 0, st>>>(
      tb, pl.ns, pl.scan ? 1 : 0, n_out, (uint32_t)pl.e_closed, pl.scan ? deg.p : off_out.p, fin_out.p);
  HIP_CHECK(hipGetLastError());
  DBuf<uint8_t> scan_tmp;
  uint64_t e_out = pl.e_closed;
  if (pl.scan) {
    scan_tmp = exclusive_scan_u32(ctx, deg.p, off_out.p, (size_t)n_out + 1);
    e_out = read_u32(ctx, off_out.p + n_out);
  }
  // ---- copy pass
  DBuf<wfst_tr> arcs_out(pool, e_out);
  const uint32_t c_tiles = a_tiles + (pl.scan ? s_tiles : 0u);
  if (c_tiles) {
    rational_copy_kernel<<<std::min(c_tiles, max_blocks), TILE, 0, st>>>(tb, pl.scan ? s_tiles : 0u, off_out.p, arcs_out.p);
    HIP_CHECK(hipGetLastError());
  }
  Handle out(adopt_device(ctx, n_out, e_out, pl.start, pl.props & props::ALL, off_out.p, arcs_out.p, fin_out.p));
  HIP_CHECK(hipStreamSynchronize(st));  // the staging block and the tables are free again
  return out.release();
}

// compute_and_update_properties(INITIAL_ACYCLIC) (fst_traits/mutable_fst.rs:435-441): the stored pair if the word knows it,
// else the DFS's four pairs replace the word's
uint64_t word_with_initial_pair(wfst_ctx* ctx, const wfst_fst* f) {
  uint64_t p = f->props & props::ALL;
  if (!props::knows(p, props::INITIAL_CYCLIC)) p = props::merge_dfs(p, structural_bits(ctx, f));
  return p;
}

// union of its[0] (which has a start state, word p0 after compute_and_update_properties) with its[1..], all with a start
// state: the closed form of the fold (union_static.rs:72-116 applied from the left)
wfst_fst* union_closed(wfst_ctx* ctx, const std::vector<const wfst_fst*>& its, uint64_t p0) {
  const bool ia = (p0 & props::INITIAL_ACYCLIC) != 0;
  const uint32_t m = (uint32_t)its.size();
  const uint32_t R = m - 1;
  Plan pl;
  uint64_t sb = 0, ab = 0, p = p0;
  std::vector<uint64_t> bases(m);
  for (uint32_t k = 0; k < m; ++k) {
    if (!ia && k == 2) sb += 1, ab += R + 1;  // the new start state sits behind item 1
    if (ia && k == 1) ab += R;               // the root's row is R arcs longer
    bases[k] = sb;
    Operand o{its[k], (uint32_t)std::min<uint64_t>(sb, NO_STATE), ab};
    if (ia && k == 0) o.root = (uint32_t)its[0]->start, o.root_extra = R;
    pl.items.push_back(o);
    sb += its[k]->n_states;
    ab += its[k]->n_arcs;
    if (k) p = props::union_(p, its[k]->props & props::ALL);
  }
  if (!ia && m == 2) sb += 1, ab += R + 1;
  pl.n_out = sb;
  pl.e_closed = ab;
  if (!ia) {  // (:103-111) the new start state: 0:0/One -> start1, then the arcs into the other starts
    const uint64_t id = bases[1] + its[1]->n_states;
    uint64_t e01 = its[0]->n_arcs + its[1]->n_arcs;
    pl.ns = NewState{(uint32_t)id, R + 1, (uint32_t)e01, INF};
    pl.extra.push_back(wfst_tr{0u, 0u, 0.0f, (uint32_t)its[0]->start});
    pl.extra_state = (uint32_t)id;
    pl.start = (int64_t)id;
  } else {  // (:95-101) the start's row grows
    pl.extra_state = (uint32_t)its[0]->start;
    pl.start = its[0]->start;
  }
  for (uint32_t k = 1; k < m; ++k) pl.extra.push_back(wfst_tr{0u, 0u, 0.0f, (uint32_t)(bases[k] + (uint64_t)its[k]->start)});
  pl.props = p;
  return run_plan(ctx, pl);
}

// concat of items that all have a start state: the closed form of the fold (concat_static.rs:65-106 applied from the left)
wfst_fst* concat_closed(wfst_ctx* ctx, const std::vector<const wfst_fst*>& its) {
  const uint32_t m = (uint32_t)its.size();
  Plan pl;
  pl.scan = true;
  uint64_t sb = 0, p = its[0]->props & props::ALL;
  std::vector<uint64_t> bases(m + 1);
  for (uint32_t k = 0; k < m; ++k) {
    bases[k] = sb;
    sb += its[k]->n_states;
    if (k) p = props::concat(p, its[k]->props & props::ALL);
  }
  pl.n_out = sb;
  for (uint32_t k = 0; k < m; ++k) {
    Operand o{its[k], (uint32_t)bases[k]};
    if (k + 1 < m) o.rule = RULE_APPEND | RULE_CLEAR, o.target = (uint32_t)(bases[k + 1] + (uint64_t)its[k + 1]->start);
    pl.items.push_back(o);
  }
  pl.start = its[0]->start;
  pl.props = p;
  return run_plan(ctx, pl);
}

}  // namespace

wfst_fst* union_fst(wfst_ctx* ctx, const wfst_fst* a, const wfst_fst* b) {
  check_operand(ctx, a, "union", "the first operand");
  check_operand(ctx, b, "union", "the second operand");
  const wfst_fst* const both[2] = {a, b};
  check_sizes_of(0, both, 2);
  const uint64_t p1 = word_with_initial_pair(ctx, a);  // (union_static.rs:61-64) first, whatever follows
  if (b->start < 0) return copy_with_props(ctx, a, a->start, p1);  // (:68-70)
  if (a->start < 0) {  // (:87-92) b's states behind a's, the start WITHOUT the offset, b's word under copy_properties()
    Plan pl;
    pl.items.push_back(Operand{a, 0u, 0});
    pl.items.push_back(Operand{b, a->n_states, a->n_arcs});
    pl.n_out = (uint64_t)a->n_states + b->n_states;
    pl.e_closed = a->n_arcs + b->n_arcs;
    pl.start = b->start;
    pl.props = b->props;
    return run_plan(ctx, pl);
  }
  return union_closed(ctx, {a, b}, p1);
}

wfst_fst* concat_fst(wfst_ctx* ctx, const wfst_fst* a, const wfst_fst* b) {
  check_operand(ctx, a, "concat", "the first operand");
  check_operand(ctx, b, "concat", "the second operand");
  const wfst_fst* const both[2] = {a, b};
  check_sizes_of(1, both, 2);
  if (a->start < 0) return copy_with_props(ctx, a, a->start, a->props);  // (concat_static.rs:62-64)
  if (b->start >= 0) return concat_closed(ctx, {a, b});
  // b without a start state (:81-106): its states are appended, a's final weights go, no arc is added, and the word is what
  // the mutations leave: add_state / set_final / add_tr per state of b, then set_final(.., None) per final state of a.
  // Every one of them is a sticky set / clear decided by one fact, followed by a mask that keeps what the others set
  // (fst_props.h add_trs_by_facts), so the fold over b equals one application with the union of the facts; the facts are
  // reduced on the device.
  ensure_device(const_cast<wfst_fst*>(a));
  ensure_device(const_cast<wfst_fst*>(b));
  DBuf<uint32_t> d_facts(*ctx->pool, 4);
  HIP_CHECK(hipMemsetAsync(d_facts.p, 0, 4 * sizeof(uint32_t), ctx->stream));
  auto facts_of = [&](const wfst_fst* f, int with_arcs, uint32_t* out) {
    if (!f->n_states) return;
    const uint32_t blocks = std::min<uint32_t>((f->n_states + TILE - 1) / TILE, grid_cap(ctx));
    rational_facts_kernel<<<blocks, TILE, 0, ctx->stream>>>(f->dev.offsets, f->dev.arcs, f->dev.finals, f->n_states, with_arcs, out);
    HIP_CHECK(hipGetLastError());
  };
  facts_of(b, 1, d_facts.p);
  facts_of(a, 0, d_facts.p + 2);
  uint32_t h[4] = {0, 0, 0, 0};
  HIP_CHECK(hipMemcpyAsync(h, d_facts.p, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  const float plain = 0.0f, heavy = 1.0f;  // stand-ins: set_final only asks whether a weight is weighted
  uint64_t p = a->props & props::ALL;
  if (b->n_states) p = props::add_state(p);
  if (h[1] & FINAL_ANY) p = props::set_final(p, nullptr, (h[1] & FINAL_WEIGHTED) ? &heavy : &plain);
  if (b->n_arcs) p = props::add_trs_by_facts(p, h[0]);
  if (h[3] & FINAL_ANY) p = props::set_final(p, (h[3] & FINAL_WEIGHTED) ? &heavy : &plain, nullptr);
  Plan pl;
  pl.items.push_back(Operand{a, 0u, 0, RULE_CLEAR});
  pl.items.push_back(Operand{b, a->n_states, a->n_arcs});
  pl.n_out = (uint64_t)a->n_states + b->n_states;
  pl.e_closed = a->n_arcs + b->n_arcs;
  pl.start = a->start;
  pl.props = p;
  return run_plan(ctx, pl);
}

wfst_fst* closure_fst(wfst_ctx* ctx, const wfst_fst* f, bool star) {
  check_operand(ctx, f, "closure", "the operand");
  check_sizes_of(star ? 2 : 3, &f, 1);
  const bool has_start = f->start >= 0;
  Plan pl;
  pl.scan = has_start;
  pl.items.push_back(Operand{f, 0u, 0, has_start ? RULE_APPEND : 0u, has_start ? (uint32_t)f->start : 0u});  // (closure_static.rs:31-48)
  pl.n_out = f->n_states;
  pl.e_closed = f->n_arcs;
  pl.start = f->start;
  if (star) {  // (:50-67) a new start state, final with One, one arc into the old start if there was one
    pl.ns = NewState{f->n_states, has_start ? 1u : 0u, (uint32_t)f->n_arcs, 0.0f};
    if (has_start) {
      pl.extra.push_back(wfst_tr{0u, 0u, 0.0f, (uint32_t)f->start});
      pl.extra_state = f->n_states;
    }
    pl.start = f->n_states;
    pl.n_out += 1;
  }
  pl.props = props::closure(f->props & props::ALL);
  return run_plan(ctx, pl);
}

namespace {
void check_list(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, const char* op, uint32_t size_op) {
  for (size_t i = 0; i < n; ++i) check_operand(ctx, fsts[i], op, "item " + std::to_string(i));
  check_sizes_of(size_op, fsts, n);
}
}  // namespace

wfst_fst* union_list_fst(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n) {
  check_list(ctx, fsts, n, "union_list", 0);
  if (n == 1) return copy_with_props(ctx, fsts[0], fsts[0]->start, fsts[0]->props);
  if (fsts[0]->start < 0) {  // degenerate: the literal fold
    Handle acc(union_fst(ctx, fsts[0], fsts[1]));
    for (size_t i = 2; i < n; ++i) acc.reset(union_fst(ctx, acc.get(), fsts[i]));
    return acc.release();
  }
  const uint64_t p0 = word_with_initial_pair(ctx, fsts[0]);
  std::vector<const wfst_fst*> its{fsts[0]};
  for (size_t i = 1; i < n; ++i)
    if (fsts[i]->start >= 0) its.push_back(fsts[i]);  // an item without a start state adds nothing (union_static.rs:68-70)
  if (its.size() == 1) return copy_with_props(ctx, fsts[0], fsts[0]->start, p0);
  return union_closed(ctx, its, p0);
}

wfst_fst* concat_list_fst(wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n) {
  check_list(ctx, fsts, n, "concat_list", 1);
  if (n == 1) return copy_with_props(ctx, fsts[0], fsts[0]->start, fsts[0]->props);
  bool all_start = true;
  for (size_t i = 0; i < n; ++i) all_start = all_start && fsts[i]->start >= 0;
  if (!all_start) {  // degenerate: the literal fold
    Handle acc(concat_fst(ctx, fsts[0], fsts[1]));
    for (size_t i = 2; i < n; ++i) acc.reset(concat_fst(ctx, acc.get(), fsts[i]));
    return acc.release();
  }
  return concat_closed(ctx, std::vector<const wfst_fst*>(fsts, fsts + n));
}

// The one size rule of the five calls.  States: the operands' sum, + 1 for union (the new start state of an initial-cyclic
// first operand) and closure star.  Arcs, by their upper bound: the operands' sum, + n for union (n - 1 arcs into the other
// starts and the new state's arc into the first), + the states of every operand but the last for concat (one appended arc
// per final state), + the operand's states (+ 1 for star) for closure.  State ids stay below 2^31 - 1, offsets are u32.
void rational_check_sizes(uint32_t op, const uint64_t* n_states, const uint64_t* n_arcs, size_t n) {
  static const char* const names[4] = {"union", "concat", "closure", "closure"};
  if (op > 3) throw Error("unknown operation " + std::to_string(op));
  if (n && (!n_states || !n_arcs)) throw Error("null pointer");
  uint64_t ns = 0, na = 0;
  for (size_t i = 0; i < n; ++i) {
    ns += n_states[i];
    na += n_arcs[i] + (op == 0 ? 1 : (op == 1 && i + 1 == n) ? 0 : n_states[i]);
  }
  if (op == 0 || op == 2) ns += 1, na += (op == 2 ? 1 : 0);
  auto too_large = [&](const char* what, uint64_t v, uint64_t limit) {
    throw Error(std::string(names[op]) + ": result too large: up to " + std::to_string(v) + " " + what + ", the limit is " +
                std::to_string(limit));
  };
  if (ns > MAX_STATES) too_large("states", ns, MAX_STATES);
  if (na > MAX_ARCS) too_large("arcs", na, MAX_ARCS);
}

}  // namespace wfst
