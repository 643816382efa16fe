// batch_driver.h — the host side of the one-workgroup-per-item batch operations (determinize_batch, minimize_batch,
// rm_epsilon_batch; their kernels share wg_ops.h): one slab per launch with the control blocks at its head, launches
// until no item asks for a larger slice, then every result adopted at once.  The op says what an item's slice holds, how
// its kernel is launched and what a returned control block means; everything else is here.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "common.h"
#include "slab.h"

namespace wfst {
namespace {

// minimize_batch and rm_epsilon_batch refuse a handle of another device or context before anything else
void check_items_owned(const wfst_ctx* ctx, const wfst_fst* const* fsts, size_t n, const char* op) {
  for (size_t i = 0; i < n; ++i) {
    const std::string at = "item " + std::to_string(i) + ": " + op;
    if (fsts[i]->device != ctx->device) throw Error(at + ": the FST lives on another device");
    if (fsts[i]->ctx != ctx) throw Error(at + ": the FST belongs to another context");
  }
}

// WFST_*_BATCH_ARENA=min (tests): the first launch's slices as small as the kernel allows, so that every item grows
bool arena_min_knob(const char* var) {
  const char* e = std::getenv(var);
  if (!e || !*e) return false;
  if (!std::strcmp(e, "min")) return true;
  throw Error(std::string(var) + ": expected min, not '" + e + "'");
}

constexpr uint32_t BATCH_MAX_LAUNCHES = 64;  // of an op whose items grow: every launch at least doubles what was short

// what the op makes of one returned control block: it has recorded the item's result (FINISHED), leaves the item to the
// single-FST path (SINGLE), or has enlarged the item's capacities for another launch (GREW; STUCK: none of them grew)
enum class BatchExit { FINISHED, SINGLE, GREW, STUCK };

struct BatchLoop {
  const char* op;              // in front of the loop's own messages
  uint32_t max_launches;       // of one call (an op that never grows: 1)
  const char* grows = nullptr; // "a slice" / "an arena": what a STUCK item reported a need for
  size_t max_slab = 0;         // bytes of one launch's slab (0: no limit) ...
  const char* slab_per = "";   // ... and what the message says it is the limit of: "call" / "launch"
};

// Launches the op's kernel, one workgroup per open item, until no item is open.  The op's callables:
//   carve(i, slab, item)    takes item i's arrays from `slab`; item == nullptr: only measures.  Returns slab.at().
//   init(i)                 item i's control block before the launch; nullptr: the blocks are zeroed on the device
//   launch(d_items, m)      the kernel, <<<m, ...>>> on ctx->stream
//   classify(i, ctl, item)  see BatchExit
// Returns the slabs, one per launch: the results of finished items stay in theirs until adopted.
template <class Item, class Ctl, class Carve, class Init, class Launch, class Classify>
std::vector<DBuf<unsigned char>> batch_launch_loop(wfst_ctx* ctx, BatchStats& stats, const BatchLoop& o, std::vector<size_t> open,
                                                   Carve carve, Init init, Launch launch, Classify classify) {
  constexpr bool zeroed = std::is_null_pointer<Init>::value;
  hipStream_t st = ctx->stream;
  std::vector<DBuf<unsigned char>> slabs;
  while (!open.empty()) {
    if (stats.launches >= o.max_launches) throw Error(std::string(o.op) + ": the arenas did not converge");
    const size_t m = open.size();
    std::vector<size_t> at(m);
    size_t bytes = (m * sizeof(Ctl) + 63) & ~(size_t)63;
    for (size_t k = 0; k < m; ++k) {
      at[k] = bytes;
      bytes = carve(open[k], Slab(nullptr, bytes), (Item*)nullptr);
    }
    if (o.max_slab && bytes > o.max_slab)
      throw Error(std::string(o.op) + ": the list needs " + std::to_string(bytes >> 20) + " MiB of scratch, more than the " +
                  std::to_string(o.max_slab >> 20) + " MiB one " + o.slab_per + " may take: split the list");
    slabs.emplace_back(*ctx->pool, bytes);
    unsigned char* base = slabs.back().p;
    Ctl* d_ctl = (Ctl*)base;
    std::vector<Item> items(m);
    std::vector<Ctl> ctls(m);
    for (size_t k = 0; k < m; ++k) {
      carve(open[k], Slab(base, at[k]), &items[k]);
      items[k].ctl = d_ctl + k;
      if constexpr (!zeroed) ctls[k] = init(open[k]);
    }
    DBuf<Item> d_items(*ctx->pool, m);
    HIP_CHECK(hipMemcpyAsync(d_items.p, items.data(), m * sizeof(Item), hipMemcpyHostToDevice, st));
    if constexpr (zeroed)
      HIP_CHECK(hipMemsetAsync(d_ctl, 0, m * sizeof(Ctl), st));
    else
      HIP_CHECK(hipMemcpyAsync(d_ctl, ctls.data(), m * sizeof(Ctl), hipMemcpyHostToDevice, st));
    launch(d_items.p, (uint32_t)m);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(ctls.data(), d_ctl, m * sizeof(Ctl), hipMemcpyDeviceToHost, st));  // the control blocks, once
    HIP_CHECK(hipStreamSynchronize(st));
    stats.launches += 1;
    std::vector<size_t> still;
    for (size_t k = 0; k < m; ++k) {
      const BatchExit e = classify(open[k], ctls[k], items[k]);
      if (e == BatchExit::STUCK) throw Error(std::string(o.op) + ": " + o.grows + " reported a need it already covers");
      if (e == BatchExit::GREW) still.push_back(open[k]);
    }
    open.swap(still);
  }
  return slabs;
}

// what becomes of item i: the single-FST path runs it, the op has its handle ready, or its arrays are adopted from a slab
struct BatchOutcome {
  enum Kind : uint8_t { SINGLE, READY, ADOPT } kind;
  wfst_fst* ready;
  AdoptDesc desc;
  static BatchOutcome single() { return {SINGLE, nullptr, {}}; }
  static BatchOutcome handle(wfst_fst* f) { return {READY, f, {}}; }
  static BatchOutcome adopt(const AdoptDesc& d) { return {ADOPT, nullptr, d}; }
};
struct BatchNoHook {
  void operator()(const std::vector<size_t>&) const {}
};

// In index order, so that the first KO is the lowest failing index: outcome(i) for every item (a throw of single(i) gets
// "item <i>: " in front), then before_adopt(the indices to adopt), then one adopt_device_many: one allocation, one
// synchronisation.  in_kernel and outs are written on success; on a throw every outs[i] made so far is deleted.
template <class Outcome, class Single, class Hook = BatchNoHook>
void batch_finish(wfst_ctx* ctx, BatchStats& stats, size_t n, wfst_fst** outs, uint8_t* in_kernel, Outcome outcome, Single single,
                  Hook before_adopt = {}) {
  try {
    std::vector<size_t> idx;
    std::vector<AdoptDesc> descs;
    std::vector<uint8_t> flag(n, 1);
    for (size_t i = 0; i < n; ++i) {
      const BatchOutcome o = outcome(i);
      if (o.kind == BatchOutcome::SINGLE) {
        try {
          outs[i] = single(i);
        } catch (const std::exception& e) {
          throw Error("item " + std::to_string(i) + ": " + e.what());
        }
        stats.items_single += 1;
        flag[i] = 0;
        continue;
      }
      stats.items_in_kernel += 1;
      if (o.kind == BatchOutcome::READY) {
        outs[i] = o.ready;
      } else {
        idx.push_back(i);
        descs.push_back(o.desc);
      }
    }
    before_adopt(idx);
    if (!idx.empty()) {
      std::vector<wfst_fst*> got(idx.size(), nullptr);
      adopt_device_many(ctx, idx.size(), descs.data(), got.data());
      for (size_t k = 0; k < idx.size(); ++k) outs[idx[k]] = got[k];
    }
    if (in_kernel) std::copy(flag.begin(), flag.end(), in_kernel);
  } catch (...) {
    for (size_t i = 0; i < n; ++i) {
      delete outs[i];
      outs[i] = nullptr;
    }
    throw;
  }
}

}  // namespace
}  // namespace wfst
