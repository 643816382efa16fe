// paths_host_loop.cpp — the comparator of tools/paths_timing.py: PathsIterator (rustfst/src/fst_traits/paths_iterator.rs:24-62)
// as a compiled host loop over the downloaded arrays of one FST, the way a shim would run it today: a FIFO of (state,
// prefix), the prefix cloned per arc, label 0 dropped per tape, tropical times in f32.  Built by the tool with the host
// compiler into a shared object; no GPU code.
#include <cstdint>
#include <cstring>
#include <deque>
#include <limits>
#include <vector>

namespace {
struct Tr {
  uint32_t ilabel, olabel;
  float weight;
  uint32_t nextstate;
};
struct Path {
  std::vector<uint32_t> il, ol;
  float w = 0.0f;
};
struct Result {
  std::vector<float> weights;
  std::vector<uint64_t> iloff{0}, oloff{0};
  std::vector<uint32_t> il, ol;
};
const float INF = std::numeric_limits<float>::infinity();
inline float times(float a, float b) { return a == INF ? a : (b == INF ? b : a + b); }
}  // namespace

extern "C" {

// max_pops bounds the loop (a cyclic input would not end); returns null beyond it
void* paths_host_run(uint32_t n_states, int64_t start, const uint32_t* off, const Tr* arcs, const float* fin, uint64_t max_pops) {
  Result* r = new Result;
  std::deque<std::pair<uint32_t, Path>> queue;
  if (start >= 0 && n_states) queue.emplace_back((uint32_t)start, Path{});
  uint64_t pops = 0;
  while (!queue.empty()) {
    if (++pops > max_pops) {
      delete r;
      return nullptr;
    }
    std::pair<uint32_t, Path> front = std::move(queue.front());
    queue.pop_front();
    const uint32_t s = front.first;
    Path& path = front.second;
    for (uint32_t i = off[s]; i < off[s + 1]; ++i) {
      Path np = path;  // clone
      if (arcs[i].ilabel != 0) np.il.push_back(arcs[i].ilabel);
      if (arcs[i].olabel != 0) np.ol.push_back(arcs[i].olabel);
      np.w = times(np.w, arcs[i].weight);
      queue.emplace_back(arcs[i].nextstate, std::move(np));
    }
    if (fin[s] != INF) {
      r->weights.push_back(times(path.w, fin[s]));
      r->il.insert(r->il.end(), path.il.begin(), path.il.end());
      r->ol.insert(r->ol.end(), path.ol.begin(), path.ol.end());
      r->iloff.push_back(r->il.size());
      r->oloff.push_back(r->ol.size());
    }
  }
  return r;
}
void paths_host_sizes(const void* h, uint64_t* n_paths, uint64_t* n_il, uint64_t* n_ol) {
  const Result* r = (const Result*)h;
  *n_paths = r->weights.size();
  *n_il = r->il.size();
  *n_ol = r->ol.size();
}
void paths_host_copy(const void* h, float* weights, uint64_t* iloff, uint32_t* il, uint64_t* oloff, uint32_t* ol) {
  const Result* r = (const Result*)h;
  if (!r->weights.empty()) std::memcpy(weights, r->weights.data(), r->weights.size() * sizeof(float));
  std::memcpy(iloff, r->iloff.data(), r->iloff.size() * sizeof(uint64_t));
  std::memcpy(oloff, r->oloff.data(), r->oloff.size() * sizeof(uint64_t));
  if (!r->il.empty()) std::memcpy(il, r->il.data(), r->il.size() * sizeof(uint32_t));
  if (!r->ol.empty()) std::memcpy(ol, r->ol.data(), r->ol.size() * sizeof(uint32_t));
}
void paths_host_free(void* h) { delete (Result*)h; }
}
