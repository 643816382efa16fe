#include <cstdint>
#include <cstdio>
#include <new>
#include <vector>
// Test program (tests/test_host.py::test_slab_carver): for mixed sequences of take() calls of slab.h, the measuring pass and
// the filling pass end at the same offset, every pointer is 64-byte aligned and inside [base, base + measured), the arrays
// do not overlap, and a null base returns null.  Built with g++ -fsanitize=address,undefined -I<repo>/rustfst_amd/csrc.
#include "slab.h"
using wfst::Slab;

struct E16 {
  uint64_t a, b;
};
struct Take {
  size_t elt, bytes;  // element size 4, 8 or 16; the array's bytes are rounded up to whole elements
};
struct Got {
  unsigned char* p;
  size_t bytes;
};

static unsigned char* take(Slab& s, const Take& t, size_t* bytes) {
  const size_t count = (t.bytes + t.elt - 1) / t.elt;
  *bytes = count * t.elt;
  if (t.elt == 4) return (unsigned char*)s.take<uint32_t>(count);
  if (t.elt == 8) return (unsigned char*)s.take<uint64_t>(count);
  return (unsigned char*)s.take<E16>(count);
}

int main() {
  const size_t sizes[6] = {0, 1, 63, 64, 65, 4097}, elts[3] = {4, 8, 16}, heads[3] = {0, 64, 192};
  std::vector<std::vector<Take>> seqs(4);
  for (size_t b : sizes)  // every size with every element size, ascending
    for (size_t e : elts) seqs[0].push_back({e, b});
  for (size_t k = seqs[0].size(); k-- > 0;) seqs[1].push_back(seqs[0][k]);                          // descending
  for (size_t k = 0; k < 3 * seqs[0].size(); ++k) seqs[2].push_back({elts[k % 3], sizes[(5 * k + 2) % 6]});  // mixed
  for (size_t k = 0; k < 7; ++k) seqs[3].push_back({elts[k % 3], 0});                               // nothing but empty arrays
  long long n = 0, bad = 0;
  auto expect = [&](bool ok, const char* what, size_t q, size_t k) {
    ++n;
    if (!ok) {
      if (bad < 5) printf("sequence %zu, take %zu: %s\n", q, k, what);
      ++bad;
    }
  };
  for (size_t q = 0; q < seqs.size(); ++q)
    for (size_t head : heads) {  // (the control blocks in front: the carving starts at a 64-byte rounded offset)
      Slab measure(nullptr, head);
      size_t bytes = 0;
      for (size_t k = 0; k < seqs[q].size(); ++k) expect(take(measure, seqs[q][k], &bytes) == nullptr, "a null base gave a pointer", q, k);
      const size_t total = measure.at();
      // 64-byte aligned storage of exactly `total` bytes: a write past it is the sanitizer's to report
      unsigned char* base = (unsigned char*)::operator new(total ? total : 1, std::align_val_t(64));
      Slab fill(base, head);
      std::vector<Got> got;
      for (size_t k = 0; k < seqs[q].size(); ++k) {
        unsigned char* p = take(fill, seqs[q][k], &bytes);
        expect(((uintptr_t)p & 63u) == 0, "not 64-byte aligned", q, k);
        expect(p >= base + head && p + bytes <= base + total, "outside the measured slab", q, k);
        for (const Got& g : got) expect(p + bytes <= g.p || g.p + g.bytes <= p, "overlaps an earlier array", q, k);
        for (size_t j = 0; j < bytes; ++j) p[j] = (unsigned char)k;  // (every byte of every array is writable)
        got.push_back({p, bytes});
      }
      expect(fill.at() == total, "the filling pass ends elsewhere than the measuring pass", q, seqs[q].size());
      for (size_t k = 0; k < got.size(); ++k)
        for (size_t j = 0; j < got[k].bytes; ++j)
          if (got[k].p[j] != (unsigned char)k) expect(false, "a later array wrote into this one", q, k);
      ::operator delete(base, std::align_val_t(64));
    }
  printf("%lld cases, %lld mismatches (%zu sequences)\n", n, bad, seqs.size());
  return bad != 0;
}
