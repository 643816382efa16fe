// slab.h — carves the arrays of one item out of a launch's slab: every array starts on a 64-byte boundary.  A null base
// only measures: the same sequence of take() calls, once without and once with memory, gives the size and then the
// pointers (batch_driver.h).  No HIP here: tests/slab_check.cpp includes it alone.
#pragma once
#include <cstddef>

namespace wfst {
class Slab {
 public:
  Slab(unsigned char* base, size_t at) : base_(base), at_(at) {}
  template <class T>
  T* take(size_t count) {
    const size_t o = at_;
    at_ += (count * sizeof(T) + 63) & ~(size_t)63;
    return base_ ? (T*)(base_ + o) : nullptr;
  }
  size_t at() const { return at_; }  // the running offset: where the next array starts

 private:
  unsigned char* base_;
  size_t at_;
};
}  // namespace wfst
