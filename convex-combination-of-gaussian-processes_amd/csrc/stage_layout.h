// Layout of a device buffer as a sequence of 256-byte aligned pieces, declared ONCE per call site and run twice:
// without a base it only measures (take returns nullptr, off advances), with a base it hands out the pointers.  The
// size a buffer is allocated with and the pointers carved from it therefore cannot disagree.  No HIP include: the
// CPU suite compiles this header with the host compiler (tests/host_stage).
#pragma once

#include <cstddef>

namespace ccgp {

struct Layout {
  char* base;
  size_t off = 0;
  explicit Layout(void* p = nullptr) : base(static_cast<char*>(p)) {}
  static size_t al(size_t b) { return (b + 255) / 256 * 256; }
  template <class T>
  T* take(size_t count) {
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += al(count * sizeof(T));
    return p;
  }
};

// bytes of the layout that `lay` declares
template <class F>
size_t layout_bytes(F&& lay) {
  Layout plan;
  lay(plan);
  return plan.off;
}

}  // namespace ccgp
