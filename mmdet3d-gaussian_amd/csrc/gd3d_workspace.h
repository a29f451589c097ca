// gd3d_workspace.h — how every indexed op cuts its caller's workspace into buffers: ONE text per op gives both the pointers and
// the size, because the *_workspace_bytes entry runs the same carve at address 0.  Host only, no HIP include (the `_cpu` twins and the
// drivers of tests/hostmath use it).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace gd3d {

inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

// Buffers in sequence, each at a multiple of 256 bytes.  The two contracts of include/gd3d.h:
//   caller-aligned  the entry refuses a workspace that is not 256-byte aligned; bytes() is the extent from the base;
//   self-aligning   the base is rounded up to 256 here and bytes() carries 256 bytes of slack for it: the entry compares the
//                   caller's workspace_bytes against it.
class Carver {
 public:
  enum Contract { CALLER_ALIGNED, SELF_ALIGNING };
  Carver(const void* base, Contract c)
      : first_(c == SELF_ALIGNING ? up256((uintptr_t)base) : (uintptr_t)base), at_(first_), slack_(c == SELF_ALIGNING ? 256 : 0) {}
  template <class T>
  T* take(size_t count) {
    T* p = reinterpret_cast<T*>(at_);
    at_ += up256(count * sizeof(T));
    return p;
  }
  size_t bytes() const { return (size_t)(at_ - first_) + slack_; }

 private:
  uintptr_t first_, at_;
  size_t slack_;
};

}  // namespace gd3d
