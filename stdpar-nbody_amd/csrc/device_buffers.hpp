// The owner of a handle's memory: every device and pinned-host allocation of one handle (or of one lazily made part of it) is made
// through a device_buffers member of the handle and freed by it, once.  The handle's members stay the raw pointers the kernels and
// the launches take; they are never freed by hand.  Depends on the HIP runtime API and the standard library only, so a host compiler
// can build it against a stand-in runtime (tests/device_buffers_main.cpp).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <utility>
#include <vector>

namespace nbody {

class device_buffers {
 public:
  device_buffers() = default;
  ~device_buffers() { release(); }
  device_buffers(const device_buffers&)            = delete;
  device_buffers& operator=(const device_buffers&) = delete;

  // hipMalloc into *p, recorded.  After the first failure every later alloc and alloc_pinned is skipped without calling the runtime,
  // so a create call is a list of allocs and one look at error(), the first failure; a failed or skipped call leaves *p NULL.
  template <class P>
  void alloc(P** p, size_t bytes) {
    take(reinterpret_cast<void**>(p), bytes, false, 0);
  }
  // hipHostMalloc(flags), likewise
  template <class P>
  void alloc_pinned(P** p, size_t bytes, unsigned flags) {
    take(reinterpret_cast<void**>(p), bytes, true, flags);
  }
  // An allocation on its own, after create (counters, the quadrupole pool): its failure is returned and not kept, the call may
  // be repeated.
  template <class P>
  hipError_t alloc_late(P** p, size_t bytes) {
    alloc(p, bytes);
    const hipError_t e = first_error_;
    first_error_       = hipSuccess;
    return e;
  }
  hipError_t error() const { return first_error_; }

  // frees what was recorded, each pointer once, and forgets it and the error; the raw pointers of the handle are the caller's to reset
  void release() {
    for (const auto& [ptr, pinned] : owned_) (void)(pinned ? hipHostFree(ptr) : hipFree(ptr));
    owned_.clear();
    first_error_ = hipSuccess;
  }

 private:
  void take(void** p, size_t bytes, bool pinned, unsigned flags) {
    *p = nullptr;
    if (first_error_ != hipSuccess) return;
    owned_.reserve(owned_.size() + 1);  // before the runtime is called: recording cannot fail after it
    first_error_ = pinned ? hipHostMalloc(p, bytes, flags) : hipMalloc(p, bytes);
    if (first_error_ != hipSuccess) *p = nullptr;
    else if (*p) owned_.emplace_back(*p, pinned);
  }

  std::vector<std::pair<void*, bool>> owned_;  // (pointer, pinned host memory)
  hipError_t first_error_ = hipSuccess;
};

}  // namespace nbody
