// pinned_buffer.h -- DeviceBuffer's twin (device_scratch.h) for pinned and mapped host memory.  Like that header it includes
// the HIP runtime and standard headers only and compiles alone on the CPU (tests/cpp/device_scratch_test.cpp).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

// One grow-only block of pinned host memory (hipHostMalloc with `flags`) with its owner, by DeviceBuffer's rules.
// host() is the block, dev() its device address where the flags ask for a mapped block (null otherwise).  Freed with
// hipHostFree.  Movable like DeviceBuffer.  (A header of its own: device_scratch.h keeps to hipMalloc / hipFree.)
template <class T = void>
class PinnedBuffer {
 public:
  PinnedBuffer() = default;
  PinnedBuffer(const PinnedBuffer&) = delete;
  PinnedBuffer& operator=(const PinnedBuffer&) = delete;
  PinnedBuffer(PinnedBuffer&& o) noexcept : p_(o.p_), dev_(o.dev_), cap_(o.cap_) { o.p_ = o.dev_ = nullptr, o.cap_ = 0; }
  PinnedBuffer& operator=(PinnedBuffer&& o) noexcept {
    if (this != &o) {
      (void)reset();
      p_ = o.p_, dev_ = o.dev_, cap_ = o.cap_;
      o.p_ = o.dev_ = nullptr, o.cap_ = 0;
    }
    return *this;
  }
  ~PinnedBuffer() { (void)reset(); }
  hipError_t reserve(size_t bytes, unsigned flags) {
    if (cap_ >= bytes) return hipSuccess;
    hipError_t e = reset();
    if (e == hipSuccess) e = hipHostMalloc(&p_, bytes, flags);
    if (e != hipSuccess) p_ = nullptr;
    if (e == hipSuccess && (flags & hipHostMallocMapped)) {
      e = hipHostGetDevicePointer(&dev_, p_, 0);
      if (e != hipSuccess) (void)reset();
    }
    cap_ = p_ ? bytes : 0;
    return e;
  }
  hipError_t reset() {
    void* p = p_;
    p_ = dev_ = nullptr;
    cap_ = 0;
    return p ? hipHostFree(p) : hipSuccess;
  }
  T* host() const { return static_cast<T*>(p_); }
  T* dev() const { return static_cast<T*>(dev_); }
  size_t capacity() const { return cap_; }

 private:
  void* p_ = nullptr;
  void* dev_ = nullptr;
  size_t cap_ = 0;
};
