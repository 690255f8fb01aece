// device_scratch.h -- who frees device memory, and the one pair of error macros of the host code (pinned host memory:
// pinned_buffer.h).  Includes the HIP runtime and standard headers only, so it compiles alone on the CPU
// (tests/cpp/device_scratch_test.cpp).  The macros expand ARTP_OK / ARTP_ERR_HIP (include/artp_c.h) where they are used.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <string>
#include <vector>

// a failed HIP call: its text and HIP's message go to ctx->last_error, the function returns ARTP_ERR_HIP
#define HIP_TRY(ctx, expr)                                                        \
  do {                                                                            \
    hipError_t _e = (expr);                                                       \
    if (_e != hipSuccess) {                                                       \
      (ctx)->last_error = std::string(#expr) + ": " + hipGetErrorString(_e);      \
      return ARTP_ERR_HIP;                                                        \
    }                                                                             \
  } while (0)
// a failed call of our own (it has set last_error): the function returns its code
#define ARTP_TRY(expr)                \
  do {                                \
    const int _rc = (expr);           \
    if (_rc != ARTP_OK) return _rc;   \
  } while (0)

// Owner of device allocations: what it still holds when it goes out of scope is freed, on every way out.  Declared at
// the top of the scope that owns the buffers (a function's temporaries) or as a member (an object's buffers).  Plain
// hipMalloc / hipFree: a hipFree waits for the device, so where and how often memory is freed is part of a step's time.
// (DeviceBuffer below and PinnedBuffer can be moved; a DeviceScratch hands single buffers over with take / adopt.)
class DeviceScratch {
 public:
  DeviceScratch() = default;
  DeviceScratch(const DeviceScratch&) = delete;
  DeviceScratch& operator=(const DeviceScratch&) = delete;
  ~DeviceScratch() {
    for (void* p : ptrs_) (void)hipFree(p);
  }
  // count elements of T (at least one: the pointer is never null on success); *out = nullptr on failure
  template <class T>
  hipError_t alloc(T** out, size_t count) {
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T));
    if (e == hipSuccess) ptrs_.push_back(p);
    *out = static_cast<T*>(p);
    return e;
  }
  hipError_t alloc(void** out, size_t bytes) { return alloc(reinterpret_cast<char**>(out), bytes); }
  // frees p now (early, to keep peak memory down, or ahead of a regrow); a pointer not held here, or null, is left alone
  void release(void* p) {
    if (forget(p)) (void)hipFree(p);
  }
  // hands p over to the caller: it is no longer freed here
  template <class T>
  T* take(T* p) {
    forget(p);
    return p;
  }
  // the other half of a hand-over between two owners: a buffer taken from another owner is freed here from now on
  template <class T>
  T* adopt(T* p) {
    if (p) ptrs_.push_back(p);
    return p;
  }

 private:
  bool forget(void* p) {
    const auto it = std::find(ptrs_.begin(), ptrs_.end(), p);
    if (p == nullptr || it == ptrs_.end()) return false;
    ptrs_.erase(it);
    return true;
  }
  std::vector<void*> ptrs_;
};

// One grow-only block of device memory with its owner: a member of whatever keeps the block (artp_ctx, a lane, a
// roadmap).  The caller decides how much to ask for (padding is its policy); the block is freed with its owner.
// Movable, not copyable, so that an object made of such members can be swapped whole: the moved-from buffer is empty,
// the assigned-to buffer frees what it held first, a move onto itself changes nothing.
template <class T = void>
class DeviceBuffer {
 public:
  DeviceBuffer() = default;
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  DeviceBuffer(DeviceBuffer&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
  DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {
    if (this != &o) {
      adopt(o.p_, o.cap_);
      o.p_ = nullptr, o.cap_ = 0;
    }
    return *this;
  }
  ~DeviceBuffer() { (void)reset(); }
  // Nothing if `bytes` fit; else the old block is freed FIRST (peak memory: one block), then exactly `bytes` are
  // allocated.  After a failure the buffer is empty -- null and capacity 0 -- so the next request allocates again.
  hipError_t reserve(size_t bytes) {
    if (cap_ >= bytes) return hipSuccess;
    hipError_t e = reset();
    if (e == hipSuccess) e = hipMalloc(&p_, bytes);
    if (e != hipSuccess) p_ = nullptr;
    cap_ = p_ ? bytes : 0;
    return e;
  }
  hipError_t reset() {  // frees the block now
    void* p = p_;
    p_ = nullptr;
    cap_ = 0;
    return p ? hipFree(p) : hipSuccess;
  }
  // a block from another owner (DeviceScratch::take), or one that hipFree frees but hipMalloc did not make
  // (hipExtMallocWithFlags), is freed here from now on; what the buffer held is freed first
  void adopt(void* p, size_t bytes) {
    (void)reset();
    p_ = p;
    cap_ = p ? bytes : 0;
  }
  T* get() const { return static_cast<T*>(p_); }
  template <class U>
  U* as() const { return static_cast<U*>(p_); }
  size_t capacity() const { return cap_; }

 private:
  void* p_ = nullptr;
  size_t cap_ = 0;
};
