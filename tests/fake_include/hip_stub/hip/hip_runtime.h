// Stand-in for <hip/hip_runtime.h> on the CPU: just what csrc/device_scratch.h and csrc/pinned_buffer.h use.  hipMalloc / hipFree and
// hipHostMalloc / hipHostFree go to malloc / free and count what is live; an allocation of either kind can be told to fail
// at its n-th call, counted over both kinds (tests/cpp/device_scratch_test.cpp).
#pragma once

#include <cstddef>
#include <cstdlib>

enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 };

namespace hip_stub {
inline int live = 0;          // allocations not yet freed
inline int mallocs = 0;       // hipMalloc calls since reset()
inline int frees = 0;         // hipFree calls of a non-null pointer since reset()
inline int fail_at = 0;       // the allocation call (1-based, counted from reset()) that fails; 0 = none
inline int host_live = 0;     // the same three counts for pinned host memory
inline int host_mallocs = 0;
inline int host_frees = 0;
inline bool fail_dev_ptr = false;  // hipHostGetDevicePointer fails
inline void reset(int fail_at_call = 0) {
  mallocs = frees = host_mallocs = host_frees = 0;
  fail_at = fail_at_call;
  fail_dev_ptr = false;
}
}  // namespace hip_stub

inline const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "out of memory"; }

inline hipError_t hipMalloc(void** p, size_t bytes) {
  *p = nullptr;
  if (++hip_stub::mallocs + hip_stub::host_mallocs == hip_stub::fail_at) return hipErrorOutOfMemory;
  if (bytes == 0) return hipSuccess;  // like the runtime: success and a null pointer
  *p = std::malloc(bytes);
  if (!*p) return hipErrorOutOfMemory;
  ++hip_stub::live;
  return hipSuccess;
}

inline hipError_t hipFree(void* p) {
  if (!p) return hipSuccess;
  ++hip_stub::frees;
  --hip_stub::live;
  std::free(p);  // a second free of the same pointer is what the address sanitizer reports
  return hipSuccess;
}

// Pinned host memory.  A pinned block starts kHostOffset bytes into its malloc block, so the wrong free is caught: hipFree
// of a pinned block, or hipHostFree of a device block, is an invalid free for the address sanitizer.
constexpr unsigned hipHostMallocDefault = 0x0, hipHostMallocMapped = 0x2;
constexpr size_t kHostOffset = 64;

inline hipError_t hipHostMalloc(void** p, size_t bytes, unsigned /*flags*/) {
  *p = nullptr;
  if (hip_stub::mallocs + ++hip_stub::host_mallocs == hip_stub::fail_at) return hipErrorOutOfMemory;
  char* raw = static_cast<char*>(std::malloc(bytes + kHostOffset));
  if (!raw) return hipErrorOutOfMemory;
  *p = raw + kHostOffset;
  ++hip_stub::host_live;
  return hipSuccess;
}

inline hipError_t hipHostFree(void* p) {
  if (!p) return hipSuccess;
  ++hip_stub::host_frees;
  --hip_stub::host_live;
  std::free(static_cast<char*>(p) - kHostOffset);
  return hipSuccess;
}

// the device address of a mapped block: the same address, as on a device with unified addressing
inline hipError_t hipHostGetDevicePointer(void** dev, void* host, unsigned /*flags*/) {
  *dev = hip_stub::fail_dev_ptr ? nullptr : host;
  return hip_stub::fail_dev_ptr ? hipErrorOutOfMemory : hipSuccess;
}
