// Stand-in for <hip/hip_runtime.h> on the CPU: just what csrc/device_scratch.h uses.  hipMalloc / hipFree go to
// malloc / free, count what is live, and hipMalloc can be told to fail at its n-th call (tests/cpp/device_scratch_test.cpp).
#pragma once

#include <cstddef>
#include <cstdlib>

enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 };

namespace hip_stub {
inline int live = 0;          // allocations not yet freed
inline int mallocs = 0;       // hipMalloc calls since reset()
inline int frees = 0;         // hipFree calls of a non-null pointer since reset()
inline int fail_at = 0;       // the hipMalloc call (1-based, counted from reset()) that fails; 0 = none
inline void reset(int fail_at_call = 0) {
  mallocs = frees = 0;
  fail_at = fail_at_call;
}
}  // namespace hip_stub

inline const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "out of memory"; }

inline hipError_t hipMalloc(void** p, size_t bytes) {
  *p = nullptr;
  if (++hip_stub::mallocs == hip_stub::fail_at) return hipErrorOutOfMemory;
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
