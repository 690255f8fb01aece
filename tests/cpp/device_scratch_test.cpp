// device_scratch_test.cpp -- csrc/device_scratch.h on the CPU, over the counting hipMalloc / hipFree of
// tests/fake_include/hip_stub.  Built with -fsanitize=address,undefined and run by tests/test_device_scratch.py:
// a leak, a double free or a use after free ends the program with a non-zero status, like a failed CHECK.
#include "../../include/artp_c.h"
#include "../../art_planner_amd/csrc/device_scratch.h"
#include "../../art_planner_amd/csrc/pinned_buffer.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <utility>

struct FakeCtx {
  std::string last_error;
};

static int failures = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
      ++failures;                                                    \
    }                                                                \
  } while (0)

// The owner of an object's buffers and the six it holds: artp_tree's log in small.
struct Log {
  uint32_t *lu = nullptr, *lv = nullptr, *lb = nullptr;
  uint8_t* lval = nullptr;
  double *cuv = nullptr, *cvu = nullptr;
  size_t n = 0, cap = 0;
  DeviceScratch mem;
};

// tree_log_reserve's body: six new buffers in a local owner, copy, release the old six, hand the new six over
static int log_reserve(FakeCtx* c, Log* t, size_t cap) {
  uint32_t *lu = nullptr, *lv = nullptr, *lb = nullptr;
  uint8_t* lval = nullptr;
  double *cuv = nullptr, *cvu = nullptr;
  DeviceScratch S;
  HIP_TRY(c, S.alloc(&lu, cap));
  HIP_TRY(c, S.alloc(&lv, cap));
  HIP_TRY(c, S.alloc(&lb, cap));
  HIP_TRY(c, S.alloc(&lval, cap));
  HIP_TRY(c, S.alloc(&cuv, cap));
  HIP_TRY(c, S.alloc(&cvu, cap));
  if (t->n) {
    std::memcpy(lu, t->lu, t->n * 4);
    std::memcpy(lv, t->lv, t->n * 4);
    std::memcpy(lb, t->lb, t->n * 4);
    std::memcpy(lval, t->lval, t->n);
    std::memcpy(cuv, t->cuv, t->n * 8);
    std::memcpy(cvu, t->cvu, t->n * 8);
  }
  for (void* p : {(void*)t->lu, (void*)t->lv, (void*)t->lb, (void*)t->lval, (void*)t->cuv, (void*)t->cvu}) t->mem.release(p);
  t->lu = t->mem.adopt(S.take(lu));
  t->lv = t->mem.adopt(S.take(lv));
  t->lb = t->mem.adopt(S.take(lb));
  t->lval = t->mem.adopt(S.take(lval));
  t->cuv = t->mem.adopt(S.take(cuv));
  t->cvu = t->mem.adopt(S.take(cvu));
  t->cap = cap;
  return ARTP_OK;
}

// A field in small (csrc/field.h artp_field): plain typed pointers beside the owner of what they point to.
struct SmallField {
  FakeCtx* ctx = nullptr;
  double* dist = nullptr;     // allocated by the build, kept to the end
  float* chunk = nullptr;     // the build's scratch, given back before the build ends
  unsigned* wacc = nullptr;   // lazy: the first update of some kinds allocates it, many fields never do
  int* nodes = nullptr;       // grows with the largest request
  size_t nodes_cap = 0;
  DeviceScratch mem;
};

// field_lazy's body
template <class T>
static int small_lazy(SmallField* f, T** p, size_t count) {
  if (!*p) HIP_TRY(f->ctx, f->mem.alloc(p, count));
  return ARTP_OK;
}

// field_ensure_scratch's body: the old block released ahead of the new alloc
static int small_ensure(SmallField* f, size_t ints) {
  if (f->nodes_cap >= ints) return ARTP_OK;
  f->mem.release(f->nodes);
  f->nodes = nullptr;
  f->nodes_cap = 0;
  HIP_TRY(f->ctx, f->mem.alloc(&f->nodes, ints));
  f->nodes_cap = ints;
  return ARTP_OK;
}

// field_create's shape: build, and on a failure delete what was built so far; *out only on success
static int small_create(FakeCtx* c, SmallField** out) {
  *out = nullptr;
  SmallField* f = new SmallField;
  f->ctx = c;
  const auto build = [&]() -> int {
    HIP_TRY(c, f->mem.alloc(&f->dist, 100));
    ARTP_TRY(small_ensure(f, 6));
    ARTP_TRY(small_lazy(f, &f->chunk, 900));
    f->chunk[899] = 1.0f;
    f->mem.release(f->chunk);  // the scratch goes back here, not with the field
    f->chunk = nullptr;
    return ARTP_OK;
  };
  const int rc = build();
  if (rc) {
    delete f;
    return rc;
  }
  *out = f;
  return ARTP_OK;
}

static int try_passes_code(int rc) {
  ARTP_TRY(rc);
  return ARTP_OK;
}

int main() {
  FakeCtx ctx;
  // every failure position of a first reserve: nothing stays allocated, the error and its text come back
  const char* const exprs[6] = {"S.alloc(&lu, cap)",   "S.alloc(&lv, cap)",  "S.alloc(&lb, cap)",
                                "S.alloc(&lval, cap)", "S.alloc(&cuv, cap)", "S.alloc(&cvu, cap)"};
  for (int n = 1; n <= 6; ++n) {
    Log t;
    ctx.last_error.clear();
    hip_stub::reset(n);
    CHECK(log_reserve(&ctx, &t, 64) == ARTP_ERR_HIP);
    CHECK(hip_stub::live == 0);
    CHECK(hip_stub::mallocs == n && hip_stub::frees == n - 1);
    CHECK(ctx.last_error == std::string(exprs[n - 1]) + ": out of memory");
    CHECK(t.cap == 0 && t.lu == nullptr);
  }
  // ... and of a regrow: the old six stay the tree's, intact, and are freed with it
  for (int n = 1; n <= 6; ++n) {
    {
      Log t;
      hip_stub::reset();
      CHECK(log_reserve(&ctx, &t, 64) == ARTP_OK);
      CHECK(hip_stub::live == 6);
      t.n = 64;
      for (size_t i = 0; i < 64; ++i) t.lu[i] = (uint32_t)i, t.cvu[i] = 0.5 * (double)i;
      hip_stub::reset(n);
      CHECK(log_reserve(&ctx, &t, 128) == ARTP_ERR_HIP);
      CHECK(hip_stub::live == 6 && t.cap == 64);
      CHECK(t.lu[63] == 63u && t.cvu[63] == 31.5);
    }
    CHECK(hip_stub::live == 0);
  }
  // success: one malloc and one free per buffer, the entries copied, nothing live after the owner is gone
  {
    Log t;
    hip_stub::reset();
    CHECK(log_reserve(&ctx, &t, 64) == ARTP_OK);
    t.n = 64;
    for (size_t i = 0; i < 64; ++i) t.lv[i] = (uint32_t)(2 * i), t.lval[i] = (uint8_t)i;
    CHECK(log_reserve(&ctx, &t, 128) == ARTP_OK);
    CHECK(hip_stub::mallocs == 12 && hip_stub::frees == 6 && hip_stub::live == 6);
    CHECK(t.cap == 128 && t.lv[63] == 126u && t.lval[63] == 63);
    t.lv[127] = 1u;  // the new size is really there
  }
  CHECK(hip_stub::live == 0);
  CHECK(hip_stub::mallocs == 12 && hip_stub::frees == 12);

  // release frees exactly once: now, not again at the end of the scope, and not at all what the owner does not hold
  {
    DeviceScratch S;
    float *a = nullptr, *b = nullptr;
    hip_stub::reset();
    CHECK(S.alloc(&a, 10) == hipSuccess && S.alloc(&b, 10) == hipSuccess);
    CHECK(hip_stub::live == 2);
    S.release(a);
    CHECK(hip_stub::live == 1 && hip_stub::frees == 1);
    S.release(a);        // forgotten: no second free (the address sanitizer would end the program)
    S.release(nullptr);
    CHECK(hip_stub::live == 1 && hip_stub::frees == 1);
    b[9] = 1.0f;         // the other buffer is untouched
  }
  CHECK(hip_stub::live == 0 && hip_stub::frees == 2);

  // take: the buffer stays live and is not the destructor's any more
  {
    double* kept = nullptr;
    hip_stub::reset();
    {
      DeviceScratch S;
      double* other = nullptr;
      CHECK(S.alloc(&kept, 7) == hipSuccess && S.alloc(&other, 7) == hipSuccess);
      CHECK(S.take(kept) == kept);
    }
    CHECK(hip_stub::live == 1 && hip_stub::frees == 1);
    kept[6] = 2.0;
    CHECK(hipFree(kept) == hipSuccess);
    CHECK(hip_stub::live == 0);
  }

  // a request of zero elements is one element: a pointer that can be passed on, freed like the others
  {
    hip_stub::reset();
    {
      DeviceScratch S;
      uint32_t* z = nullptr;
      void* raw = nullptr;
      CHECK(S.alloc(&z, 0) == hipSuccess && z != nullptr);
      z[0] = 7u;
      CHECK(S.alloc(&raw, 0) == hipSuccess && raw != nullptr);  // the untyped form counts bytes
      CHECK(hip_stub::live == 2);
    }
    CHECK(hip_stub::live == 0 && hip_stub::frees == 2);
  }

  // a failed alloc leaves a null pointer and nothing to free
  {
    hip_stub::reset(1);
    DeviceScratch S;
    int* p = reinterpret_cast<int*>(&ctx);
    CHECK(S.alloc(&p, 4) == hipErrorOutOfMemory && p == nullptr);
    CHECK(hip_stub::live == 0);
  }

  // a field in small: every failure position of the build frees what the build had, and nothing twice
  for (int n = 1; n <= 3; ++n) {
    SmallField* f = reinterpret_cast<SmallField*>(&ctx);
    hip_stub::reset(n);
    CHECK(small_create(&ctx, &f) == ARTP_ERR_HIP && f == nullptr);
    CHECK(hip_stub::live == 0 && hip_stub::mallocs == n && hip_stub::frees == n - 1);
  }
  // ... a field that is built and destroyed: the lazy buffer never allocated, the build's scratch long gone
  {
    SmallField* f = nullptr;
    hip_stub::reset();
    CHECK(small_create(&ctx, &f) == ARTP_OK && f != nullptr);
    CHECK(hip_stub::live == 2 && hip_stub::frees == 1 && f->chunk == nullptr && f->wacc == nullptr);
    delete f;
    CHECK(hip_stub::live == 0 && hip_stub::mallocs == 3 && hip_stub::frees == 3);
  }
  // ... and one that lives: the lazy buffer allocated once, the scratch back for good, two regrows, a failed third
  {
    SmallField* f = nullptr;
    hip_stub::reset();
    CHECK(small_create(&ctx, &f) == ARTP_OK);
    CHECK(small_lazy(f, &f->wacc, 9) == ARTP_OK && small_lazy(f, &f->wacc, 9) == ARTP_OK);
    CHECK(hip_stub::mallocs == 4 && hip_stub::live == 3);
    f->wacc[8] = 1u;
    CHECK(small_lazy(f, &f->chunk, 900) == ARTP_OK && small_lazy(f, &f->chunk, 900) == ARTP_OK);  // kept from here on
    f->chunk[899] = 2.0f;
    int* const first = f->nodes;
    CHECK(small_ensure(f, 4) == ARTP_OK && f->nodes == first && f->nodes_cap == 6);  // fits: nothing happens
    CHECK(small_ensure(f, 64) == ARTP_OK && f->nodes_cap == 64);
    f->nodes[63] = 1;
    CHECK(small_ensure(f, 640) == ARTP_OK && f->nodes_cap == 640);
    f->nodes[639] = 1;
    CHECK(hip_stub::mallocs == 7 && hip_stub::frees == 3 && hip_stub::live == 4);
    hip_stub::reset(1);
    ctx.last_error.clear();
    CHECK(small_ensure(f, 6400) == ARTP_ERR_HIP && f->nodes == nullptr && f->nodes_cap == 0);  // the old block is gone,
    CHECK(ctx.last_error == "f->mem.alloc(&f->nodes, ints): out of memory");                   // the field says so
    CHECK(hip_stub::live == 3);
    f->dist[99] = 1.0;  // the others are untouched
    delete f;
    CHECK(hip_stub::live == 0);
  }

  // DeviceBuffer: the grow-only block of a context or a lane
  {
    hip_stub::reset();
    {
      DeviceBuffer<int> b;
      CHECK(b.get() == nullptr && b.capacity() == 0);
      CHECK(b.reserve(0) == hipSuccess && hip_stub::mallocs == 0);   // nothing asked, nothing done
      CHECK(b.reserve(64) == hipSuccess && b.get() != nullptr && b.capacity() == 64);
      int* const first = b.get();
      first[15] = 1;
      CHECK(b.reserve(64) == hipSuccess && b.reserve(8) == hipSuccess);   // fits: no allocation, the same block
      CHECK(b.get() == first && b.capacity() == 64 && hip_stub::mallocs == 1 && hip_stub::frees == 0);
      CHECK(b.reserve(65) == hipSuccess && b.capacity() == 65);           // exactly what was asked for
      CHECK(hip_stub::mallocs == 2 && hip_stub::frees == 1 && hip_stub::live == 1);
      b.as<char>()[64] = 1;
    }
    CHECK(hip_stub::live == 0 && hip_stub::frees == 2);   // destruction frees exactly once
  }
  // ... a regrow frees the old block BEFORE it allocates: at the failing allocation nothing is live any more
  {
    DeviceBuffer<> b;
    hip_stub::reset();
    CHECK(b.reserve(100) == hipSuccess && hip_stub::live == 1);
    hip_stub::reset(1);
    CHECK(b.reserve(200) == hipErrorOutOfMemory);
    CHECK(hip_stub::frees == 1 && hip_stub::mallocs == 1 && hip_stub::live == 0);
    CHECK(b.get() == nullptr && b.capacity() == 0);   // empty, not "null with the old capacity"
    // the request the open-coded idiom let through with a null pointer: smaller than the block that was lost
    CHECK(b.reserve(50) == hipSuccess && b.get() != nullptr && b.capacity() == 50);
    CHECK(hip_stub::mallocs == 2 && hip_stub::live == 1);
    b.as<char>()[49] = 1;
    CHECK(b.reset() == hipSuccess && b.get() == nullptr && b.capacity() == 0 && hip_stub::live == 0);
    CHECK(b.reset() == hipSuccess && hip_stub::frees == 2);   // nothing left to free a second time
  }
  CHECK(hip_stub::live == 0);
  // ... a first reserve that fails, and a block handed over from another allocator call
  {
    hip_stub::reset(1);
    DeviceBuffer<float> b;
    CHECK(b.reserve(16) == hipErrorOutOfMemory && b.get() == nullptr && b.capacity() == 0);
    void* p = nullptr;
    CHECK(hipMalloc(&p, 32) == hipSuccess);
    b.adopt(p, 32);
    CHECK(b.get() == p && b.capacity() == 32 && b.reserve(32) == hipSuccess && hip_stub::mallocs == 2);
  }
  CHECK(hip_stub::live == 0 && hip_stub::frees == 1);
  // ... moved: the block changes owner without a malloc or a free, the moved-from buffer is empty and can be used again
  {
    hip_stub::reset();
    {
      DeviceBuffer<int> a;
      CHECK(a.reserve(64) == hipSuccess);
      int* const block = a.get();
      block[15] = 7;
      DeviceBuffer<int> b(std::move(a));                                  // move construction
      CHECK(b.get() == block && b.capacity() == 64 && a.get() == nullptr && a.capacity() == 0);
      CHECK(hip_stub::mallocs == 1 && hip_stub::frees == 0 && hip_stub::live == 1);
      DeviceBuffer<int> e;
      e = std::move(b);                                                   // move assignment onto an empty buffer
      CHECK(e.get() == block && e.capacity() == 64 && b.get() == nullptr && b.capacity() == 0 && hip_stub::frees == 0);
      DeviceBuffer<int>& self = e;
      e = std::move(self);                                                // onto itself: nothing changes, nothing freed
      CHECK(e.get() == block && e.capacity() == 64 && e.get()[15] == 7 && hip_stub::frees == 0 && hip_stub::live == 1);
      DeviceBuffer<int> full;
      CHECK(full.reserve(32) == hipSuccess && hip_stub::live == 2);
      full = std::move(e);                                                // onto a non-empty buffer: its block goes first
      CHECK(full.get() == block && full.capacity() == 64 && e.get() == nullptr && e.capacity() == 0);
      CHECK(hip_stub::frees == 1 && hip_stub::live == 1 && full.get()[15] == 7);
      CHECK(a.reserve(8) == hipSuccess && a.get() != nullptr && hip_stub::live == 2);  // a moved-from buffer grows again
      // a struct of such members swaps whole (the roadmap's std::swap): three moves, no malloc, no free
      struct Pair { DeviceBuffer<int> x; DeviceBuffer<> y; int tag; };
      Pair p, q;
      p.tag = 1, q.tag = 2;
      CHECK(p.x.reserve(16) == hipSuccess && q.y.reserve(24) == hipSuccess);
      int* const px = p.x.get();
      void* const qy = q.y.get();
      const int m = hip_stub::mallocs, f = hip_stub::frees;
      std::swap(p, q);
      CHECK(q.x.get() == px && p.y.get() == qy && p.x.get() == nullptr && q.y.get() == nullptr && p.tag == 2);
      CHECK(hip_stub::mallocs == m && hip_stub::frees == f && hip_stub::live == 4);
    }
    CHECK(hip_stub::live == 0 && hip_stub::mallocs == hip_stub::frees);   // every block freed exactly once
  }

  // PinnedBuffer: the same rules, freed with the host call and never the device one
  {
    hip_stub::reset();
    {
      PinnedBuffer<double> m, plain;
      CHECK(m.reserve(56, hipHostMallocMapped) == hipSuccess && m.host() != nullptr && m.dev() == m.host());
      CHECK(plain.reserve(56, hipHostMallocDefault) == hipSuccess && plain.host() != nullptr && plain.dev() == nullptr);
      m.host()[6] = 1.0;
      double* const first = m.host();
      CHECK(m.reserve(8, hipHostMallocMapped) == hipSuccess && m.host() == first && hip_stub::host_mallocs == 2);
      CHECK(m.reserve(112, hipHostMallocMapped) == hipSuccess && m.capacity() == 112 && m.dev() == m.host());
      CHECK(hip_stub::host_mallocs == 3 && hip_stub::host_frees == 1 && hip_stub::host_live == 2);
      m.host()[13] = 1.0;
    }
    CHECK(hip_stub::host_live == 0 && hip_stub::host_frees == 3);
    CHECK(hip_stub::mallocs == 0 && hip_stub::frees == 0 && hip_stub::live == 0);   // no device call at all
  }
  {
    PinnedBuffer<> m;
    hip_stub::reset();
    CHECK(m.reserve(100, hipHostMallocMapped) == hipSuccess);
    hip_stub::reset(1);
    CHECK(m.reserve(200, hipHostMallocMapped) == hipErrorOutOfMemory);
    CHECK(hip_stub::host_frees == 1 && hip_stub::host_live == 0);
    CHECK(m.host() == nullptr && m.dev() == nullptr && m.capacity() == 0);
    CHECK(m.reserve(50, hipHostMallocMapped) == hipSuccess && m.host() != nullptr && m.capacity() == 50);
    // no device address for a mapped block: the block goes back, the buffer is empty
    hip_stub::fail_dev_ptr = true;
    CHECK(m.reserve(400, hipHostMallocMapped) == hipErrorOutOfMemory);
    CHECK(m.host() == nullptr && m.dev() == nullptr && m.capacity() == 0 && hip_stub::host_live == 0);
    hip_stub::fail_dev_ptr = false;
    CHECK(hip_stub::frees == 0);
  }
  // ... moved: host and device address travel together
  {
    hip_stub::reset();
    {
      PinnedBuffer<double> a;
      CHECK(a.reserve(56, hipHostMallocMapped) == hipSuccess);
      double* const block = a.host();
      block[6] = 3.0;
      PinnedBuffer<double> b(std::move(a));
      CHECK(b.host() == block && b.dev() == block && b.capacity() == 56);
      CHECK(a.host() == nullptr && a.dev() == nullptr && a.capacity() == 0 && hip_stub::host_frees == 0);
      PinnedBuffer<double>& self = b;
      b = std::move(self);
      CHECK(b.host() == block && b.dev() == block && b.capacity() == 56 && hip_stub::host_frees == 0);
      PinnedBuffer<double> full;
      CHECK(full.reserve(16, hipHostMallocDefault) == hipSuccess && hip_stub::host_live == 2);
      full = std::move(b);
      CHECK(full.host() == block && full.dev() == block && full.capacity() == 56 && full.host()[6] == 3.0);
      CHECK(b.host() == nullptr && b.dev() == nullptr && b.capacity() == 0);
      CHECK(hip_stub::host_frees == 1 && hip_stub::host_live == 1);
      CHECK(a.reserve(8, hipHostMallocDefault) == hipSuccess && a.host() != nullptr && a.dev() == nullptr);
    }
    CHECK(hip_stub::host_live == 0 && hip_stub::host_mallocs == hip_stub::host_frees && hip_stub::frees == 0);
  }

  CHECK(try_passes_code(ARTP_OK) == ARTP_OK);
  CHECK(try_passes_code(ARTP_ERR_CAPACITY) == ARTP_ERR_CAPACITY);

  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("device_scratch ok\n");
  return 0;
}
