// csrc/devmem.h on the CPU: the four HIP allocation entry points it calls are defined here
// over malloc, with a count of live allocations, a log of the calls and a "fail the k-th
// allocation" switch.  Built with -fsanitize=address,undefined and no GPU library
// (tests/test_devmem.py); a double free or a leak is the sanitizer's report, a wrong state
// is a CHECK below.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "devmem.h"

static int g_live = 0, g_pinned_live = 0, g_allocs = 0, g_fail_at = 0;  // g_fail_at: 1-based, 0 = never
static size_t g_last_bytes = 0;
static std::string g_log;  // 'A' per allocation, 'F' per free, 'x' per refused allocation

static hipError_t stub_alloc(void** p, size_t bytes, int& live) {
  if (++g_allocs == g_fail_at) {
    g_log += 'x';
    *p = (void*)0x1;  // a failed call's output is not to be trusted: the owner must not keep it
    return hipErrorOutOfMemory;
  }
  *p = malloc(bytes ? bytes : 1);
  g_last_bytes = bytes;
  g_log += 'A';
  ++live;
  return hipSuccess;
}
extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) { return stub_alloc(p, bytes, g_live); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) { return stub_alloc(p, bytes, g_pinned_live); }
hipError_t hipFree(void* p) {
  if (p) free(p), --g_live, g_log += 'F';
  return hipSuccess;
}
hipError_t hipHostFree(void* p) {
  if (p) free(p), --g_pinned_live, g_log += 'F';
  return hipSuccess;
}
}

static int g_bad = 0;
#define CHECK(c)                                                 \
  do {                                                           \
    if (!(c)) printf("line %d: %s\n", __LINE__, #c), ++g_bad;   \
  } while (0)

static void fail_next() { g_fail_at = g_allocs + 1; }
static void fail_second_next() { g_fail_at = g_allocs + 2; }

using namespace srr;

struct TwoOwners {  // stands for FrameSlot / AdaptiveState: reset by assigning a fresh one
  DeviceMem<float> a;
  PinnedMem<int> h;
};

int main() {
  {  // grow: below capacity nothing, above it one free before the one allocation
    DeviceMem<float> m;
    CHECK(m.get() == nullptr && m.capacity() == 0);
    CHECK(m.grow(0) == hipSuccess && m.get() == nullptr && g_log.empty());  // zero elements: no allocation
    CHECK(m.grow(100) == hipSuccess && m.get() && m.capacity() == 100 && g_last_bytes == 400);
    float* p = m.get();
    p[99] = 1.f;
    g_log.clear();
    CHECK(m.grow(100) == hipSuccess && m.grow(7) == hipSuccess && m.grow(0) == hipSuccess);
    CHECK(g_log.empty() && m.get() == p && m.capacity() == 100);
    CHECK(m.grow(101) == hipSuccess && g_log == "FA" && m.capacity() == 101 && g_live == 1);
    // a failed grow: the old buffer is gone (freed first), the owner empty
    g_log.clear();
    fail_next();
    CHECK(m.grow(500) == hipErrorOutOfMemory && g_log == "Fx");
    CHECK(m.get() == nullptr && m.capacity() == 0 && g_live == 0);
    // ... and nothing remembers the old capacity: a request the old buffer covered allocates
    g_log.clear();
    CHECK(m.grow(50) == hipSuccess && g_log == "A" && m.capacity() == 50 && g_live == 1);
    fail_next();
    CHECK(m.grow(60) != hipSuccess && g_live == 0);
  }  // destruction after a failed grow: nothing to free (a second free is the sanitizer's report)
  CHECK(g_live == 0);
  {  // reset, and pinned memory through the same owner
    PinnedMem<int> h;
    CHECK(h.grow(16) == hipSuccess && g_pinned_live == 1 && g_live == 0 && g_last_bytes == 64);
    h.get()[15] = 3;
    h.reset();
    CHECK(h.get() == nullptr && h.capacity() == 0 && g_pinned_live == 0);
    h.reset();
    CHECK(h.grow(1) == hipSuccess && g_pinned_live == 1);
  }
  CHECK(g_pinned_live == 0);
  {  // moves
    DeviceMem<int> a, b;
    CHECK(a.grow(10) == hipSuccess && b.grow(20) == hipSuccess && g_live == 2);
    int* pa = a.get();
    DeviceMem<int> c(std::move(a));  // moving out: the source is empty, nothing freed
    CHECK(c.get() == pa && c.capacity() == 10 && a.get() == nullptr && a.capacity() == 0 && g_live == 2);
    b = std::move(c);  // over a live owner: what it held is freed
    CHECK(b.get() == pa && b.capacity() == 10 && c.get() == nullptr && c.capacity() == 0 && g_live == 1);
    b = DeviceMem<int>{};
    CHECK(b.get() == nullptr && b.capacity() == 0 && g_live == 0);
    TwoOwners s;
    CHECK(s.a.grow(5) == hipSuccess && s.h.grow(5) == hipSuccess && g_live == 1 && g_pinned_live == 1);
    s = TwoOwners{};  // F = FrameSlot{}
    CHECK(g_live == 0 && g_pinned_live == 0 && s.a.get() == nullptr && s.h.get() == nullptr);
  }
  {  // the bag, and the 16-byte floor
    float* f = nullptr;
    double* d = nullptr;
    unsigned char* u = nullptr;
    {
      DeviceBag bag;
      CHECK(bag.add(&f, 0) == hipSuccess && f != nullptr && g_last_bytes == 16);  // an empty table is not null
      CHECK(bag.add(&u, 5) == hipSuccess && u != nullptr && g_last_bytes == 16);
      CHECK(bag.add(&d, 3) == hipSuccess && g_last_bytes == 24 && g_live == 3);
      d[2] = 1.0;
      bag.clear();
      CHECK(g_live == 0);
      CHECK(bag.add(&f, 4) == hipSuccess && bag.add(&d, 1) == hipSuccess && g_live == 2);
      fail_next();
      u = (unsigned char*)&g_bad;
      CHECK(bag.add(&u, 64) == hipErrorOutOfMemory && u == nullptr && g_live == 2);  // the earlier entries stay
      bag.clear();
      CHECK(g_live == 0);  // empty after a failed add and clear()
      bag.clear();
      CHECK(bag.add(&f, 1) == hipSuccess && bag.add(&f, 1) == hipSuccess && g_live == 2);
      DeviceBag other(std::move(bag));
      CHECK(g_live == 2);
      bag = DeviceBag{};
      CHECK(g_live == 2);
    }  // destruction frees what is left
    CHECK(g_live == 0);
    // the floor applies where it is asked for, and only there
    CHECK(at_least_16_bytes<float>(0) == 4 && at_least_16_bytes<float>(3) == 4 && at_least_16_bytes<float>(5) == 5);
    CHECK(at_least_16_bytes<unsigned char>(0) == 16 && at_least_16_bytes<double>(1) == 2);
    DeviceMem<float> m;
    CHECK(m.grow(at_least_16_bytes<float>(0)) == hipSuccess && m.get() && g_last_bytes == 16);
    DeviceMem<float> z;
    CHECK(z.grow(1) == hipSuccess && g_last_bytes == 4);  // a plain owner does not round up
  }
  {  // grow_pair, the helper the kept paths (and a pixel list with its sums) grow through
    DeviceMem<float> raw;
    DeviceMem<unsigned char> rays;
    CHECK(grow_pair(raw, 300, rays, 100) == hipSuccess && raw.capacity() == 300 && rays.capacity() == 100);
    g_log.clear();
    CHECK(grow_pair(raw, 30, rays, 10) == hipSuccess && g_log.empty());  // larger than needed: kept
    fail_second_next();  // the first allocation succeeds, the second does not
    CHECK(grow_pair(raw, 600, rays, 200) == hipErrorOutOfMemory && g_log == "FFAxF");
    CHECK(raw.get() == nullptr && rays.get() == nullptr && raw.capacity() == 0 && rays.capacity() == 0 && g_live == 0);
    // the next request that the OLD buffers would have covered allocates afresh
    g_log.clear();
    CHECK(grow_pair(raw, 300, rays, 100) == hipSuccess && g_log == "AA" && raw.get() && rays.get() && g_live == 2);
    fail_next();  // the first allocation fails: the second is not tried
    g_log.clear();
    CHECK(grow_pair(raw, 301, rays, 101) == hipErrorOutOfMemory && g_log == "FFx" && g_live == 0);
    CHECK(raw.capacity() == 0 && rays.capacity() == 0);
  }
  CHECK(g_live == 0 && g_pinned_live == 0);
  printf("devmem: %d allocations, %d live at exit, %d checks failed\n", g_allocs, g_live + g_pinned_live, g_bad);
  return g_bad != 0 || g_live != 0 || g_pinned_live != 0;
}
