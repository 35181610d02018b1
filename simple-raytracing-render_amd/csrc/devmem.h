// Owners of the host runtime's device and pinned allocations (host translation units only):
// every hipMalloc / hipFree / hipHostMalloc / hipHostFree of renderer.cpp, capi.cpp and
// capi_kat.cpp is one of the calls below.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstddef>
#include <utility>
#include <vector>

namespace srr {

struct DeviceSpace {
  static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static void release(void* p) { (void)hipFree(p); }
};
struct PinnedSpace {
  static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static void release(void* p) { (void)hipHostFree(p); }
};

// The one rule on empty tables.  An owner asked for zero elements allocates nothing and
// stays null.  A table that a kernel is handed even when it is empty must not be null:
// its site asks for at_least_16_bytes<T>(n) elements instead (DeviceBag::add always does).
template <class T>
constexpr size_t at_least_16_bytes(size_t n) {
  return std::max(n, (16 + sizeof(T) - 1) / sizeof(T));
}

// One growable buffer, move-only.  Either it holds capacity() > 0 elements or it is
// empty (null, capacity 0); there is no state in between, whatever fails.
template <class T, class Space>
class Mem {
 public:
  Mem() = default;
  Mem(Mem&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
  Mem& operator=(Mem&& o) noexcept {
    if (this != &o) {
      reset();
      std::swap(p_, o.p_);
      std::swap(cap_, o.cap_);
    }
    return *this;
  }
  ~Mem() { reset(); }
  T* get() const { return p_; }
  size_t capacity() const { return cap_; }  // elements
  void reset() {
    if (p_) Space::release(p_);
    p_ = nullptr;
    cap_ = 0;
  }
  // Holds at least n elements afterwards; the contents are NOT preserved.  The old buffer
  // is freed before the new one is allocated (frames are sized near the device's memory);
  // on failure the owner is empty.
  hipError_t grow(size_t n) {
    if (n <= cap_) return hipSuccess;
    reset();
    const hipError_t e = Space::alloc((void**)&p_, n * sizeof(T));
    if (e == hipSuccess) cap_ = n;
    else p_ = nullptr;
    return e;
  }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};
template <class T>
using DeviceMem = Mem<T, DeviceSpace>;
template <class T>
using PinnedMem = Mem<T, PinnedSpace>;

// Two buffers that are sized together (kept paths: radiance and ray counts; a pixel list
// and its sums): both hold at least na / nb elements afterwards, or both are empty.  Both
// old buffers are freed before either new one is allocated.
template <class A, class B>
hipError_t grow_pair(DeviceMem<A>& a, size_t na, DeviceMem<B>& b, size_t nb) {
  if (na <= a.capacity() && nb <= b.capacity()) return hipSuccess;
  a.reset();
  b.reset();
  hipError_t e = a.grow(na);
  if (e == hipSuccess) e = b.grow(nb);
  if (e != hipSuccess) a.reset(), b.reset();
  return e;
}

// Many device allocations with one lifetime (a scene's tables, a lane's path state).  The
// pointers handed out stay plain, as the kernels' argument structs hold them; clear() or the
// bag's end frees them all.  Every entry has at least 16 bytes, so none is null.
class DeviceBag {
 public:
  template <class T>
  hipError_t add(T** p, size_t n) {
    *p = nullptr;
    DeviceMem<unsigned char> b;
    const hipError_t e = b.grow(at_least_16_bytes<unsigned char>(n * sizeof(T)));
    if (e != hipSuccess) return e;
    *p = (T*)b.get();
    bufs_.push_back(std::move(b));
    return e;
  }
  void clear() { bufs_.clear(); }

 private:
  std::vector<DeviceMem<unsigned char>> bufs_;
};

}  // namespace srr
