// What the translation units of the C-ABI share (capi.cpp: the product's entry points;
// capi_kat.cpp: the test entry points): the error text, the scene handle and DevBuf.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/srr_capi.h"
#include "devmem.h"
#include "scene.h"

struct srr_scene {
  srr::Scene s;
};

namespace srr {
// sets the calling thread's srr_last_error text and returns code (defined in capi.cpp)
int fail(int code, const std::string& msg);

#define HIPCHK(x)                                                                         \
  do {                                                                                    \
    hipError_t e_ = (x);                                                                  \
    if (e_ != hipSuccess) return fail(SRR_EIO, std::string(#x) + ": " + hipGetErrorString(e_)); \
  } while (0)

// One device allocation (a devmem.h owner), freed when it goes out of scope, so that an entry
// point can return at its first error.  The constructors take the call's error code: with rc != 0 they do
// nothing, and a failure sets rc (and the error text), so a run of declarations needs one
// `if (rc) return rc;` after it.  Zero elements: no allocation and a null pointer.
template <class T>
class DevBuf {
 public:
  DevBuf(size_t n, int& rc) {  // n elements, uninitialised
    if (!rc && m_.grow(n) != hipSuccess) rc = fail(SRR_ENOMEM, "device allocation failed");
  }
  DevBuf(const T* host, size_t n, int& rc) : DevBuf(n, rc) {  // a copy of host[0 .. n)
    if (!rc && n && hipMemcpy(get(), host, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess)
      rc = fail(SRR_EIO, "copy to device failed");
  }
  DevBuf(const std::vector<T>& v, int& rc) : DevBuf(v.data(), v.size(), rc) {}
  T* get() const { return m_.get(); }
  // false if the copy failed; the caller words the error (it knows which kernel ran)
  bool download(T* host, size_t n) const { return hipMemcpy(host, get(), n * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess; }

 private:
  DeviceMem<T> m_;  // (move-only, and so is DevBuf)
};
}  // namespace srr
