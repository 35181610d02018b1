// The host build of csrc/glibc_mathf.h and include/srr/glibc_math64.h over an array
// (tests/test_device_libm.py): the same headers the device compiles, built with
// g++ -O2 -mfma -ffp-contract=off, under the names srr_device_libm uses.
//   libm_host FN X.bin Y.bin|- OUT0.bin OUT1.bin|-
// Elements are raw float32 ("rsin" ... "atanf") or float64 ("sin64" ... "log64").
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/srr/glibc_math64.h"
#include "../../simple-raytracing-render_amd/csrc/glibc_mathf.h"

namespace gm = srr::gm;
namespace g64 = srr::gm64;

template <class T>
static bool slurp(const char* path, std::vector<T>& v) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  fseek(f, 0, SEEK_END);
  const long b = ftell(f);
  fseek(f, 0, SEEK_SET);
  v.resize((size_t)b / sizeof(T));
  const bool ok = fread(v.data(), sizeof(T), v.size(), f) == v.size();
  fclose(f);
  return ok;
}

template <class T>
static bool dump(const char* path, const std::vector<T>& v) {
  FILE* f = fopen(path, "wb");
  if (!f) return false;
  const bool ok = fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
  return fclose(f) == 0 && ok;
}

template <class T, class F>
static int run(char** a, bool two_in, bool two_out, F f) {
  std::vector<T> x, y;
  if (!slurp(a[2], x) || (two_in && (!slurp(a[3], y) || y.size() != x.size()))) return 3;
  std::vector<T> o0(x.size()), o1(two_out ? x.size() : 0);
  for (size_t i = 0; i < x.size(); ++i) {
    T s = 0, c = 0;
    f(x[i], two_in ? y[i] : T(0), s, c);
    o0[i] = s;
    if (two_out) o1[i] = c;
  }
  if (!dump(a[4], o0) || (two_out && !dump(a[5], o1))) return 4;
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 6) return 2;
  const std::string fn = argv[1];
#define F32_1(NAME, EXPR) \
  if (fn == NAME) return run<float>(argv, false, false, [](float x, float, float& o, float&) { o = EXPR; })
#define F64_1(NAME, EXPR) \
  if (fn == NAME) return run<double>(argv, false, false, [](double x, double, double& o, double&) { o = EXPR; })
  F32_1("rsin", gm::sinf_(x));
  F32_1("rcos", gm::cosf_(x));
  F32_1("rexp", gm::expf_(x));
  F32_1("rlog", gm::logf_(x));
  F32_1("racos", gm::acosf_(x));
  F32_1("rasin", gm::asinf_(x));
  F32_1("atanf", gm::atanf_(x));
  if (fn == "rpow") return run<float>(argv, true, false, [](float x, float y, float& o, float&) { o = gm::powf_(x, y); });
  if (fn == "ratan2")
    return run<float>(argv, true, false, [](float x, float y, float& o, float&) { o = gm::atan2f_(x, y); });
  if (fn == "sincosf") return run<float>(argv, false, true, [](float x, float, float& s, float& c) { gm::sincosf_(x, s, c); });
  F64_1("sin64", g64::sin(x));
  F64_1("cos64", g64::cos(x));
  F64_1("acos64", g64::acos(x));
  F64_1("log64", g64::log(x));
  if (fn == "sincos64")
    return run<double>(argv, false, true, [](double x, double, double& s, double& c) { g64::sincos(x, s, c); });
  if (fn == "atan2_64")
    return run<double>(argv, true, false, [](double x, double y, double& o, double&) { o = g64::atan2(x, y); });
  fprintf(stderr, "libm_host: no function named %s\n", fn.c_str());
  return 2;
}
