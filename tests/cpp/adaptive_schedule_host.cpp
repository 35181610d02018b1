// The schedule of speculative adaptive passes (csrc/adaptive_schedule.h) on the CPU, built
// with -fsanitize=address,undefined (tests/test_adaptive_spec.py): every width over a
// grid that includes the extremes of each argument is checked against the definition
// written out in 128-bit integers, so an overflow fails twice, by value and by UBSan.
#include <cstdio>
#include <initializer_list>

#include "adaptive_schedule.h"

int main() {
  using srr::adaptive_pass_width;
  const int64_t big_n = (int64_t)1 << 31;
  long checked = 0, failed = 0;
  for (int64_t n_active : {(int64_t)1, (int64_t)2, (int64_t)1073, (int64_t)262144, big_n - 1, big_n})
    for (int batch : {1, 4, 6, 64, 2147483647})
      for (int pmax : {0, 1, 3, 8, 10, 12, 1024, 2147483647})
        for (int64_t fill : {(int64_t)0, (int64_t)1, (int64_t)6000, (int64_t)1 << 40, INT64_MAX})
          for (int budget : {1, 30, 32, 1024, 2147483647})
            for (int n : {0, 1, 8, 29, 1023, 2147483646}) {
              const int w = adaptive_pass_width(n_active, n, budget, batch, pmax, fill);
              ++checked;
              if (n >= budget) {
                failed += w != -1;
                continue;
              }
              const __int128 f = fill ? fill : srr::kAdaptiveFillDefault;
              __int128 kmax = pmax / batch;
              if (kmax < 1) kmax = 1;
              __int128 k = f / ((__int128)n_active * batch);
              if (k < 1) k = 1;
              if (k > kmax) k = kmax;
              __int128 want = k * batch;
              if (want > (__int128)budget - n) want = (__int128)budget - n;
              if (w != (int)want || w < 1) {
                ++failed;
                printf("width(%lld, %d, %d, %d, %d, %lld) = %d, want %d\n", (long long)n_active, n, budget, batch, pmax,
                       (long long)fill, w, (int)want);
              }
            }
  // refusals
  const int bad[] = {adaptive_pass_width(0, 0, 8, 4, 8, 0),  adaptive_pass_width(big_n + 1, 0, 8, 4, 8, 0),
                     adaptive_pass_width(1, -1, 8, 4, 8, 0), adaptive_pass_width(1, 8, 8, 4, 8, 0),
                     adaptive_pass_width(1, 0, 8, 0, 8, 0),  adaptive_pass_width(1, 0, 8, 4, -1, 0),
                     adaptive_pass_width(1, 0, 8, 4, 8, -1)};
  for (int b : bad) {
    ++checked;
    failed += b != -1;
  }
  printf("%ld widths checked, %ld checks failed\n", checked, failed);
  return failed ? 1 : 0;
}
