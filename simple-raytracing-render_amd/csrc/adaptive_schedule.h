// The schedule of speculative adaptive passes (include/srr_capi.h srr_adaptive_speculate):
// plain host C++, no HIP, so that the pass loops (renderer.cpp), srr_adaptive_pass_width
// (capi.cpp) and a stand-alone program under host sanitizers (tests/cpp) run one definition.
#pragma once
#include <algorithm>
#include <cstdint>

namespace srr {

// fill_paths = 0 of srr_adaptive_speculate: the 262,144 persistent lanes k_paths launches
// on an MI355X (a pass with fewer paths than lanes cannot fill the GPU) times 8, from the
// sweep on C2 in DESIGN §4.1 (profiles/r15/adaptive_spec.txt): a factor of 4 and below
// leaves the rel_tol = 0.02 frame at 16 passes, 8 takes the 0.05 frame from 16.2 to 9.9 ms
// with 4 % of the traced samples discarded, and 16 gains 0.2 ms more for twice the discard.
constexpr int64_t kAdaptiveFillDefault = (int64_t)262144 * 8;

// Samples a pass at level n (the count its n_active slots hold, n < budget) gives each
// slot: k = clamp(fill_paths / (n_active * batch_spp), 1, max(1, pass_spp_max / batch_spp))
// batches, cut at the budget.  k = 1 is the pass without speculation.  -1: an argument
// out of range.
inline int adaptive_pass_width(int64_t n_active, int n, int budget, int batch_spp, int pass_spp_max,
                               int64_t fill_paths) {
  if (n_active < 1 || n_active > ((int64_t)1 << 31) || n < 0 || budget <= n || batch_spp < 1 || pass_spp_max < 0 || fill_paths < 0) return -1;
  if (fill_paths == 0) fill_paths = kAdaptiveFillDefault;
  const int64_t kmax = std::max(1, pass_spp_max / batch_spp);
  // (n_active <= 2^31 slots of batch_spp < 2^31 samples: the product stays below 2^62)
  const int64_t k = std::min(kmax, std::max<int64_t>(1, fill_paths / (n_active * (int64_t)batch_spp)));
  return (int)std::min<int64_t>(k * batch_spp, (int64_t)budget - n);
}

}  // namespace srr
