// The binary search over a batch's offset table, shared by every kernel that finds the utterance of a global row.
// Static to the including translation unit.  (owner_of in kernels_onehot.hip is no copy of it: it steps over
// repeated entries.)
#ifndef SNF_UTT_SEARCH_H_
#define SNF_UTT_SEARCH_H_

#include <hip/hip_runtime.h>

#include <cstdint>

namespace snf {

namespace {

// largest u with offsets[u] <= g (offsets[n] > g): the utterance that owns global row g
__device__ __forceinline__ int64_t find_utt(const int64_t* __restrict__ offsets, int64_t n,
                                            int64_t g) {
  int64_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (offsets[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

}  // namespace

}  // namespace snf

#endif  // SNF_UTT_SEARCH_H_
