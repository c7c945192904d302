// best_model_device.h -- the best-model rule of a RANSAC fit over one block of candidates, stated once.
//
// The rule (src/RansacFitter.h:196-214 with the tries in order): the first eligible candidate whose inlier share
// reaches the required one wins and ends the search; else, with find_best, the eligible candidate with the most
// inliers, the earliest among equals, wins if it has more inliers than the model kept so far.  ransac_reduce_kernel
// (ransac.hip), ransac_batch_reduce_kernel (ransac_batch.hip) and resect_reduce_kernel (resect_batch.hip) call it
// and copy the winner into their own state; what "reaches" means is the caller's: above the share for the two-view
// fits, at or above it for resection.
#pragma once

#include "common.h"

namespace spv {

// For every thread of a workgroup of THREADS threads, all of which must call it: the index of the winner among the
// candidates [0, ncand), or -1 when the kept model stands; *success: the winner reached the required share.
//   over      the kept model has already succeeded: no candidate is looked at
//   npt       the rows of the set, as a double: a candidate's share is (double)count / npt
//   kept      the inliers of the kept model, 0 where there is none
//   count_of  (int i) -> the inlier count of candidate i, negative where i is not eligible
//   reaches   (double share) -> whether that share meets the required one
// A candidate without an inlier never wins on count: its count is not above `kept`.
template <int THREADS, typename CountOf, typename Reaches>
__device__ __forceinline__ int best_model(int ncand, bool over, double npt, int kept, int find_best, CountOf count_of,
                                          Reaches reaches, int *success) {
  __shared__ unsigned int s_first;
  __shared__ unsigned long long s_best;
  if (threadIdx.x == 0) {
    s_first = 0xFFFFFFFFu;
    s_best = 0ull;
  }
  __syncthreads();
  unsigned int first = 0xFFFFFFFFu;
  unsigned long long best = 0ull;
  for (int i = threadIdx.x; i < ncand && !over; i += THREADS) {
    const int c = count_of(i);
    if (c < 0) continue;
    if (reaches((double)c / npt)) first = min(first, (unsigned int)i);
    // most inliers, the earliest among equals
    if (find_best) best = max(best, ((unsigned long long)(unsigned int)c << 32) | (0xFFFFFFFFu - (unsigned int)i));
  }
  if (first != 0xFFFFFFFFu) atomicMin(&s_first, first);
  if (best) atomicMax(&s_best, best);
  __syncthreads();
  *success = 0;
  if (s_first != 0xFFFFFFFFu) {
    *success = 1;
    return (int)s_first;
  }
  if ((int)(s_best >> 32) > kept) return (int)(0xFFFFFFFFu - (unsigned int)(s_best & 0xFFFFFFFFu));
  return -1;
}

}  // namespace spv
