// What the sampled pairwise SGD kernels (bpr.hip, warp.hip) have in common: the lane-group layout of a sample, the G-ary
// membership search of a sorted CSR row, the count reduction, the dispatch over columns per lane, the cap on samples in
// flight and the id pre-pass that runs before either update kernel.
#ifndef IMPLICIT_AMD_CSRC_PAIR_SGD_H_
#define IMPLICIT_AMD_CSRC_PAIR_SGD_H_
#include <algorithm>
#include <type_traits>

#include "common.h"

namespace imp {

// the lanes of the aligned group of G = 16 / 32 / 64 that `lane` belongs to, as a ballot mask
template <int G> __device__ __forceinline__ uint64_t group_mask(int lane) {
  return G == 64 ? ~0ull : ((1ull << G) - 1) << (lane & ~(G - 1));
}

// Whether item j is among itemids[lo, hi), a sorted CSR row.  A G-ary search: the group's lanes load G splitters of the range, a
// ballot narrows it to one of G slices -- ceil(log_G(hi - lo)) dependent loads instead of log2.  Every active lane of the group
// passes the same lo, hi and j and gets the same answer; lanes of other groups may be inactive or searching other rows.
template <int G>
__device__ __forceinline__ bool group_row_contains(const int32_t *__restrict__ itemids, int64_t lo, int64_t hi, int j, int gl,
                                                   uint64_t gmask) {
  while (hi - lo > G) {  // group-uniform trip count
    const int64_t step = (hi - lo + G - 1) / G;
    const int64_t p = lo + gl * step;
    // lanes whose splitter is <= j form a prefix of the group (sorted row): the answer lies in slice k-1
    const int k = __popcll(__builtin_amdgcn_ballot_w64(p < hi && itemids[p] <= j) & gmask);
    if (k == 0) {
      hi = lo;  // j precedes the whole row
      break;
    }
    lo += (int64_t)(k - 1) * step;
    hi = lo + step < hi ? lo + step : hi;
  }
  const int64_t p = lo + gl;
  return (__builtin_amdgcn_ballot_w64(p < hi && itemids[p] == j) & gmask) != 0;
}

// Two per-lane counts of a 256-thread workgroup into stats[0] and stats[1]: wave sum, then one atomic per workgroup.  Every
// thread of the workgroup calls it.
__device__ __forceinline__ void block_add_counts(unsigned long long c0, unsigned long long c1, unsigned long long *stats) {
  for (int o = 32; o > 0; o >>= 1) {
    c0 += __shfl_xor(c0, o);
    c1 += __shfl_xor(c1, o);
  }
  __shared__ unsigned long long red[2];
  if (threadIdx.x == 0) red[0] = red[1] = 0;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&red[0], c0);
    atomicAdd(&red[1], c1);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    atomicAdd(&stats[0], red[0]);
    atomicAdd(&stats[1], red[1]);
  }
}

// calls f(std::integral_constant<int, CPL>) for the smallest instantiated CPL (columns per lane) >= cpl, cpl <= 16
template <typename F> void for_columns_per_lane(int cpl, F f) {
  if (cpl <= 1) f(std::integral_constant<int, 1>{});
  else if (cpl <= 2) f(std::integral_constant<int, 2>{});
  else if (cpl <= 3) f(std::integral_constant<int, 3>{});
  else if (cpl <= 4) f(std::integral_constant<int, 4>{});
  else if (cpl <= 6) f(std::integral_constant<int, 6>{});
  else if (cpl <= 8) f(std::integral_constant<int, 8>{});
  else if (cpl <= 12) f(std::integral_constant<int, 12>{});
  else f(std::integral_constant<int, 16>{});
}

// Samples in flight: at most min(users, items) / 16 (at least 16).  Hogwild needs concurrent samples to collide rarely; on a
// small matrix a full device of samples (32 K groups) would overwrite each row's updates dozens of times per round and the
// model stops learning.  From about 500 K rows on, the device is full anyway.
inline int64_t hogwild_in_flight(int64_t samples, size_t users, size_t items) {
  return std::min<int64_t>(samples, std::max<int64_t>(16, (int64_t)std::min(users, items) / 16));
}

// bpr.hip.  Lanes per sample for C columns: the narrowest group that keeps a row in at most 8 registers per lane.
int bpr_group(int C);
// bpr.hip.  The id pre-pass: 0 <= userids < x_rows, 0 <= itemids < y_rows, 0 <= indptr <= nnz, checked on the device before
// an update kernel turns them into addresses.  `bad` is a zeroed device word; throws out_of_range_error naming `who` (the
// entry point maps it to IMP_OUT_OF_RANGE) with nothing else launched.  `prof`: the profiler scope of the check kernel.
// Synchronises the library stream.
void check_pair_ids(const char *who, const char *prof, const imp_intvector *userids, const imp_intvector *itemids,
                    const imp_intvector *indptr, size_t x_rows, size_t y_rows, unsigned long long *bad);

}  // namespace imp
#endif  // IMPLICIT_AMD_CSRC_PAIR_SGD_H_
