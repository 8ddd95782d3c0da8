// What the three SGD trainers (bpr.hip, warp.hip, lmf.hip) have in common.  On the device: the lane-group layout of a row -- a
// group of G = 16 / 32 / 64 lanes per sample or row, lane l owning columns l, l + G, ... in CPL registers -- with its loads,
// stores and dot product, the G-ary membership search of a sorted CSR row and the count reduction.  On the host: the rule for
// G, the dispatch from a run-time (G, C) to a compiled (G, CPL), the cap on samples in flight, and the declarations of the
// pairwise entry points' shared body (pair_sgd.hip).
#ifndef IMPLICIT_AMD_CSRC_SGD_GROUP_H_
#define IMPLICIT_AMD_CSRC_SGD_GROUP_H_
#include <algorithm>
#include <functional>
#include <stdexcept>
#include <type_traits>

#include "common.h"
#include "wave_ops.h"

namespace imp {

// the lanes of the aligned group of G = 16 / 32 / 64 that `lane` belongs to, as a ballot mask
template <int G> __device__ __forceinline__ uint64_t group_mask(int lane) {
  return G == 64 ? ~0ull : ((1ull << G) - 1) << (lane & ~(G - 1));
}

// A thread's place in the layout, built once at the top of a kernel: `const LaneGroup<G> g;`.  blockDim.x is a default
// argument so that it is read in the kernel itself, where the compiler takes every workgroup to be full; read inside a device
// function it comes with the code for a partial last workgroup (7 more instructions per kernel, measured on the code objects).
template <int G> struct LaneGroup {
  int gl;           // lane inside the group
  uint64_t gmask;   // the group's lanes as a ballot mask
  int64_t index;    // the group's index in the grid: its first sample or row
  int64_t ngroups;  // groups in the grid: the stride to its next one
  __device__ __forceinline__ LaneGroup(unsigned block = blockDim.x) {
    const int lane = threadIdx.x & 63;
    gl = lane & (G - 1);
    gmask = group_mask<G>(lane);
    index = ((int64_t)blockIdx.x * block + threadIdx.x) / G;
    ngroups = (int64_t)gridDim.x * (block / G);
  }
};

// v = the lane's columns gl, gl + G, ... of a C-wide row, 0 past its end
template <int G, int CPL>
__device__ __forceinline__ void group_load(const float *row, int C, int gl, float (&v)[CPL]) {
#pragma unroll
  for (int k = 0; k < CPL; ++k) {
    const int c = gl + G * k;
    v[k] = c < C ? row[c] : 0.f;
  }
}

// the lane's columns of a C-wide row = v
template <int G, int CPL>
__device__ __forceinline__ void group_store(float *row, int C, int gl, const float (&v)[CPL]) {
#pragma unroll
  for (int k = 0; k < CPL; ++k)
    if (gl + G * k < C) row[gl + G * k] = v[k];
}

// The dot product of two rows held as above, bitwise the same in every lane of the group (wave_ops.h group_allsum).  Every
// lane of the group must be active.
template <int G, int CPL> __device__ __forceinline__ float group_dot(const float (&a)[CPL], const float (&b)[CPL]) {
  return group_allsum<G>(dot_local(a, b));
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

// ---- host: lanes per row, columns per lane ---------------------------------------------------------------------------------
// Lanes per row for C columns: the narrowest group that keeps a row in at most 8 registers per lane (more rows per wave in
// flight).  LMF takes this rule as it stands.
constexpr int group_lanes(int C) { return C <= 128 ? 16 : C <= 256 ? 32 : 64; }
// pair_sgd.hip.  The same for the pairwise kernels: IMP_BPR_LANES=16/32/64, read per call, overrides the rule for measurement
// where C <= 16 x lanes.
int pair_group_lanes(int C);

// the smallest instantiated CPL (columns per lane) >= cpl, cpl <= 16
constexpr int columns_per_lane(int cpl) {
  for (int v : {1, 2, 3, 4, 6, 8, 12})
    if (cpl <= v) return v;
  return 16;
}

// whether group_lanes alone picks (G, CPL) for some C up to 1024: 12 of the 24 pairs
constexpr bool rule_reaches(int G, int CPL) {
  for (int C = 1; C <= 1024; ++C)
    if (group_lanes(C) == G && columns_per_lane((C + G - 1) / G) == CPL) return true;
  return false;
}

template <bool kRuleOnly, int G, typename F> void for_columns_per_lane(int C, F f) {
  const int cpl = columns_per_lane((C + G - 1) / G);
  bool found = false;
  auto at = [&](auto c) {
    if constexpr (!kRuleOnly || rule_reaches(G, decltype(c)::value)) {
      if (cpl == decltype(c)::value) f(std::integral_constant<int, G>{}, c), found = true;
    }
  };
  at(std::integral_constant<int, 1>{}), at(std::integral_constant<int, 2>{}), at(std::integral_constant<int, 3>{});
  at(std::integral_constant<int, 4>{}), at(std::integral_constant<int, 6>{}), at(std::integral_constant<int, 8>{});
  at(std::integral_constant<int, 12>{}), at(std::integral_constant<int, 16>{});
  if (!found) throw std::logic_error("no kernel is compiled for this (lanes, columns per lane)");
}

// Calls f(std::integral_constant<int, G>, std::integral_constant<int, CPL>) for a group of G = 16 / 32 / 64 lanes over C <=
// 16 G columns.  kRuleOnly: the caller's G is group_lanes(C), and f is instantiated for the 12 pairs that rule reaches only.
template <bool kRuleOnly, typename F> void for_group_shape(int G, int C, F f) {
  if (G == 16) for_columns_per_lane<kRuleOnly, 16>(C, f);
  else if (G == 32) for_columns_per_lane<kRuleOnly, 32>(C, f);
  else for_columns_per_lane<kRuleOnly, 64>(C, f);
}

// Samples in flight: at most min(users, items) / 16 (at least 16).  Hogwild needs concurrent samples to collide rarely; on a
// small matrix a full device of samples (32 K groups) would overwrite each row's updates dozens of times per round and the
// model stops learning.  From about 500 K rows on, the device is full anyway.
inline int64_t hogwild_in_flight(int64_t samples, size_t users, size_t items) {
  return std::min<int64_t>(samples, std::max<int64_t>(16, (int64_t)std::min(users, items) / 16));
}

// ---- host: the pairwise entry points (pair_sgd.hip) ------------------------------------------------------------------------
// The id pre-pass: 0 <= userids < x_rows, 0 <= itemids < y_rows, 0 <= indptr <= nnz, checked on the device before an update
// kernel turns them into addresses.  `bad` is a zeroed device word; throws out_of_range_error naming `who` (the entry point
// maps it to IMP_OUT_OF_RANGE) with nothing else launched.  `prof`: the profiler scope of the check kernel.  Synchronises the
// library stream.
void check_pair_ids(const char *who, const char *prof, const imp_intvector *userids, const imp_intvector *itemids,
                    const imp_intvector *indptr, size_t x_rows, size_t y_rows, unsigned long long *bad);

// The body imp_bpr_update and imp_warp_update share, inside guarded(): the argument checks (messages start with `who`), zeroed
// counts and an early return on nnz == 0 or no samples, the pre-pass, the write notes on X and Y, then launch(G, grid, samples,
// stats) under the profiler scope `prof` -- G from pair_group_lanes, the grid from hogwild_in_flight, stats two zeroed device
// counters -- and the read-back of the two counters into *count0 and *count1.  Synchronous.
using PairLaunch = std::function<void(int G, int grid, int64_t samples, unsigned long long *stats)>;
void pair_update(const char *who, const char *check_prof, const char *prof, const imp_intvector *userids,
                 const imp_intvector *itemids, const imp_intvector *indptr, imp_matrix *X, imp_matrix *Y, int64_t samples,
                 int64_t *count0, int64_t *count1, const PairLaunch &launch);

}  // namespace imp
#endif  // IMPLICIT_AMD_CSRC_SGD_GROUP_H_
