// Selection primitives shared by the top-k kernels (topk.hip, topk_select.h, topk_resident.h) and the IVF index (ivf.hip):
// the score/id key, a descending sort of keys in LDS, and the byte-wise radix select.  Device-only, no state: every
// function works on LDS the caller owns and is called by ALL threads of a workgroup of BLOCK threads (uniformly).
//
// The key is ordered(score) << 32 | id: unsigned order of keys = (score descending, id descending) when read from the
// largest key down, which is the output order of the reference (implicit/cpu/topk.pyx:15-67 + select.h:12-40).  Ids are
// distinct within a row, so keys are, and any correct sort of them gives the same bytes.
#ifndef IMPLICIT_AMD_CSRC_SELECT_OPS_H_
#define IMPLICIT_AMD_CSRC_SELECT_OPS_H_
#include <hip/hip_runtime.h>

#include <cstdint>

namespace imp {

// ---- score/id key --------------------------------------------------------------------------------------------------------
// float -> uint32 whose unsigned order is the floats' order
__device__ __forceinline__ uint32_t ordered(float s) {
  uint32_t u = __float_as_uint(s);
  if (u == 0x80000000u) u = 0u;  // -0.0 compares equal to +0.0 in the reference's heap
  return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float unordered(uint32_t u) {
  return __uint_as_float(u ^ ((u >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}
__device__ __forceinline__ uint64_t make_key(float s, int id) { return ((uint64_t)ordered(s) << 32) | (uint32_t)id; }
__device__ __forceinline__ int32_t key_id(uint64_t key) { return (int32_t)(uint32_t)key; }
__device__ __forceinline__ float key_score(uint64_t key) { return unordered((uint32_t)(key >> 32)); }

// ---- sorts in LDS --------------------------------------------------------------------------------------------------------
// Bitonic network: v[0 .. n_pow2) descending.  The caller's writes to v must be behind a barrier; ends on a barrier.
template <int BLOCK> __device__ __forceinline__ void block_sort_desc(uint64_t *v, int n_pow2) {
  const int tid = threadIdx.x;
  for (int size = 2; size <= n_pow2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < (n_pow2 >> 1); t += BLOCK) {
        int lo = 2 * t - (t & (stride - 1));
        int hi = lo + stride;
        bool desc = ((lo & size) == 0);
        uint64_t a = v[lo], b = v[hi];
        if ((a < b) == desc) {
          v[lo] = b;
          v[hi] = a;
        }
      }
      __syncthreads();
    }
  }
}

// Sort by counting, for short lists of DISTINCT keys: in[i] goes to out[number of keys greater than it].  One barrier
// instead of the network's log^2 n, quadratic work.  `in` and `out` must not overlap; ends on a barrier.
template <int BLOCK> __device__ __forceinline__ void block_rank_sort(const uint64_t *in, uint64_t *out, int n) {
  for (int i = threadIdx.x; i < n; i += BLOCK) {
    const uint64_t key = in[i];
    int rank = 0;
    for (int j = 0; j < n; ++j) rank += in[j] > key;
    out[rank] = key;
  }
  __syncthreads();
}

// ---- radix select --------------------------------------------------------------------------------------------------------
// One digit (the byte at `shift`) of an MSB-first radix select of the remaining-th largest of the keys that match
// (key & mask) == prefix.  for_each_key(body) has the workgroup enumerate every key once, body(key) per key.  The 256 bins
// are zeroed and filled, thread 0 walks down from bin 255 to the boundary bucket -- the one the remaining-th largest key
// falls into -- and prefix, mask and remaining (now counted inside that bucket) are advanced in every thread.
// hist[256], sh_bucket, sh_remaining: LDS scratch.  With sh_count (one more LDS word, for callers that stop early) the
// return value tells whether the boundary bucket is taken whole, i.e. holds exactly the keys still wanted: (key & mask) >=
// prefix then selects exactly the wanted keys and no finer digit is needed.  (Thread 0 publishes the bucket's count beside the
// other two words: reading hist[bucket] afterwards would be a second, dependent LDS round trip per digit.)
template <int BLOCK, typename Key, typename ForEachKey>
__device__ __forceinline__ bool radix_select_digit(ForEachKey &&for_each_key, int shift, Key &prefix, Key &mask,
                                                   unsigned int &remaining, unsigned int *hist, unsigned int *sh_bucket,
                                                   unsigned int *sh_remaining, unsigned int *sh_count = nullptr) {
  const int tid = threadIdx.x;
  for (int i = tid; i < 256; i += BLOCK) hist[i] = 0;
  __syncthreads();
  for_each_key([&](Key key) {
    if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 0xFF], 1u);
  });
  __syncthreads();
  if (tid == 0) {
    unsigned int acc = 0;
    int b = 255;
    for (; b > 0; --b) {
      if (acc + hist[b] >= remaining) break;
      acc += hist[b];
    }
    *sh_bucket = b;
    *sh_remaining = remaining - acc;
    if (sh_count) *sh_count = hist[b];
  }
  __syncthreads();
  prefix |= (Key)*sh_bucket << shift;
  mask |= (Key)0xFF << shift;
  remaining = *sh_remaining;
  const bool whole = sh_count && *sh_count == remaining;
  __syncthreads();
  return whole;
}

// ordered key of the m-th largest of n values (the four digits of the 32-bit key; one workgroup)
template <int BLOCK>
__device__ __forceinline__ uint32_t kth_largest_key(const float *__restrict__ v, int n, unsigned int m, unsigned int *hist,
                                                    unsigned int *sh_bucket, unsigned int *sh_remaining) {
  uint32_t prefix = 0, mask = 0;
  unsigned int remaining = m;
  auto keys = [&](auto &&body) {
    for (int i = threadIdx.x; i < n; i += BLOCK) body(ordered(v[i]));
  };
  for (int digit = 3; digit >= 0; --digit)
    radix_select_digit<BLOCK, uint32_t>(keys, digit * 8, prefix, mask, remaining, hist, sh_bucket, sh_remaining);
  return prefix;
}

}  // namespace imp
#endif  // IMPLICIT_AMD_CSRC_SELECT_OPS_H_
