// K14: scores and ranks per-query candidate lists.  NEW: the reference dropped its rank_items; here it is the
// second stage of a retrieve-then-rank pipeline, one launch per chunk of rows.
//
// Row r of `query` is scored against candidates[offsets[r] .. offsets[r + 1]) of `items`.  One workgroup per row:
//   1. scores   one wavefront per candidate, kRankUnroll candidates in flight: lane l takes columns l, l + 64, ... in order with
//               fmaf, then the fixed DPP tree of wave_allsum.  The instruction sequence depends on the width alone, so the same
//               (query row bits, item row bits) give the same score bits in every list, row, chunk, mode and path.  fp16 operands
//               are widened exactly.  Column loads are 4 (2) bytes per lane, 256 (128) bytes per wavefront: no alignment is asked
//               of a row, widths 33 and 34 included.
//   2. filter   one thread per candidate: binary search of the id in the query's liked row (strictly increasing); a hit scores
//               -FLT_MAX and stays in the list, the rule of recommend().
//   3. order    (n >= 1) a list of <= kRankLdsKeys candidates keeps its keys in the LDS and is sorted there (bitonic network: a list
//               may repeat an id, and the counting sort of select_ops.h wants distinct keys).  A longer list writes its keys to a
//               device scratch, finds its n-th largest key by the byte-wise radix select over the 64-bit keys, gathers the keys
//               above it and as many of the keys equal to it as are still wanted, and sorts those in the LDS.  Equal keys are
//               equal bytes, so the output is unique either way.
// n == 0: the scores go out in the candidates' own order and step 3 does not run.  No floating-point atomic anywhere.
#include <hip/hip_fp16.h>

#include <algorithm>
#include <cfloat>

#include "common.h"
#include "select_ops.h"
#include "wave_ops.h"

namespace imp {

constexpr int kRankBlock = 512;
constexpr int kRankWaves = kRankBlock / 64;
constexpr int kRankUnroll = 4;        // candidate rows a wavefront has in flight
constexpr int kRankLdsKeys = 4096;    // longest list sorted whole in the LDS (32 KB of keys)
constexpr int kRankMaxSelect = 1024;  // largest n of a longer list (the winners are sorted in the LDS)

__device__ __forceinline__ float rank_widen(float v) { return v; }
__device__ __forceinline__ float rank_widen(__half v) { return __half2float(v); }

static int pow2_at_least(int n) {
  int p = 2;
  while (p < n) p <<= 1;
  return p;
}
static size_t rank_lds_bytes(int lds_keys) { return (size_t)lds_keys * sizeof(uint64_t) + (256 + 8) * sizeof(unsigned int); }

// offsets / liked_indptr hold the chunk's rows + 1 entries, relative to the chunk's first candidate / liked index; query points at
// the chunk's first row.  lds_keys: a power of two >= every list of <= kRankLdsKeys entries and, when a longer one exists, >= n.
template <typename TI, typename TQ>
__global__ __launch_bounds__(kRankBlock) void rank_kernel(const TI *__restrict__ items, int w, const TQ *__restrict__ query,
                                                          const int64_t *__restrict__ offsets, const int32_t *__restrict__ cand,
                                                          const int64_t *__restrict__ liked_indptr,
                                                          const int32_t *__restrict__ liked_indices, int n, int lds_keys,
                                                          uint64_t *scratch, int32_t *__restrict__ ids_out, float *scores_out) {
  extern __shared__ __attribute__((aligned(16))) uint64_t lds_keys_base[];
  uint64_t *lkeys = lds_keys_base;                                       // [lds_keys]
  unsigned int *hist = reinterpret_cast<unsigned int *>(lkeys + lds_keys);  // [256]
  unsigned int *words = hist + 256;                                      // bucket, remaining, bucket count, gathered, equal seen
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t r = blockIdx.x;
  const int64_t begin = offsets[r];
  const int len = (int)(offsets[r + 1] - begin);
  const int32_t *c = cand + begin;
  const TQ *q = query + r * (size_t)w;
  const bool in_lds = len <= kRankLdsKeys;
  uint64_t *keys = n > 0 ? (in_lds ? lkeys : scratch + begin) : nullptr;
  float *srow = scores_out + begin;  // score mode

  // ---- 1. scores ---------------------------------------------------------------------------------------------------------------
  for (int e0 = wave * kRankUnroll; e0 < len; e0 += kRankWaves * kRankUnroll) {
    int id[kRankUnroll];
    float acc[kRankUnroll];
#pragma unroll
    for (int u = 0; u < kRankUnroll; ++u) {
      id[u] = c[min(e0 + u, len - 1)];  // past the end: a valid row, scored and dropped
      acc[u] = 0.f;
    }
    for (int i0 = 0; i0 < w; i0 += 64) {
      const int i = i0 + lane;
      if (i < w) {
        const float qv = rank_widen(q[i]);
#pragma unroll
        for (int u = 0; u < kRankUnroll; ++u) acc[u] = fmaf(qv, rank_widen(items[(size_t)id[u] * w + i]), acc[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < kRankUnroll; ++u) {
      const float s = wave_allsum(acc[u]);
      if (lane == 0 && e0 + u < len) {
        if (n > 0) keys[e0 + u] = make_key(s, id[u]);
        else srow[e0 + u] = s;
      }
    }
  }
  __syncthreads();

  // ---- 2. liked filter -----------------------------------------------------------------------------------------------------------
  if (liked_indptr) {
    const int64_t lbegin = liked_indptr[r], lend = liked_indptr[r + 1];
    if (lend > lbegin) {
      for (int e = tid; e < len; e += kRankBlock) {
        const int32_t id = c[e];
        int64_t lo = lbegin, hi = lend;  // first index >= id
        while (lo < hi) {
          const int64_t mid = lo + ((hi - lo) >> 1);
          if (liked_indices[mid] < id) lo = mid + 1;
          else hi = mid;
        }
        if (lo < lend && liked_indices[lo] == id) {
          if (n > 0) keys[e] = make_key(-FLT_MAX, id);
          else srow[e] = -FLT_MAX;
        }
      }
    }
    __syncthreads();
  }
  if (n <= 0) return;

  // ---- 3. order --------------------------------------------------------------------------------------------------------------------
  int count = len;  // keys in lkeys[0 .. count)
  if (!in_lds) {
    uint64_t prefix = 0, mask = 0;
    unsigned int remaining = (unsigned int)n;  // n <= kRankMaxSelect < len
    auto each_key = [&](auto &&body) {
      for (int e = tid; e < len; e += kRankBlock) body(keys[e]);
    };
    for (int shift = 56; shift >= 0; shift -= 8)
      if (radix_select_digit<kRankBlock, uint64_t>(each_key, shift, prefix, mask, remaining, hist, &words[0], &words[1], &words[2]))
        break;
    // (key & mask) > prefix: n - remaining keys, all winners; == prefix: the boundary bucket, of which `remaining` are wanted (all
    // of it when the select stopped early; after the last digit its keys are equal, so whichever are taken are the same bytes)
    if (tid == 0) words[3] = 0, words[4] = 0;
    __syncthreads();
    for (int e = tid; e < len; e += kRankBlock) {
      const uint64_t key = keys[e], head = key & mask;
      bool take = head > prefix;
      if (head == prefix) take = atomicAdd(&words[4], 1u) < remaining;
      if (take) {
        const unsigned int slot = atomicAdd(&words[3], 1u);
        if (slot < (unsigned int)lds_keys) lkeys[slot] = key;
      }
    }
    __syncthreads();
    count = n;
  }
  int np2 = 2;
  while (np2 < count) np2 <<= 1;
  for (int e = count + tid; e < np2; e += kRankBlock) lkeys[e] = 0;  // below every key that is sorted with it or equal to it
  __syncthreads();
  block_sort_desc<kRankBlock>(lkeys, np2);
  const int written = min(n, count);
  int32_t *ids_r = ids_out + r * (size_t)n;
  float *scores_r = scores_out + r * (size_t)n;
  for (int j = tid; j < n; j += kRankBlock) {
    ids_r[j] = j < written ? key_id(lkeys[j]) : -1;
    scores_r[j] = j < written ? key_score(lkeys[j]) : -FLT_MAX;
  }
}

struct RankCall {
  const imp_matrix *items, *query;
  const int64_t *offsets;
  const int32_t *candidates;
  int n;
  const int64_t *liked_indptr;
  const int32_t *liked_indices;
  int32_t *indices;
  float *scores;
  bool any_long;  // some list is longer than kRankLdsKeys: the chunk carries a key scratch
  int lds_keys;
};

// device bytes of one row's share of a chunk
static size_t rank_row_bytes(const RankCall &c, size_t r) {
  const size_t len = (size_t)(c.offsets[r + 1] - c.offsets[r]);
  size_t b = len * sizeof(int32_t) + 2 * sizeof(int64_t);
  if (c.n > 0) b += (size_t)c.n * (sizeof(int32_t) + sizeof(float)) + (c.any_long ? len * sizeof(uint64_t) : 0);
  else b += len * sizeof(float);
  if (c.liked_indptr) b += (size_t)(c.liked_indptr[r + 1] - c.liked_indptr[r]) * sizeof(int32_t) + sizeof(int64_t);
  return b;
}

template <typename TI, typename TQ> static void rank_chunk(const RankCall &c, size_t r0, size_t r1) {
  const size_t rows = r1 - r0, w = c.items->cols;
  const int64_t c0 = c.offsets[r0], nc = c.offsets[r1] - c0;
  std::vector<int64_t> h_off(rows + 1), h_lptr;
  for (size_t r = 0; r <= rows; ++r) h_off[r] = c.offsets[r0 + r] - c0;
  DeviceArray<int64_t> d_off, d_lptr;
  DeviceArray<int32_t> d_cand, d_lidx, d_ids;
  DeviceArray<uint64_t> d_scratch;
  DeviceArray<float> d_scores;
  d_off.upload(h_off.data(), rows + 1);
  d_cand.upload(c.candidates + c0, (size_t)nc);
  if (c.liked_indptr) {
    const int64_t l0 = c.liked_indptr[r0], nl = c.liked_indptr[r1] - l0;
    h_lptr.resize(rows + 1);
    for (size_t r = 0; r <= rows; ++r) h_lptr[r] = c.liked_indptr[r0 + r] - l0;
    d_lptr.upload(h_lptr.data(), rows + 1);
    d_lidx.upload(c.liked_indices + l0, (size_t)nl);
  }
  const size_t out = c.n > 0 ? rows * (size_t)c.n : (size_t)nc;
  d_scores.alloc(out);
  if (c.n > 0) d_ids.alloc(out);
  if (c.n > 0 && c.any_long) d_scratch.alloc((size_t)nc);
  const size_t lds = rank_lds_bytes(c.lds_keys);
  const TQ *q = c.query->as<TQ>() + r0 * w;
  {
    IMP_PROF("rank");
    rank_kernel<TI, TQ><<<(unsigned int)rows, kRankBlock, lds, stream()>>>(
        c.items->as<TI>(), (int)w, q, d_off.data(), d_cand.data(), c.liked_indptr ? d_lptr.data() : nullptr,
        d_lidx.data(), c.n, c.lds_keys, d_scratch.data(), d_ids.data(), d_scores.data());
    IMP_CHECK_HIP(hipGetLastError());
  }
  if (c.n > 0) {
    IMP_CHECK_HIP(hipMemcpyAsync(c.indices + r0 * (size_t)c.n, d_ids.data(), out * sizeof(int32_t), hipMemcpyDeviceToHost, stream()));
    IMP_CHECK_HIP(hipMemcpyAsync(c.scores + r0 * (size_t)c.n, d_scores.data(), out * sizeof(float), hipMemcpyDeviceToHost, stream()));
  } else if (out) {
    IMP_CHECK_HIP(hipMemcpyAsync(c.scores + c0, d_scores.data(), out * sizeof(float), hipMemcpyDeviceToHost, stream()));
  }
  sync();  // the host vectors and device arrays of the chunk die here
}

template <typename TI, typename TQ> static void rank_rows(const RankCall &c, size_t budget) {
  const size_t rows = c.query->rows;
  for (size_t r0 = 0; r0 < rows;) {  // greedy chunks of whole rows; every row fits (checked by the caller)
    size_t r1 = r0, bytes = 0;
    while (r1 < rows && r1 - r0 < (size_t)INT32_MAX) {
      const size_t b = rank_row_bytes(c, r1);
      if (r1 > r0 && bytes + b > budget) break;
      bytes += b, ++r1;
    }
    rank_chunk<TI, TQ>(c, r0, r1);
    r0 = r1;
  }
}

}  // namespace imp

using namespace imp;

extern "C" int imp_knn_rank(imp_knn *knn, const imp_matrix *items, const imp_matrix *query, const int64_t *offsets,
                            const int32_t *candidates, int n, const int64_t *liked_indptr, const int32_t *liked_indices,
                            int32_t *indices, float *scores) {
  return guarded([&] {
    if (query->cols != items->cols) throw std::invalid_argument("rank: items and query must have the same number of columns");
    if (items->cols < 1 || items->cols > (size_t)INT32_MAX) throw std::invalid_argument("rank: a matrix needs at least one column");
    if ((items->itemsize != 4 && items->itemsize != 2) || (query->itemsize != 4 && query->itemsize != 2))
      throw std::invalid_argument("rank: items and query must be float32 or float16");
    if (n < 0) throw std::invalid_argument("rank: n must be >= 0");
    if (items->rows > (size_t)INT32_MAX) throw std::invalid_argument("rank: too many items");
    if ((liked_indptr == nullptr) != (liked_indices == nullptr))
      throw std::invalid_argument("rank: liked_indptr and liked_indices go together");
    const size_t rows = query->rows;
    if (rows == 0) return;
    if (offsets[0] != 0) throw std::invalid_argument("rank: offsets must start at 0");
    int64_t longest = 0, longest_short = 0;
    for (size_t r = 0; r < rows; ++r) {
      const int64_t len = offsets[r + 1] - offsets[r];
      if (len < 0) throw std::invalid_argument("rank: offsets decrease at row " + std::to_string(r));
      if (len > (int64_t)INT32_MAX) throw std::invalid_argument("rank: the list of row " + std::to_string(r) + " is too long");
      longest = std::max(longest, len);
      if (len <= kRankLdsKeys) longest_short = std::max(longest_short, len);
    }
    const int64_t total = offsets[rows];
    for (int64_t e = 0; e < total; ++e)
      if (candidates[e] < 0 || (size_t)candidates[e] >= items->rows)
        throw std::invalid_argument("rank: candidate id " + std::to_string(candidates[e]) + " (position " + std::to_string(e) +
                                    ") is outside the item factors (" + std::to_string(items->rows) + " rows)");
    if (liked_indptr) {
      if (liked_indptr[0] != 0) throw std::invalid_argument("rank: liked_indptr must start at 0");
      for (size_t r = 0; r < rows; ++r) {
        if (liked_indptr[r + 1] < liked_indptr[r]) throw std::invalid_argument("rank: liked_indptr decreases at row " + std::to_string(r));
        for (int64_t e = liked_indptr[r] + 1; e < liked_indptr[r + 1]; ++e)
          if (liked_indices[e] <= liked_indices[e - 1])
            throw std::invalid_argument("rank: the liked row " + std::to_string(r) + " is not strictly increasing");
      }
    }
    const bool any_long = n > 0 && longest > kRankLdsKeys;
    if (any_long && n > kRankMaxSelect)
      throw std::invalid_argument("rank: a list of more than " + std::to_string(kRankLdsKeys) + " candidates (" + std::to_string(longest) +
                                  ") is ranked for n <= " + std::to_string(kRankMaxSelect) + " only, got n = " + std::to_string(n));
    const int lds_keys = std::max(pow2_at_least((int)longest_short), any_long ? pow2_at_least(n) : 2);
    const RankCall c{items, query, offsets, candidates, n, liked_indptr, liked_indices, indices, scores, any_long, lds_keys};
    const size_t budget = knn_temp_budget(knn);
    for (size_t r = 0; r < rows; ++r) {
      const size_t need = rank_row_bytes(c, r);
      if (need > budget)
        throw std::invalid_argument("rank: row " + std::to_string(r) + " alone needs " + std::to_string(need) +
                                    " bytes of temporaries, max_temp_memory is " + std::to_string(budget));
    }
    const bool ih = items->itemsize == 2, qh = query->itemsize == 2;
    if (ih) qh ? rank_rows<__half, __half>(c, budget) : rank_rows<__half, float>(c, budget);
    else qh ? rank_rows<float, __half>(c, budget) : rank_rows<float, float>(c, budget);
  });
}
