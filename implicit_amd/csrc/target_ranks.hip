// K24: the rank of held-out items among everything a user could be recommended (imp_knn_target_ranks).
//
// No reference counterpart: the reference scores a top-K list on the host (evaluation.pyx) and cannot say where an item below
// position K stands.  Y (items x C) and Q (rows x C) are float32, 2 <= C <= 1024 (a bias column is a column like any other).
// Row u has the targets targets[offsets[u] .. offsets[u + 1]), strictly increasing ids; the exclusion of the call is the device
// COO (row, col) pattern top-k queries take (an entry outside the batch or the catalogue excludes nothing).  With s(u, j) the
// fp32 score of the tile routine below and C_u the items not excluded for row u, a target t in C_u gets
//     rank(u, t) = #{ j in C_u, j != t : s(u, j) > s(u, t)  or  (s(u, j) == s(u, t) and j < t) }
// (-0.0 as +0.0), a target outside C_u gets -1, and candidates[u] = |C_u|.  A NaN score is not defined.
//
// s(u, j) is ONE function of the pair: every score of the call comes from score_tile -- 32 query rows against 128 item rows,
// v_mfma_f32_32x32x2_f32 (exact fp32 products, the instruction of svd.hip, spd_inverse.hip and softmax_mf.hip), one accumulator
// element per pair, the columns taken two at a time in ascending order, zero columns up to the next multiple of 32.  What
// the other 31 rows and 127 items of the tile hold never enters the element, so the target pass (item rows gathered by id)
// and the dense pass (item rows in catalogue order) produce the same bits for the same pair, whatever tile it falls into.
//
// Four launches per chunk of query rows (a chunk's exclusion bitmap, rows x ceil(items / 32) words, fits the handle's budget):
//   bits        the COO entries of the chunk's rows set their bits (atomic or; a repeated entry is harmless);
//   thresholds  a workgroup per tile of 32 query rows runs score_tile over its rows' targets, 128 gathered item rows a step --
//               they are consecutive in `targets` -- and writes each target's key: ordered(score) << 32 | ~id, so a larger
//               key is a better place under the tie rule; 0 for an excluded target.  Its rank is preset to -1;
//   sort        a workgroup per row sorts the row's keys descending (bitonic: in the LDS up to 2048 keys, in place in global
//               memory beyond), counts the valid ones (the zeros sort last) and clears the row's bins;
//   dense       workgroup (tile of 32 rows, split s) keeps the tile's Q columns in the LDS (a panel of up to 512; a wider Q is
//               re-read panel by panel), its rows' sorted keys and bins too where a row has at most 64 valid targets, and
//               strides over the 128-item tiles s, s + splits, ...: Y streams through the LDS in slices of 32 columns
//               (leading dimension 33), one 32 x 32 accumulator tile per wavefront.  The epilogue never stores a score: each
//               accumulator element that is a candidate (in range, bit clear) finds p = #{keys of its row >= its key} by a
//               branch-free binary search and increments bin p of its row -- LDS atomics, or global ones for a row of more
//               than 64 targets.  A target meets its own key there and lands one bin below itself, so it never counts for
//               itself.  At the end the LDS bins are added to the row's global bins;
//   finish      a workgroup per row: the prefix sum of the bins -- rank of the q-th best target = bins[0] + .. + bins[q] --
//               written to the target's place (its id is in the key, its place found by binary search), and |C_u| = items -
//               the row's set bits.
// Counts are integers: the atomics make the result independent of any order.  Rows without valid targets cost the dense pass
// nothing (a tile of such rows returns at once).  Every item id that becomes an address is < items by construction (dense
// pass) or was checked on the host before anything is launched (targets); the COO entries are checked where they are read.
#include <algorithm>
#include <string>
#include <vector>

#include "common.h"
#include "select_ops.h"

namespace imp {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kRows = 32;         // query rows of a tile
constexpr int kItems = 128;       // item rows of a step: 32 per wavefront
constexpr int kSlice = 32;        // columns per slice of Y
constexpr int kLd = kSlice + 1;   // leading dimension of the slice
constexpr int kPanel = 512;       // columns of Q held in the LDS
constexpr int kBinCap = 64;       // valid targets of a row whose keys and bins live in the LDS
constexpr int kSortLds = 2048;    // keys of a row sorted in the LDS
constexpr int kBlock = 256;

struct RankArgs {
  const float *__restrict__ Y, *__restrict__ Q;  // Q: the chunk's first row
  int C, items, rows;                            // rows of the chunk
  const int64_t *__restrict__ offsets;           // [rows + 1] targets of the chunk's rows, relative to `targets`
  const int32_t *__restrict__ targets;
  const int64_t *__restrict__ koff;              // [rows + 1] first key slot of a row: power-of-two capacities
  uint64_t *keys;
  int32_t *nvalid;                               // [rows] valid targets = sorted keys in front
  int32_t *bins;                                 // row r: bins + koff[r] + r, nvalid[r] + 1 in use
  const uint32_t *bits;                          // exclusion bitmap rows x words, or null
  int words;
  int32_t *ranks, *candidates;
};

__device__ __forceinline__ int panel_ld(int C) { return min((C + kSlice - 1) / kSlice * kSlice, kPanel) + 1; }
size_t q_lds_floats(int C) { return (size_t)kRows * (std::min((C + kSlice - 1) / kSlice * kSlice, kPanel) + 1); }

// row of element e of a lane's 32 x 32 accumulator; its column is lane & 31
__device__ __forceinline__ int tile_row(int e, int lane) { return (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5); }
__device__ __forceinline__ bool excluded(const RankArgs &a, int r, int id) {
  return a.bits && ((a.bits[(size_t)r * a.words + (id >> 5)] >> (id & 31)) & 1u);
}
__device__ __forceinline__ uint64_t rank_key(float s, int id) { return make_key(s, ~id); }

// The one definition of a score.  acc[e] = Q[r0 + tile_row(e, lane)] . Y[sid[32 wave + (lane & 31)]]; sid (LDS, 128 ids, -1: a
// zero row) must be behind a barrier.  Qs holds a panel of the tile's rows; `q_ready` says it already holds panel 0 of a
// one-panel Q.  Called by all 256 threads; ends on a barrier.
__device__ __forceinline__ f32x16 score_tile(const RankArgs &a, int r0, const int *sid, float *Qs, float *Ys, bool &q_ready) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = tid & 31, slot = tid >> 5, l31 = lane & 31, lk = lane >> 5;
  const int C = a.C, ldq = panel_ld(C);
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  for (int p0 = 0; p0 < C; p0 += kPanel) {
    const int pc = min(kPanel, (C - p0 + kSlice - 1) / kSlice * kSlice);
    if (!q_ready) {
      for (int i = tid; i < kRows * pc; i += kBlock) {
        const int r = i / pc, c = i - r * pc;
        Qs[r * ldq + c] = (r0 + r < a.rows && p0 + c < C) ? a.Q[(size_t)(r0 + r) * C + p0 + c] : 0.f;
      }
      q_ready = C <= kPanel;
    }
    for (int c0 = 0; c0 < pc; c0 += kSlice) {
      const int c = p0 + c0 + col;
#pragma unroll 4
      for (int n = slot; n < kItems; n += kBlock / 32) {
        const int id = sid[n];
        Ys[n * kLd + col] = (id >= 0 && c < C) ? a.Y[(size_t)id * C + c] : 0.f;
      }
      __syncthreads();
      const float *qa = Qs + l31 * ldq + c0 + lk, *yb = Ys + (wave * 32 + l31) * kLd + lk;
#pragma unroll
      for (int ks = 0; ks < kSlice / 2; ++ks) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[2 * ks], yb[2 * ks], acc, 0, 0, 0);
      __syncthreads();  // the slice (and, past its last slice, the panel) has been consumed
    }
  }
  return acc;
}

__global__ __launch_bounds__(kBlock) void bits_kernel(const int32_t *__restrict__ row, const int32_t *__restrict__ col, size_t nnz,
                                                      int64_t row0, int rows, int items, int words, uint32_t *bits) {
  for (size_t e = blockIdx.x * (size_t)kBlock + threadIdx.x; e < nnz; e += (size_t)gridDim.x * kBlock) {
    const int64_t r = (int64_t)row[e] - row0;
    const int c = col[e];
    if (r >= 0 && r < rows && c >= 0 && c < items) atomicOr(&bits[(size_t)r * words + (c >> 5)], 1u << (c & 31));
  }
}

__global__ __launch_bounds__(kBlock) void thresholds_kernel(RankArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float *Qs = lds, *Ys = Qs + kRows * panel_ld(a.C);
  int *sid = reinterpret_cast<int *>(Ys + kItems * kLd);
  __shared__ int64_t off[kRows + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lk = lane >> 5;
  const int r0 = blockIdx.x * kRows;
  if (tid <= kRows) off[tid] = a.offsets[min(r0 + tid, a.rows)];
  __syncthreads();
  const int64_t tb = off[0], te = off[kRows];
  bool q_ready = false;
  for (int64_t t0 = tb; t0 < te; t0 += kItems) {
    if (tid < kItems) sid[tid] = t0 + tid < te ? a.targets[t0 + tid] : -1;
    __syncthreads();
    const f32x16 acc = score_tile(a, r0, sid, Qs, Ys, q_ready);
    const int n = wave * 32 + l31;
    const int64_t t = t0 + n;
    if (t < te) {
      int rl = 0;  // the row of the tile that holds entry t: the last one with off[rl] <= t
#pragma unroll
      for (int step = 16; step; step >>= 1) rl += (off[rl + step] <= t) ? step : 0;
      if (lk == ((rl >> 2) & 1)) {  // the lane of the pair that holds row rl, in element e
        const int e = (rl & 3) + 4 * (rl >> 3);
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) s = i == e ? acc[i] : s;
        const int r = r0 + rl, id = sid[n];
        a.keys[a.koff[r] + (t - off[rl])] = excluded(a, r, id) ? 0ull : rank_key(s, id);
        a.ranks[t] = -1;
      }
    }
    __syncthreads();  // sid is rewritten
  }
}

__global__ __launch_bounds__(kBlock) void sort_kernel(RankArgs a) {
  __shared__ uint64_t sk[kSortLds];
  __shared__ int count;
  const int tid = threadIdx.x, r = blockIdx.x;
  const int len = (int)(a.offsets[r + 1] - a.offsets[r]), cap = (int)(a.koff[r + 1] - a.koff[r]);
  uint64_t *K = a.keys + a.koff[r];
  if (tid == 0) count = 0;
  if (len == 0) {
    if (tid == 0) a.nvalid[r] = 0;
    return;
  }
  uint64_t *v = cap <= kSortLds ? sk : K;
  for (int i = tid; i < cap; i += kBlock) v[i] = i < len ? K[i] : 0ull;
  __syncthreads();
  block_sort_desc<kBlock>(v, cap);
  int mine = 0;
  for (int i = tid; i < cap; i += kBlock) {
    const uint64_t k = v[i];
    if (v != K) K[i] = k;
    mine += k != 0;
  }
  atomicAdd(&count, mine);
  int32_t *bins = a.bins + a.koff[r] + r;
  for (int i = tid; i <= len; i += kBlock) bins[i] = 0;
  __syncthreads();
  if (tid == 0) a.nvalid[r] = count;
}

__global__ __launch_bounds__(kBlock) void dense_kernel(RankArgs a, int splits) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  uint64_t *thr = reinterpret_cast<uint64_t *>(lds);                   // [kRows][kBinCap]
  int *lbins = reinterpret_cast<int *>(thr + kRows * kBinCap);         // [kRows][kBinCap + 1]
  int *sid = lbins + kRows * (kBinCap + 1), *snv = sid + kItems;       // [kItems], [kRows]
  float *Qs = reinterpret_cast<float *>(snv + kRows), *Ys = Qs + kRows * panel_ld(a.C);
  __shared__ int any;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31;
  const int r0 = blockIdx.x * kRows, split = blockIdx.y;
  if (tid == 0) any = 0;
  __syncthreads();
  if (tid < kRows) {
    const int nv = r0 + tid < a.rows ? a.nvalid[r0 + tid] : 0;
    snv[tid] = nv;
    if (nv) any = 1;
  }
  __syncthreads();
  if (!any) return;  // no row of the tile has a valid target
  for (int i = tid; i < kRows * kBinCap; i += kBlock) {
    const int rl = i / kBinCap, p = i - rl * kBinCap, nv = snv[rl];
    thr[i] = (nv <= kBinCap && p < nv) ? a.keys[a.koff[r0 + rl] + p] : 0ull;
  }
  for (int i = tid; i < kRows * (kBinCap + 1); i += kBlock) lbins[i] = 0;
  __syncthreads();

  bool q_ready = false;
  const int tiles = (a.items + kItems - 1) / kItems;
  for (int it = split; it < tiles; it += splits) {
    const int64_t base = (int64_t)it * kItems;
    if (tid < kItems) sid[tid] = base + tid < a.items ? (int)(base + tid) : -1;
    __syncthreads();
    const f32x16 acc = score_tile(a, r0, sid, Qs, Ys, q_ready);
    const int64_t j64 = base + wave * 32 + l31;
    if (j64 < a.items) {
      const int j = (int)j64;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int rl = tile_row(e, lane), nv = snv[rl], r = r0 + rl;
        if (nv == 0 || excluded(a, r, j)) continue;
        const uint64_t key = rank_key(acc[e], j);
        int pos = 0;  // #{keys of the row >= key}; the keys are sorted descending
        if (nv <= kBinCap) {
          const uint64_t *k = thr + rl * kBinCap;
#pragma unroll
          for (int step = kBinCap; step; step >>= 1) {
            const int idx = pos + step;
            pos = (idx <= nv && k[min(idx, kBinCap) - 1] >= key) ? idx : pos;
          }
          atomicAdd(&lbins[rl * (kBinCap + 1) + pos], 1);
        } else {
          const uint64_t *k = a.keys + a.koff[r];
          int step = 1;
          while (2 * step <= nv) step *= 2;
          for (; step; step >>= 1) {
            const int idx = pos + step;
            pos = (idx <= nv && k[min(idx, nv) - 1] >= key) ? idx : pos;
          }
          atomicAdd(&a.bins[a.koff[r] + r + pos], 1);
        }
      }
    }
    __syncthreads();  // sid is rewritten
  }
  for (int i = tid; i < kRows * (kBinCap + 1); i += kBlock) {
    const int rl = i / (kBinCap + 1), p = i - rl * (kBinCap + 1), nv = snv[rl], c = lbins[i];
    if (c && nv <= kBinCap && p <= nv) atomicAdd(&a.bins[a.koff[r0 + rl] + r0 + rl + p], c);
  }
}

__global__ __launch_bounds__(kBlock) void finish_kernel(RankArgs a) {
  __shared__ int wsum[kBlock / 64], carry, set_bits;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = blockIdx.x;
  if (tid == 0) carry = 0, set_bits = 0;
  __syncthreads();
  if (a.bits) {
    int mine = 0;
    for (int w = tid; w < a.words; w += kBlock) mine += __popc(a.bits[(size_t)r * a.words + w]);
    atomicAdd(&set_bits, mine);
  }
  __syncthreads();
  if (tid == 0) a.candidates[r] = a.items - set_bits;
  const int nv = a.nvalid[r];
  const int64_t tb = a.offsets[r];
  const int len = (int)(a.offsets[r + 1] - tb);
  const uint64_t *K = a.keys + a.koff[r];
  const int32_t *bins = a.bins + a.koff[r] + r;
  for (int q0 = 0; q0 < nv; q0 += kBlock) {  // uniform trip count
    const int q = q0 + tid;
    int v = q < nv ? bins[q] : 0;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {  // inclusive scan of the wavefront
      const int up = __shfl_up(v, d);
      v += lane >= d ? up : 0;
    }
    if (lane == 63) wsum[wave] = v;
    __syncthreads();
    int before = carry;
    for (int w = 0; w < wave; ++w) before += wsum[w];
    v += before;
    if (q < nv) {
      const int id = ~key_id(K[q]);
      int lo = 0, hi = len;  // the target's place in its row
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a.targets[tb + mid] < id) lo = mid + 1;
        else hi = mid;
      }
      if (lo < len) a.ranks[tb + lo] = v;
    }
    __syncthreads();
    if (tid == kBlock - 1) carry = v;
    __syncthreads();
  }
}

size_t dense_lds_bytes(int C) {
  return (size_t)kRows * kBinCap * 8 + ((size_t)kRows * (kBinCap + 1) + kItems + kRows) * 4 + (q_lds_floats(C) + (size_t)kItems * kLd) * 4;
}
size_t thresholds_lds_bytes(int C) { return (q_lds_floats(C) + (size_t)kItems * kLd + kItems) * 4; }

int64_t pow2_capacity(int64_t len) {
  if (len == 0) return 0;
  int64_t p = 2;
  while (p < len) p <<= 1;
  return p;
}

}  // namespace
}  // namespace imp

using namespace imp;

extern "C" int imp_knn_target_ranks(imp_knn *knn, const imp_matrix *items, const imp_matrix *query, const int64_t *offsets,
                                    const int32_t *targets, const imp_coo *query_filter, int32_t *ranks, int32_t *candidates) {
  return guarded([&] {
    const std::string w("target_ranks");
    if (!knn || !items || !query || !offsets || !candidates) throw std::invalid_argument(w + ": NULL argument");
    if (query->cols != items->cols) throw std::invalid_argument(w + ": items and query must have the same number of columns");
    if (items->cols < 2 || items->cols > 1024) throw std::invalid_argument(w + ": factor matrices need 2 .. 1024 columns");
    if (items->itemsize != 4 || query->itemsize != 4) throw std::invalid_argument(w + ": items and query must be float32");
    if (items->rows < 1 || items->rows > (size_t)INT32_MAX) throw std::invalid_argument(w + ": 1 .. 2^31 - 1 items");
    if (query->rows > (size_t)INT32_MAX) throw std::invalid_argument(w + ": more than 2^31 - 1 query rows");
    const size_t rows = query->rows;
    const int n_items = (int)items->rows, C = (int)items->cols;
    if (rows == 0) return;
    if (offsets[0] != 0) throw std::invalid_argument(w + ": offsets must start at 0");
    for (size_t r = 0; r < rows; ++r) {
      if (offsets[r + 1] < offsets[r]) throw std::invalid_argument(w + ": offsets decrease at row " + std::to_string(r));
      if (offsets[r + 1] - offsets[r] > n_items) throw std::invalid_argument(w + ": row " + std::to_string(r) + " has more targets than there are items");
    }
    const int64_t total = offsets[rows];
    if (total && (!targets || !ranks)) throw std::invalid_argument(w + ": NULL argument");
    for (size_t r = 0; r < rows; ++r)
      for (int64_t e = offsets[r]; e < offsets[r + 1]; ++e) {
        if (targets[e] < 0 || targets[e] >= n_items)
          throw out_of_range_error(w + ": target id " + std::to_string(targets[e]) + " (position " + std::to_string(e) +
                                   ") is outside the item factors (" + std::to_string(n_items) + " rows)");
        if (e > offsets[r] && targets[e] <= targets[e - 1])
          throw std::invalid_argument(w + ": the targets of row " + std::to_string(r) + " are not strictly increasing");
      }
    const imp_coo *qf = query_filter && query_filter->nnz ? query_filter : nullptr;

    // chunks of whole tiles whose bitmap takes at most half the budget
    const int words = (n_items + 31) / 32;
    size_t chunk = rows;
    if (qf) chunk = std::max<size_t>(kRows, knn_temp_budget(knn) / 2 / ((size_t)words * 4) / kRows * kRows);
    chunk = std::min<size_t>(chunk, (size_t)kRows << 20);

    DeviceArray<int32_t> d_targets, d_ranks;
    if (total) {
      d_targets.upload(targets, (size_t)total);
      d_ranks.alloc((size_t)total);
    }
    const size_t dense_lds = dense_lds_bytes(C), thr_lds = thresholds_lds_bytes(C);
    const int tiles = (n_items + kItems - 1) / kItems;
    for (size_t r0 = 0; r0 < rows; r0 += chunk) {
      const size_t n = std::min(chunk, rows - r0);
      std::vector<int64_t> h_off(n + 1), h_koff(n + 1);
      h_koff[0] = 0;
      for (size_t r = 0; r <= n; ++r) h_off[r] = offsets[r0 + r];
      for (size_t r = 0; r < n; ++r) h_koff[r + 1] = h_koff[r] + pow2_capacity(h_off[r + 1] - h_off[r]);
      DeviceArray<int64_t> d_off, d_koff;
      DeviceArray<uint64_t> d_keys;
      DeviceArray<int32_t> d_nvalid, d_bins, d_cand;
      DeviceArray<uint32_t> d_bits;
      d_off.upload(h_off.data(), n + 1);
      d_koff.upload(h_koff.data(), n + 1);
      d_keys.alloc((size_t)h_koff[n] + 1);
      d_bins.alloc((size_t)h_koff[n] + n + 1);
      d_nvalid.alloc(n);
      d_cand.alloc(n);
      if (qf) {
        IMP_PROF("target_filter_bits");
        d_bits.alloc(n * (size_t)words);
        IMP_CHECK_HIP(hipMemsetAsync(d_bits.data(), 0, n * (size_t)words * 4, stream()));
        const int grid = (int)std::min<size_t>(((size_t)qf->nnz + kBlock - 1) / kBlock, (size_t)ctx().num_cus * 8);
        bits_kernel<<<grid, kBlock, 0, stream()>>>(qf->row.data(), qf->col.data(), (size_t)qf->nnz, (int64_t)r0, (int)n, n_items, words, d_bits.data());
        IMP_CHECK_HIP(hipGetLastError());
      }
      const RankArgs a{items->f32(), query->f32() + r0 * (size_t)C, C, n_items, (int)n, d_off.data(), d_targets.data(), d_koff.data(),
                       d_keys.data(), d_nvalid.data(), d_bins.data(), qf ? d_bits.data() : nullptr, words, d_ranks.data(), d_cand.data()};
      const unsigned row_tiles = (unsigned)((n + kRows - 1) / kRows);
      if (h_off[n] > h_off[0]) {
        {
          IMP_PROF("target_thresholds");
          allow_dynamic_lds(thresholds_kernel, thr_lds);
          thresholds_kernel<<<row_tiles, kBlock, thr_lds, stream()>>>(a);
          IMP_CHECK_HIP(hipGetLastError());
        }
        {
          IMP_PROF("target_sort");
          sort_kernel<<<(unsigned)n, kBlock, 0, stream()>>>(a);
          IMP_CHECK_HIP(hipGetLastError());
        }
        {
          IMP_PROF("target_ranks_dense");
          // enough workgroups to fill the device four times over, never more splits than item tiles
          const int splits = (int)std::min<int64_t>({(int64_t)tiles, (int64_t)65535, std::max<int64_t>(1, ((int64_t)ctx().num_cus * 4 + row_tiles - 1) / row_tiles)});
          allow_dynamic_lds(dense_kernel, dense_lds);
          dense_kernel<<<dim3(row_tiles, (unsigned)splits), kBlock, dense_lds, stream()>>>(a, splits);
          IMP_CHECK_HIP(hipGetLastError());
        }
      } else {
        IMP_CHECK_HIP(hipMemsetAsync(d_nvalid.data(), 0, n * sizeof(int32_t), stream()));
      }
      {
        IMP_PROF("target_finish");
        finish_kernel<<<(unsigned)n, kBlock, 0, stream()>>>(a);
        IMP_CHECK_HIP(hipGetLastError());
      }
      IMP_CHECK_HIP(hipMemcpyAsync(candidates + r0, d_cand.data(), n * sizeof(int32_t), hipMemcpyDeviceToHost, stream()));
      sync();  // the host vectors and device arrays of the chunk die here
    }
    if (total) {
      IMP_CHECK_HIP(hipMemcpyAsync(ranks, d_ranks.data(), (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost, stream()));
      sync();
    }
  });
}
