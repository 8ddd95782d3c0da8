// K13: explanations of ALS recommendations.  NEW on the GPU side: the reference explains on the CPU only
// (implicit/cpu/als.py explain / user_linear_weights), one user at a time, with a Python loop over the liked items.
//
// For user u with row (j, c_j):  A_u = YtY + reg I + sum_j (|c_j| - 1) y_j y_j^T = L L^T;  for item i  w = A_u^-1 y_i;  liked item j
// (c_j > 0) contributes s_j = c_j (w . y_j);  total = sum s_j (= y_i . x_u);  the answer is the N largest s_j under
// (score descending, item id descending).
//
// Two kernels, fp32 throughout, no matrix-core and no reduced-precision product:
//   explain_factor_kernel   one workgroup per user: A_u as 4 x 4 register blocks on the vector ALU (the A-build of the
//                           workgroup Cholesky kernel, als_cholesky.hip, without its augmented row), the packed lower triangle in
//                           the LDS, a left-looking column Cholesky (row i belongs to thread i, two barriers per column), L
//                           written as a dense f x f block with zeros above the diagonal.
//   explain_contrib_kernel  one workgroup per (user, item) pair: L staged into the LDS, both triangular solves by one wavefront,
//                           one wavefront per liked item for w . y_j, the contributions kept as sortable 64-bit keys (in the LDS
//                           up to kKeysLds entries, in a device workspace beyond), total by a fixed-order sum, the top N by
//                           counting ranks.  No floating-point atomic anywhere: the same call gives the same bits.
#include <algorithm>
#include <cfloat>

#include "common.h"
#include "wave_ops.h"

namespace imp {

constexpr int kExplainMaxF = 256;   // the packed triangle at f = 256 is 128.5 KB of the CU's 160 KiB
constexpr int kExplainTile = 8;     // gathered factor rows staged per step of the A-build
constexpr int kExplainBlocks = 4;   // 4 x 4 blocks a thread holds at a time: 1024 per round (f <= 176 in one round, f = 256 in three)
constexpr int kKeysLds = 2048;      // contributions of one pair kept in the LDS (16 KB); longer rows use the workspace
typedef unsigned long long key_t64;

__device__ __forceinline__ int tri_at(int i, int j) { return i * (i + 1) / 2 + j; }  // j <= i

static size_t tri_words(int f) { return ((size_t)f * (f + 1) / 2 + 3) & ~(size_t)3; }
static size_t factor_lds_bytes(int f) {
  const int FS = 4 * ((f + 3) / 4);
  return (tri_words(f) + 2 * (size_t)kExplainTile * FS + 4) * sizeof(float);
}
static size_t contrib_lds_bytes(int f) {
  const int FS = 4 * ((f + 3) / 4);
  return (size_t)kKeysLds * sizeof(key_t64) + (tri_words(f) + FS + 256 + 4) * sizeof(float);
}

// ---- factor kernel --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void explain_factor_kernel(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                             const float *__restrict__ data, int rows, const float *__restrict__ Y,
                                                             const float *__restrict__ YtY, int f, float reg, float *__restrict__ W,
                                                             unsigned long long *failed_row) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int nb = (f + 3) >> 2, FS = 4 * nb;  // 4 x 4 blocks per side, padded stride of a staged row
  float *A = smem;                             // packed lower triangle
  float *yt = A + (((size_t)f * (f + 1) / 2 + 3) & ~(size_t)3);  // [TILE][FS]  gathered rows, zero beyond f
  float *ut = yt + (size_t)kExplainTile * FS;  // [TILE][FS]  (|c| - 1) y
  int *flag = reinterpret_cast<int *>(ut + (size_t)kExplainTile * FS);
  const int tid = threadIdx.x;
  const int n_blocks = nb * (nb + 1) / 2;  // blocks of the lower triangle, numbered block-row after block-row

  for (int b = blockIdx.x; b < rows; b += gridDim.x) {
    const int row_begin = indptr[b], row_end = indptr[b + 1];
    if (tid == 0) *flag = 0;
    // ---- A = YtY + reg I + sum (|c| - 1) y y^T in register blocks; the row is staged once per round of blocks ----------------
    for (int round0 = 0; round0 < n_blocks; round0 += 256 * kExplainBlocks) {
      float acc[kExplainBlocks][4][4];
      int bi[kExplainBlocks], bj[kExplainBlocks];
#pragma unroll
      for (int q = 0; q < kExplainBlocks; ++q) {
        const int blk = round0 + tid + 256 * q;
        bi[q] = bj[q] = -1;
        if (blk < n_blocks) {
          int r = (int)((sqrtf(8.f * (float)blk + 1.f) - 1.f) * 0.5f);
          while (r * (r + 1) / 2 > blk) --r;
          while ((r + 1) * (r + 2) / 2 <= blk) ++r;
          bi[q] = r, bj[q] = blk - r * (r + 1) / 2;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const int i = 4 * bi[q] + r, j = 4 * bj[q] + c;
            acc[q][r][c] = (bi[q] >= 0 && i < f && j <= i) ? YtY[(size_t)i * f + j] + (i == j ? reg : 0.f) : 0.f;
          }
      }
      for (int k0 = row_begin; k0 < row_end; k0 += kExplainTile) {
        const int cnt = min(kExplainTile, row_end - k0);
        __syncthreads();  // the previous tile has been consumed
        for (int e = tid; e < kExplainTile * FS; e += 256) {
          const int t = e / FS, c = e - t * FS;
          float yv = 0.f, uv = 0.f;
          if (t < cnt && c < f) {
            yv = Y[(size_t)indices[k0 + t] * f + c];
            uv = (fabsf(data[k0 + t]) - 1.f) * yv;
          }
          yt[e] = yv;
          ut[e] = uv;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kExplainBlocks; ++q) {
          if (bi[q] < 0) continue;
#pragma unroll
          for (int t = 0; t < kExplainTile; ++t) {
            const float4 u4 = *reinterpret_cast<const float4 *>(ut + t * FS + 4 * bi[q]);
            const float4 y4 = *reinterpret_cast<const float4 *>(yt + t * FS + 4 * bj[q]);
            const float uu[4] = {u4.x, u4.y, u4.z, u4.w}, yy[4] = {y4.x, y4.y, y4.z, y4.w};
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
              for (int c = 0; c < 4; ++c) acc[q][r][c] = fmaf(uu[r], yy[c], acc[q][r][c]);
          }
        }
      }
#pragma unroll
      for (int q = 0; q < kExplainBlocks; ++q) {
        if (bi[q] < 0) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const int i = 4 * bi[q] + r, j = 4 * bj[q] + c;
            if (i < f && j <= i) A[tri_at(i, j)] = acc[q][r][c];
          }
      }
    }
    __syncthreads();

    // ---- left-looking Cholesky: column j of L from the finished columns before it; thread i owns row i (f <= 256) --------------
    bool failed = false;
    for (int j = 0; j < f; ++j) {
      float s = 0.f;
      if (tid >= j && tid < f) {
        const float *ri = A + tri_at(tid, 0), *rj = A + tri_at(j, 0);
        s = ri[j];
        for (int k = 0; k < j; ++k) s = fmaf(-ri[k], rj[k], s);
        if (tid == j) {
          if (s > 0.f) A[tri_at(j, j)] = sqrtf(s);
          else *flag = 1;
        }
      }
      __syncthreads();
      if (*flag) {  // uniform
        failed = true;
        break;
      }
      if (tid > j && tid < f) A[tri_at(tid, j)] = s / A[tri_at(j, j)];
      __syncthreads();
    }
    if (failed) {
      if (tid == 0) atomicMin(failed_row, (unsigned long long)b);
      __syncthreads();  // the flag is reset behind it
      continue;
    }
    // ---- L, dense with zeros above the diagonal, into rows [b f, (b + 1) f) of W ----------------------------------------------
    float *Wb = W + (size_t)b * f * f;
    for (int e = tid; e < f * f; e += 256) {
      const int i = e / f, j = e - i * f;
      Wb[e] = j <= i ? A[tri_at(i, j)] : 0.f;
    }
    __syncthreads();
  }
}

// ---- contribution kernel --------------------------------------------------------------------------------------------------------
// Sortable key of a contribution: the score's bits mapped so that unsigned order = float order, then the item id + 1 (so that no
// valid key is 0, the mark of an entry that contributes nothing).  Unsigned key order = (score, id) order.
// (Not select_ops.h's key: this one stores id + 1, keeps -0.0 distinct from +0.0 and breaks ties by position; golden files pin it.)
__device__ __forceinline__ key_t64 make_key(float score, int id) {
  unsigned u = __builtin_bit_cast(unsigned, score);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((key_t64)u << 32) | (unsigned)(id + 1);
}
__device__ __forceinline__ float key_score(key_t64 key) {
  unsigned u = (unsigned)(key >> 32);
  u = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
  return __builtin_bit_cast(float, u);
}
__device__ __forceinline__ int key_id(key_t64 key) { return (int)(unsigned)(key & 0xFFFFFFFFu) - 1; }

__global__ __launch_bounds__(256) void explain_contrib_kernel(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                              const float *__restrict__ data, const float *__restrict__ Y,
                                                              const float *__restrict__ W, const int32_t *__restrict__ itemids,
                                                              int items_per_row, long pairs, int f, int n, float *__restrict__ total_out,
                                                              int32_t *__restrict__ ids_out, float *__restrict__ scores_out,
                                                              key_t64 *__restrict__ ws, size_t ws_stride) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int FS = 4 * ((f + 3) >> 2);
  key_t64 *lds_keys = reinterpret_cast<key_t64 *>(smem);                       // [kKeysLds]
  float *L = smem + 2 * kKeysLds;                                               // packed lower triangle
  float *w = L + (((size_t)f * (f + 1) / 2 + 3) & ~(size_t)3);                  // [FS]
  float *red = w + FS;                                                          // [256]
  int *count = reinterpret_cast<int *>(red + 256);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  for (long p = blockIdx.x; p < pairs; p += gridDim.x) {
    const int b = (int)(p / items_per_row);
    const int item = itemids[p];
    const int row_begin = indptr[b], len = indptr[b + 1] - row_begin;
    const float *Wb = W + (size_t)b * f * f;
    for (int e = tid; e < f * f; e += 256) {
      const int i = e / f, j = e - i * f;
      if (j <= i) L[tri_at(i, j)] = Wb[e];
    }
    if (tid == 0) *count = 0;
    __syncthreads();
    // ---- w = L^-T L^-1 y_item by one wavefront; lane l owns elements l + 64 m ------------------------------------------------
    if (wave == 0) {
      float z[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int i = lane + 64 * m;
        z[m] = i < f ? Y[(size_t)item * f + i] : 0.f;
      }
      for (int k = 0; k < f; ++k) {  // L z = y, column by column
        float zk = 0.f;
#pragma unroll
        for (int m = 0; m < 4; ++m)
          if ((k >> 6) == m) zk = lane_bcast(z[m], k & 63);
        zk = zk / L[tri_at(k, k)];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          const int i = lane + 64 * m;
          if (i > k && i < f) z[m] = fmaf(-L[tri_at(i, k)], zk, z[m]);
          if (i == k) z[m] = zk;
        }
      }
      for (int k = f - 1; k >= 0; --k) {  // L^T w = z, row k of L is column k of L^T
        float wk = 0.f;
#pragma unroll
        for (int m = 0; m < 4; ++m)
          if ((k >> 6) == m) wk = lane_bcast(z[m], k & 63);
        wk = wk / L[tri_at(k, k)];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          const int i = lane + 64 * m;
          if (i < k) z[m] = fmaf(-L[tri_at(k, i)], wk, z[m]);
          if (i == k) z[m] = wk;
        }
      }
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int i = lane + 64 * m;
        if (i < FS) w[i] = i < f ? z[m] : 0.f;
      }
    }
    __syncthreads();
    // ---- s_j = c_j (w . y_j): one wavefront per entry, the same instruction sequence whichever wavefront or position -----------
    key_t64 *keys = len <= kKeysLds ? lds_keys : ws + (size_t)blockIdx.x * ws_stride;
    for (int e = wave; e < len; e += 4) {
      const int j = indices[row_begin + e];
      const float c = data[row_begin + e];
      float part = 0.f;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int i = lane + 64 * m;
        if (i < f) part = fmaf(w[i], Y[(size_t)j * f + i], part);
      }
      const float s = c * wave_allsum(part);
      if (lane == 0) keys[e] = c > 0.f ? make_key(s, j) : 0;
    }
    __syncthreads();
    // ---- total: thread t sums entries t, t + 256, ... in order, then a fixed tree over the threads ------------------------------
    float t = 0.f;
    int mine = 0;
    for (int e = tid; e < len; e += 256) {
      const key_t64 key = keys[e];
      if (key) t += key_score(key), ++mine;
    }
    red[tid] = t;
    if (mine) atomicAdd(count, mine);  // an integer count: order-independent
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
      if (tid < h) red[tid] += red[tid + h];
      __syncthreads();
    }
    if (tid == 0) total_out[p] = red[0];
    // ---- the N best: an entry's rank is the number of entries ahead of it in (score, id) order; equal keys by position ---------
    int32_t *ids_p = ids_out + (size_t)p * n;
    float *scores_p = scores_out + (size_t)p * n;
    for (int r = min(*count, n) + tid; r < n; r += 256) ids_p[r] = -1, scores_p[r] = -FLT_MAX;
    for (int e = tid; e < len; e += 256) {
      const key_t64 key = keys[e];
      if (!key) continue;
      int rank = 0;
      for (int e2 = 0; e2 < len; ++e2) {
        const key_t64 other = keys[e2];
        rank += (other > key || (other == key && e2 < e)) ? 1 : 0;
      }
      if (rank < n) ids_p[rank] = key_id(key), scores_p[rank] = key_score(key);
    }
    __syncthreads();  // the LDS is reused by the next pair
  }
}

static void check_explain_args(const imp_csr *C, const imp_matrix *Y, const imp_matrix *weights, const char *who) {
  const std::string name(who);
  if (!C->parts.empty()) throw std::invalid_argument(name + ": a matrix of more than 2^31 - 1 nonzeros is not supported");
  if (Y->itemsize != 4) throw std::invalid_argument(name + ": Y must be float32 (convert a float16 model first)");
  if (Y->cols < 1 || Y->cols > (size_t)kExplainMaxF)
    throw std::invalid_argument(name + ": factors must be in 1 .. " + std::to_string(kExplainMaxF) + " (the triangle is kept in the LDS), got " +
                                std::to_string(Y->cols));
  if ((size_t)C->cols > Y->rows) throw std::invalid_argument(name + ": Dimensionality mismatch between cols of Cui and rows of Y");
  if (weights->itemsize != 4) throw std::invalid_argument(name + ": weights must be float32");
  if (weights->cols != Y->cols || weights->rows != (size_t)C->rows * Y->cols)
    throw std::invalid_argument(name + ": weights must have Cui.rows * factors rows and factors columns, got " +
                                std::to_string(weights->rows) + " x " + std::to_string(weights->cols));
}

int64_t explain_factor(const imp_csr *C, const imp_matrix *YtY, const imp_matrix *Y, double reg, imp_matrix *weights) {
  const int f = (int)Y->cols;
  if (C->rows == 0) return -1;
  unsigned long long *g_failed = reset_fail_word();
  const size_t lds = factor_lds_bytes(f);
  const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(8, (160 * 1024) / lds));
  const int grid = std::min(C->rows, ctx().num_cus * per_cu * 4);
  allow_dynamic_lds(explain_factor_kernel, lds);
  {
    IMP_PROF("explain_factor");
    explain_factor_kernel<<<grid, 256, lds, stream()>>>(C->indptr.data(), C->indices.data(), C->data.data(), C->rows, Y->f32(),
                                                        YtY->f32(), f, (float)reg, weights->mut<float>(), g_failed);
    IMP_CHECK_HIP(hipGetLastError());
  }
  return read_fail_word(g_failed);
}

void explain_contributions(const imp_csr *C, const imp_matrix *Y, const imp_matrix *weights, const imp_intvector *itemids,
                           int items_per_row, int n, float *total, int32_t *ids, float *scores) {
  const int f = (int)Y->cols;
  const size_t pairs = (size_t)C->rows * items_per_row;
  if (pairs == 0) return;
  // host copies of the ids (range check) and of the row offsets (the longest row sizes the workspace); neither is a launch
  std::vector<int32_t> h_items(pairs), h_indptr((size_t)C->rows + 1);
  IMP_CHECK_HIP(hipMemcpyAsync(h_items.data(), itemids->v.data(), pairs * sizeof(int32_t), hipMemcpyDeviceToHost, stream()));
  IMP_CHECK_HIP(hipMemcpyAsync(h_indptr.data(), C->indptr.data(), h_indptr.size() * sizeof(int32_t), hipMemcpyDeviceToHost, stream()));
  sync();
  for (size_t p = 0; p < pairs; ++p)
    if (h_items[p] < 0 || (size_t)h_items[p] >= Y->rows)
      throw std::invalid_argument("explain: item id " + std::to_string(h_items[p]) + " (pair " + std::to_string(p) +
                                  ") is outside the item factors (" + std::to_string(Y->rows) + " rows)");
  int32_t longest = 0;
  for (int32_t r = 0; r < C->rows; ++r) longest = std::max(longest, h_indptr[r + 1] - h_indptr[r]);
  // one workgroup per pair up to four per CU; rows beyond the LDS key buffer: a slice of `longest` keys per WORKGROUP, and fewer
  // workgroups when the slices would pass 256 MB
  int grid = (int)std::min<size_t>(pairs, (size_t)ctx().num_cus * 4);
  DeviceArray<key_t64> ws;
  size_t ws_stride = 0;
  if (longest > kKeysLds) {
    ws_stride = ((size_t)longest + 1) & ~(size_t)1;
    grid = (int)std::max<size_t>(1, std::min<size_t>(grid, ((size_t)256 << 20) / (ws_stride * sizeof(key_t64))));
    ws.alloc(ws_stride * (size_t)grid);
  }
  DeviceArray<float> d_total, d_scores;
  DeviceArray<int32_t> d_ids;
  d_total.alloc(pairs);
  d_scores.alloc(pairs * (size_t)n);
  d_ids.alloc(pairs * (size_t)n);
  const size_t lds = contrib_lds_bytes(f);
  allow_dynamic_lds(explain_contrib_kernel, lds);
  {
    IMP_PROF("explain_contributions");
    explain_contrib_kernel<<<grid, 256, lds, stream()>>>(C->indptr.data(), C->indices.data(), C->data.data(), Y->f32(), weights->f32(),
                                                         itemids->v.data(), items_per_row, (long)pairs, f, n, d_total.data(),
                                                         d_ids.data(), d_scores.data(), ws.data(), ws_stride);
    IMP_CHECK_HIP(hipGetLastError());
  }
  IMP_CHECK_HIP(hipMemcpyAsync(total, d_total.data(), pairs * sizeof(float), hipMemcpyDeviceToHost, stream()));
  IMP_CHECK_HIP(hipMemcpyAsync(ids, d_ids.data(), pairs * (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, stream()));
  IMP_CHECK_HIP(hipMemcpyAsync(scores, d_scores.data(), pairs * (size_t)n * sizeof(float), hipMemcpyDeviceToHost, stream()));
  sync();
}

}  // namespace imp

using namespace imp;

extern "C" {

int imp_solver_explain_factor(imp_solver *, const imp_csr *cui, const imp_matrix *YtY, const imp_matrix *Y, double regularization,
                              imp_matrix *weights, int64_t *failed_row) {
  return guarded([&] {
    if (failed_row) *failed_row = -1;
    check_explain_args(cui, Y, weights, "explain_factor");
    if (YtY->itemsize != 4) throw std::invalid_argument("explain_factor: YtY must be float32");
    if (YtY->rows != YtY->cols || YtY->cols != Y->cols)
      throw std::invalid_argument("explain_factor: YtY must be square with as many columns as Y");
    const int64_t failed = explain_factor(cui, YtY, Y, regularization, weights);
    if (failed_row) *failed_row = failed;
    if (failed >= 0)
      throw std::invalid_argument("cholesky factorisation failed on row " + std::to_string(failed) +
                                  ". Try increasing the regularization parameter.");
  });
}

int imp_solver_explain(imp_solver *, const imp_csr *cui, const imp_matrix *Y, const imp_matrix *weights, const imp_intvector *itemids,
                       int items_per_row, int n, float *total, int32_t *ids, float *scores) {
  return guarded([&] {
    check_explain_args(cui, Y, weights, "explain");
    if (items_per_row < 1) throw std::invalid_argument("explain: items_per_row must be >= 1");
    if (n < 1) throw std::invalid_argument("explain: n must be >= 1");
    if (itemids->size != (size_t)cui->rows * (size_t)items_per_row)
      throw std::invalid_argument("explain: itemids must hold Cui.rows * items_per_row ids, got " + std::to_string(itemids->size));
    explain_contributions(cui, Y, weights, itemids, items_per_row, n, total, ids, scores);
  });
}

}  // extern "C"
