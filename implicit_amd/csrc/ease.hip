// K16b: the sparse and serving parts of EASE: imp_ease_gram, imp_ease_weights, imp_ease_topk.  The dense inverse
// between the first two is spd_inverse.hip.  No floating-point atomics: equal inputs give bitwise equal outputs.
//
// ease_gram_kernel    G = X^T X + reg I.  One workgroup per (output row i, slab of kGramSlab columns at or left of i): it walks
//   item_users[i] in stored order; for user u its threads take the entries (j, x_uj) of user_items[u] inside the slab with
//   j <= i and add x_ui * x_uj (product and sum rounded separately) to an accumulator of the slab in the LDS.  A user row holds
//   no column twice, so the threads of a step never meet; a workgroup barrier orders the steps, so every G[i][j] is the sum over
//   the co-occurring users in item_users[i]'s order.  The users of a batch of 256 are staged in the LDS and the first 256
//   entries of the next user are fetched during the current step.  The diagonal takes + reg last; mirror_lower fills j > i.
// ease_weights        B[i][j] = -(P[i][j] / P[j][j]), B[j][j] = 0 in place: the diagonal is checked and copied aside first.
// ease_score_kernel   grid (query row, slab of kSlabCols columns): a thread owns 8 columns 256 apart and walks the row's entries
//   in stored order, s = s + x * B[i][c], reading B[i, slab] coalesced; filtered columns (the row's own, the item filter's) become
//   -FLT_MAX and stay candidates; the slab's keys (select_ops.h) are sorted in the LDS and its best min(topk, kSlabCols) go to a
//   scratch.  ease_merge_kernel: one workgroup per row finds the min(topk, items) largest of the row's slab winners by the
//   byte-wise radix select, sorts them in the LDS and writes ids and scores, padded with (-1, -FLT_MAX).
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "common.h"
#include "select_ops.h"
#include "spd_inverse.h"

namespace imp {

namespace {
constexpr int kGramSlab = 16384;  // fp32 accumulators of one workgroup (64 KiB of LDS)
constexpr int kSlabCols = 2048, kEaseBlock = 256, kEaseColsPerThread = kSlabCols / kEaseBlock;
constexpr int kEaseMaxTopk = 1024;

__global__ __launch_bounds__(256) void ease_gram_kernel(const int32_t *__restrict__ iu_ptr, const int32_t *__restrict__ iu_idx,
                                                        const float *__restrict__ iu_val, const int32_t *__restrict__ ui_ptr,
                                                        const int32_t *__restrict__ ui_idx, const float *__restrict__ ui_val,
                                                        int items, float reg, float *__restrict__ G) {
  extern __shared__ float gram_acc[];  // [kGramSlab]
  __shared__ float s_w[256];
  __shared__ int s_q0[256], s_q1[256];
  const int i = blockIdx.x, c0 = blockIdx.y * kGramSlab;
  if (c0 > i) return;
  const int c1 = min(i + 1, c0 + kGramSlab), tid = threadIdx.x;
  for (int t = tid; t < c1 - c0; t += 256) gram_acc[t] = 0.f;
  const int p0 = iu_ptr[i], p1 = iu_ptr[i + 1];
  for (int pb = p0; pb < p1; pb += 256) {
    __syncthreads();  // the previous batch has been consumed (and, the first time, the accumulators are zero)
    if (pb + tid < p1) {
      const int u = iu_idx[pb + tid];
      s_w[tid] = iu_val[pb + tid];
      s_q0[tid] = ui_ptr[u];
      s_q1[tid] = ui_ptr[u + 1];
    }
    __syncthreads();
    const int cnt = min(256, p1 - pb);
    int jn = -1;
    float vn = 0.f;
    if (s_q0[0] + tid < s_q1[0]) jn = ui_idx[s_q0[0] + tid], vn = ui_val[s_q0[0] + tid];
    for (int e = 0; e < cnt; ++e) {
      const float w = s_w[e];
      const int q0 = s_q0[e], q1 = s_q1[e];
      const int j = jn;
      const float v = vn;
      jn = -1;
      if (e + 1 < cnt && s_q0[e + 1] + tid < s_q1[e + 1]) jn = ui_idx[s_q0[e + 1] + tid], vn = ui_val[s_q0[e + 1] + tid];
      if (j >= c0 && j < c1) gram_acc[j - c0] = gram_acc[j - c0] + w * v;
      for (int q = q0 + 256 + tid; q < q1; q += 256) {
        const int jq = ui_idx[q];
        if (jq >= c0 && jq < c1) gram_acc[jq - c0] = gram_acc[jq - c0] + w * ui_val[q];
      }
      __syncthreads();
    }
  }
  __syncthreads();
  for (int t = tid; t < c1 - c0; t += 256) {
    const int c = c0 + t;
    G[(size_t)i * items + c] = c == i ? gram_acc[t] + reg : gram_acc[t];
  }
}

// bad[0] |= 1 where the diagonal is zero or not finite; diag = a copy of it
__global__ void ease_diag_kernel(const float *__restrict__ P, long n, float *__restrict__ diag, int *__restrict__ bad) {
  const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const float d = P[j * n + j];
  diag[j] = d;
  if (d == 0.f || !isfinite(d)) atomicOr(bad, 1);
}

__global__ void ease_weights_kernel(float *__restrict__ P, long n, const float *__restrict__ diag) {
  const long c = (long)blockIdx.y * blockDim.x + threadIdx.x, r = blockIdx.x;
  if (c >= n) return;
  P[r * n + c] = r == c ? 0.f : -(P[r * n + c] / diag[c]);
}

__global__ void ease_filter_bits_kernel(const int32_t *__restrict__ ids, size_t n, unsigned int *__restrict__ bits) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) atomicOr(&bits[ids[t] >> 5], 1u << (ids[t] & 31));
}

// indptr: the chunk's rows + 1 offsets relative to its first entry; scratch: [row][slab][kk] keys, 0 = no key
__global__ __launch_bounds__(kEaseBlock) void ease_score_kernel(const float *__restrict__ B, int items, const int64_t *__restrict__ indptr,
                                                                const int32_t *__restrict__ idx, const float *__restrict__ val, int kk,
                                                                int filter_liked, const unsigned int *__restrict__ filter_bits,
                                                                uint64_t *__restrict__ scratch) {
  __shared__ __attribute__((aligned(16))) uint64_t keys[kSlabCols];
  __shared__ float sc[kSlabCols];
  __shared__ int e_i[kEaseBlock];
  __shared__ float e_x[kEaseBlock];
  const int tid = threadIdx.x, c0 = blockIdx.y * kSlabCols;
  const size_t row = blockIdx.x;
  const int64_t p0 = indptr[row], p1 = indptr[row + 1];
  float s[kEaseColsPerThread];
  int cc[kEaseColsPerThread];  // a column past the matrix reads the last one and is dropped below
#pragma unroll
  for (int q = 0; q < kEaseColsPerThread; ++q) s[q] = 0.f, cc[q] = min(c0 + tid + kEaseBlock * q, items - 1);
  for (int64_t pb = p0; pb < p1; pb += kEaseBlock) {
    __syncthreads();
    if (pb + tid < p1) e_i[tid] = idx[pb + tid], e_x[tid] = val[pb + tid];
    __syncthreads();
    const int cnt = (int)min((int64_t)kEaseBlock, p1 - pb);
#pragma unroll 2
    for (int e = 0; e < cnt; ++e) {
      const float x = e_x[e];
      const float *brow = B + (size_t)e_i[e] * items;
#pragma unroll
      for (int q = 0; q < kEaseColsPerThread; ++q) s[q] = s[q] + x * brow[cc[q]];
    }
  }
#pragma unroll
  for (int q = 0; q < kEaseColsPerThread; ++q) {
    const int col = c0 + tid + kEaseBlock * q;
    float v = s[q];
    if (filter_bits && col < items && ((filter_bits[col >> 5] >> (col & 31)) & 1u)) v = -FLT_MAX;
    sc[tid + kEaseBlock * q] = v;
  }
  __syncthreads();
  if (filter_liked) {
    for (int64_t p = p0 + tid; p < p1; p += kEaseBlock) {
      const int c = idx[p] - c0;
      if (c >= 0 && c < kSlabCols) sc[c] = -FLT_MAX;
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < kEaseColsPerThread; ++q) {
    const int c = tid + kEaseBlock * q;
    keys[c] = c0 + c < items ? make_key(sc[c], c0 + c) : 0ull;
  }
  __syncthreads();
  block_sort_desc<kEaseBlock>(keys, kSlabCols);
  uint64_t *out = scratch + (row * gridDim.y + blockIdx.y) * (size_t)kk;
  for (int t = tid; t < kk; t += kEaseBlock) out[t] = keys[t];
}

// total = slabs * kk keys per row (0 = none), of which at least want = min(topk, items) are real and all real ones distinct
__global__ __launch_bounds__(kEaseBlock) void ease_merge_kernel(const uint64_t *__restrict__ scratch, int total, int want, int topk,
                                                                int32_t *__restrict__ ids, float *__restrict__ scores) {
  __shared__ __attribute__((aligned(16))) uint64_t lk[kEaseMaxTopk];
  __shared__ unsigned int hist[256], words[5];
  const int tid = threadIdx.x;
  const uint64_t *in = scratch + (size_t)blockIdx.x * total;
  uint64_t prefix = 0, mask = 0;
  unsigned int remaining = (unsigned int)want;
  auto each_key = [&](auto &&body) {
    for (int e = tid; e < total; e += kEaseBlock) {
      const uint64_t key = in[e];
      if (key) body(key);
    }
  };
  for (int shift = 56; shift >= 0; shift -= 8)
    if (radix_select_digit<kEaseBlock, uint64_t>(each_key, shift, prefix, mask, remaining, hist, &words[0], &words[1], &words[2])) break;
  // (key & mask) > prefix: winners; == prefix: the boundary bucket, of which `remaining` are wanted (all of it when the select
  // stopped early; after the last digit it holds one key)
  if (tid == 0) words[3] = 0, words[4] = 0;
  __syncthreads();
  for (int e = tid; e < total; e += kEaseBlock) {
    const uint64_t key = in[e];
    if (!key) continue;
    const uint64_t head = key & mask;
    bool take = head > prefix;
    if (head == prefix) take = atomicAdd(&words[4], 1u) < remaining;
    if (take) {
      const unsigned int slot = atomicAdd(&words[3], 1u);
      if (slot < (unsigned int)kEaseMaxTopk) lk[slot] = key;
    }
  }
  __syncthreads();
  int np2 = 2;
  while (np2 < want) np2 <<= 1;
  for (int e = want + tid; e < np2; e += kEaseBlock) lk[e] = 0;
  __syncthreads();
  block_sort_desc<kEaseBlock>(lk, np2);
  int32_t *ids_r = ids + (size_t)blockIdx.x * topk;
  float *scores_r = scores + (size_t)blockIdx.x * topk;
  for (int j = tid; j < topk; j += kEaseBlock) {
    ids_r[j] = j < want ? key_id(lk[j]) : -1;
    scores_r[j] = j < want ? key_score(lk[j]) : -FLT_MAX;
  }
}

struct EaseCall {
  const imp_matrix *B;
  const int64_t *indptr;
  const int32_t *indices;
  const float *data;
  int topk, filter_liked, slabs, kk;
  const unsigned int *filter_bits;
  int32_t *ids;
  float *scores;
};

size_t ease_row_bytes(const EaseCall &c, size_t r) {
  const size_t len = (size_t)(c.indptr[r + 1] - c.indptr[r]);
  return len * (sizeof(int32_t) + sizeof(float)) + sizeof(int64_t) + (size_t)c.slabs * c.kk * sizeof(uint64_t) +
         (size_t)c.topk * (sizeof(int32_t) + sizeof(float));
}

void ease_chunk(const EaseCall &c, size_t r0, size_t r1) {
  const size_t rows = r1 - r0;
  const int items = (int)c.B->rows;
  const int64_t e0 = c.indptr[r0], ne = c.indptr[r1] - e0;
  std::vector<int64_t> h_ptr(rows + 1);
  for (size_t r = 0; r <= rows; ++r) h_ptr[r] = c.indptr[r0 + r] - e0;
  DeviceArray<int64_t> d_ptr;
  DeviceArray<int32_t> d_idx, d_ids;
  DeviceArray<float> d_val, d_scores;
  DeviceArray<uint64_t> d_scratch;
  d_ptr.upload(h_ptr.data(), rows + 1);
  d_idx.upload(c.indices + e0, (size_t)ne);
  d_val.upload(c.data + e0, (size_t)ne);
  d_scratch.alloc(rows * c.slabs * (size_t)c.kk);
  d_ids.alloc(rows * (size_t)c.topk);
  d_scores.alloc(rows * (size_t)c.topk);
  {
    IMP_PROF("ease_score");
    ease_score_kernel<<<dim3((unsigned)rows, (unsigned)c.slabs), kEaseBlock, 0, stream()>>>(
        c.B->f32(), items, d_ptr.data(), d_idx.data(), d_val.data(), c.kk, c.filter_liked, c.filter_bits, d_scratch.data());
    IMP_CHECK_HIP(hipGetLastError());
  }
  {
    IMP_PROF("ease_merge");
    ease_merge_kernel<<<(unsigned)rows, kEaseBlock, 0, stream()>>>(d_scratch.data(), c.slabs * c.kk, std::min(c.topk, items), c.topk,
                                                                  d_ids.data(), d_scores.data());
    IMP_CHECK_HIP(hipGetLastError());
  }
  IMP_CHECK_HIP(hipMemcpyAsync(c.ids + r0 * (size_t)c.topk, d_ids.data(), rows * (size_t)c.topk * sizeof(int32_t), hipMemcpyDeviceToHost, stream()));
  IMP_CHECK_HIP(hipMemcpyAsync(c.scores + r0 * (size_t)c.topk, d_scores.data(), rows * (size_t)c.topk * sizeof(float), hipMemcpyDeviceToHost, stream()));
  sync();  // the host vector and the device arrays of the chunk die here
}
}  // namespace

}  // namespace imp

using namespace imp;

extern "C" int imp_ease_gram(const imp_csr *item_users, const imp_csr *user_items, float regularization, imp_matrix *G) {
  return guarded([&] {
    if (!item_users || !user_items || !G) throw std::invalid_argument("ease_gram: NULL argument");
    if (!item_users->parts.empty() || !user_items->parts.empty() || item_users->nnz > INT32_MAX || user_items->nnz > INT32_MAX)
      throw std::invalid_argument("ease_gram: more than 2^31-1 nonzeros is not supported");
    if (item_users->rows != user_items->cols || item_users->cols != user_items->rows || item_users->nnz != user_items->nnz)
      throw std::invalid_argument("ease_gram: item_users and user_items must be the two orientations of one matrix");
    const size_t items = (size_t)item_users->rows;
    if (G->itemsize != 4 || G->rows != items || G->cols != items) throw std::invalid_argument("ease_gram: G must be float32, items x items");
    if (items == 0) return;
    IMP_PROF("ease_gram");
    float *const g = G->mut<float>();
    allow_dynamic_lds_once<ease_gram_kernel>(kGramSlab * sizeof(float));
    const unsigned slabs = (unsigned)((items + kGramSlab - 1) / kGramSlab);
    ease_gram_kernel<<<dim3((unsigned)items, slabs), 256, kGramSlab * sizeof(float), stream()>>>(
        item_users->indptr.data(), item_users->indices.data(), item_users->data.data(), user_items->indptr.data(),
        user_items->indices.data(), user_items->data.data(), (int)items, regularization, g);
    IMP_CHECK_HIP(hipGetLastError());
    mirror_lower(g, items);
    sync();
  });
}

extern "C" int imp_ease_weights(imp_matrix *P) {
  return guarded([&] {
    if (!P) throw std::invalid_argument("ease_weights: NULL matrix");
    if (P->itemsize != 4 || P->rows != P->cols) throw std::invalid_argument("ease_weights: the matrix must be square float32");
    const size_t n = P->rows;
    if (n == 0) return;
    if (n > (size_t)INT32_MAX) throw std::invalid_argument("ease_weights: too many items");
    IMP_PROF("ease_weights");
    DeviceArray<float> diag;
    DeviceArray<int> bad;
    diag.alloc(n);
    bad.alloc(1, true);
    ease_diag_kernel<<<(unsigned)((n + 255) / 256), 256, 0, stream()>>>(P->f32(), (long)n, diag.data(), bad.data());
    IMP_CHECK_HIP(hipGetLastError());
    int h_bad = 0;
    IMP_CHECK_HIP(hipMemcpyAsync(&h_bad, bad.data(), sizeof(int), hipMemcpyDeviceToHost, stream()));
    sync();
    if (h_bad) throw std::invalid_argument("ease_weights: a diagonal entry is zero or not finite");
    ease_weights_kernel<<<dim3((unsigned)n, (unsigned)((n + 255) / 256)), 256, 0, stream()>>>(P->mut<float>(), (long)n, diag.data());
    IMP_CHECK_HIP(hipGetLastError());
    sync();
  });
}

extern "C" int imp_ease_topk(imp_knn *knn, const imp_matrix *B, int32_t rows, const int64_t *indptr, const int32_t *indices,
                             const float *data, int topk, int filter_liked, const imp_intvector *item_filter, int32_t *ids,
                             float *scores) {
  return guarded([&] {
    if (!knn || !B) throw std::invalid_argument("ease_topk: NULL handle");
    if (B->itemsize != 4 || B->rows != B->cols || B->rows < 1 || B->rows > (size_t)INT32_MAX - kSlabCols)
      throw std::invalid_argument("ease_topk: B must be a square float32 matrix of at least one item");
    if (topk < 1 || topk > kEaseMaxTopk) throw std::invalid_argument("ease_topk: topk must lie in 1 .. " + std::to_string(kEaseMaxTopk));
    if (rows < 0) throw std::invalid_argument("ease_topk: negative row count");
    if (rows == 0) return;
    if (!indptr || !ids || !scores) throw std::invalid_argument("ease_topk: NULL array");
    if (indptr[0] != 0) throw std::invalid_argument("ease_topk: indptr must start at 0");
    const int items = (int)B->rows;
    for (int32_t r = 0; r < rows; ++r) {
      if (indptr[r + 1] < indptr[r]) throw std::invalid_argument("ease_topk: indptr decreases at row " + std::to_string(r));
      if (indptr[r + 1] > indptr[r] && (!indices || !data)) throw std::invalid_argument("ease_topk: NULL array");
      for (int64_t e = indptr[r]; e < indptr[r + 1]; ++e) {
        if (indices[e] < 0 || indices[e] >= items)
          throw std::invalid_argument("ease_topk: column " + std::to_string(indices[e]) + " of row " + std::to_string(r) +
                                      " is outside the model (" + std::to_string(items) + " items)");
        if (e > indptr[r] && indices[e] <= indices[e - 1])
          throw std::invalid_argument("ease_topk: row " + std::to_string(r) + " is not strictly increasing");
      }
    }
    DeviceArray<unsigned int> bits;
    if (item_filter && item_filter->size) {
      std::vector<int32_t> h(item_filter->size);
      IMP_CHECK_HIP(hipMemcpyAsync(h.data(), item_filter->v.data(), h.size() * sizeof(int32_t), hipMemcpyDeviceToHost, stream()));
      sync();
      for (int32_t id : h)
        if (id < 0 || id >= items) throw std::invalid_argument("ease_topk: item_filter id " + std::to_string(id) + " is outside the model");
    }
    const int slabs = (items + kSlabCols - 1) / kSlabCols;
    EaseCall c{B, indptr, indices, data, topk, filter_liked ? 1 : 0, slabs, std::min(topk, kSlabCols), nullptr, ids, scores};
    const size_t budget = knn_temp_budget(knn);
    for (int32_t r = 0; r < rows; ++r) {
      const size_t need = ease_row_bytes(c, r);
      if (need > budget)
        throw std::invalid_argument("ease_topk: row " + std::to_string(r) + " alone needs " + std::to_string(need) +
                                    " bytes of temporaries, max_temp_memory is " + std::to_string(budget));
    }
    if (item_filter && item_filter->size) {
      bits.alloc((size_t)(items + 31) / 32, true);
      ease_filter_bits_kernel<<<(unsigned)((item_filter->size + 255) / 256), 256, 0, stream()>>>(item_filter->v.data(), item_filter->size, bits.data());
      IMP_CHECK_HIP(hipGetLastError());
      c.filter_bits = bits.data();
    }
    for (size_t r0 = 0; r0 < (size_t)rows;) {  // greedy chunks of whole rows
      size_t r1 = r0, bytes = 0;
      while (r1 < (size_t)rows) {
        const size_t b = ease_row_bytes(c, r1);
        if (r1 > r0 && bytes + b > budget) break;
        bytes += b, ++r1;
      }
      ease_chunk(c, r0, r1);
      r0 = r1;
    }
  });
}
